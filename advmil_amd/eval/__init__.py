from .cindex import concordance_index, concordance_index_censored, NoComparablePairException  # noqa: F401
from .evaluator import ContSurv_Evaluator, DiscSurv_Evaluator, CoxSurv_Evaluator  # noqa: F401
from .utils import prepare_evaluator  # noqa: F401
