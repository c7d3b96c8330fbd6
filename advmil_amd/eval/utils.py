"""prepare_evaluator of the reference's eval/utils.py: the evaluator class for a model's output type."""
from .evaluator import ContSurv_Evaluator, CoxSurv_Evaluator, DiscSurv_Evaluator

_BY_OUTPUT = {"continuous": ContSurv_Evaluator, "discrete": DiscSurv_Evaluator, "prohazard": CoxSurv_Evaluator}


def prepare_evaluator(output_type, **kws):
    """'continuous' | 'discrete' | 'prohazard' -> an evaluator built from `kws`; any other output type -> None."""
    cls = _BY_OUTPUT.get(output_type)
    return cls(**kws) if cls is not None else None
