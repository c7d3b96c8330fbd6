from .cindex import concordance_index, concordance_index_censored, NoComparablePairException  # noqa: F401
from .bootstrap import (bootstrap_concordance_index, bootstrap_concordance_samples, concordance_counts_weighted,  # noqa: F401
                        multiplicities, paired_bootstrap_concordance, resample_indices)
from .stratify import (kaplan_meier, logrank_from_rows, logrank_permutation_test, logrank_rows, logrank_scan, logrank_test,  # noqa: F401
                       permutation_groups, risk_groups, stratify)
from .timedep import (bootstrap_timedep, brier_score, cumulative_dynamic_auc, default_times, integrated_brier_score, ipcw_rows,  # noqa: F401
                      statistics_from_rows, survival_from_hazards, survival_from_samples)
from .concordance import (bootstrap_concordance, columns_at_own_times, concord_rows, concordance_ipcw, concordance_td,  # noqa: F401
                          surv_at_own_times)
from .calibration import (bootstrap_calibration, calib_rows, d_calibration, survival_at_own_time, time_error)  # noqa: F401
from .evaluator import ContSurv_Evaluator, DiscSurv_Evaluator, CoxSurv_Evaluator  # noqa: F401
from .utils import prepare_evaluator  # noqa: F401
