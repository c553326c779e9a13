"""dis_project_amd — MI355X-native drop-in for the GPJax hot path of wejpurvis/DIS_project:
the SIM latent-force-model covariance (src/model.py) and its Cholesky-based log marginal
likelihood (src/objectives.py), on hand-written gfx950 HIP kernels behind a ctypes C-ABI
(``liblfm.so``, declared in ``include/lfm.h``).
"""

from ._lib import LfmError, device_count, get_context, load_library  # noqa: F401
from .dataset import Dataset, SyntheticP53Data, dataset_3d  # noqa: F401
from .distributions import GaussianDistribution, randn, seed_to_u64  # noqa: F401
from .farm import MidBatchEvaluator  # noqa: F401
from .model import ExactLFM  # noqa: F401
from .objectives import CustomConjLOOCV, CustomConjMLL  # noqa: F401
from .predict import BatchPredictor, MidBatchPredictor, Posterior  # noqa: F401
from .trainer import MidBatchTrainer  # noqa: F401

__all__ = [
    "BatchPredictor",
    "CustomConjLOOCV",
    "CustomConjMLL",
    "Dataset",
    "ExactLFM",
    "GaussianDistribution",
    "LfmError",
    "MidBatchEvaluator",
    "MidBatchPredictor",
    "MidBatchTrainer",
    "Posterior",
    "SyntheticP53Data",
    "dataset_3d",
    "device_count",
    "get_context",
    "load_library",
    "randn",
    "seed_to_u64",
]
