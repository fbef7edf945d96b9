from .classification import ClassificationModel  # noqa: F401
from .gru import GRU  # noqa: F401
from .lstm import LSTM  # noqa: F401
