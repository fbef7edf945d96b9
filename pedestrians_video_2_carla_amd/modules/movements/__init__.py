from .lstm import LSTM  # noqa: F401
