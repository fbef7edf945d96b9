from .linear import Linear  # noqa: F401
from .lstm import LSTM  # noqa: F401
from .transformers import SimpleTransformer  # noqa: F401
