from .mvca import MVCA  # noqa: F401
from .bace import BACE  # noqa: F401
