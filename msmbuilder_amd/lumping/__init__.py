from .mvca import MVCA  # noqa: F401
