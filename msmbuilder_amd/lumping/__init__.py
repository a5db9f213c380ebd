from .mvca import MVCA  # noqa: F401
from .bace import BACE  # noqa: F401
from .pcca import PCCA  # noqa: F401
from .pcca_plus import PCCAPlus  # noqa: F401
