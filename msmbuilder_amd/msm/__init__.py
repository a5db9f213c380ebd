"""Post-clustering MSM step: ``_transition_counts`` and ``MarkovStateModel`` as in ``msmbuilder.msm``."""
from .core import _transition_counts  # noqa: F401
from .msm import MarkovStateModel  # noqa: F401

__all__ = ['_transition_counts', 'MarkovStateModel']
