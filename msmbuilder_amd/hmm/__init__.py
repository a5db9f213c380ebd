"""Hidden Markov models (reference: msmbuilder/hmm): ``GaussianHMM`` with its E-step on the device."""
from .gaussian import GaussianHMM

__all__ = ['GaussianHMM']
