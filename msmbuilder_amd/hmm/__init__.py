"""Hidden Markov models (reference: msmbuilder/hmm): ``GaussianHMM`` and ``VonMisesHMM`` with their E-steps on the device."""
from .gaussian import GaussianHMM
from .vonmises import VonMisesHMM

__all__ = ['GaussianHMM', 'VonMisesHMM']
