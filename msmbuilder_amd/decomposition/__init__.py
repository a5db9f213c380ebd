"""Decompositions of the MSMBuilder hot path on MI355X (reference: msmbuilder/decomposition)."""
from .tica import tICA
from .kernel_approximation import Nystroem, LandmarkNystroem
from .ktica import KernelTICA
from .sparsetica import SparseTICA

__all__ = ['tICA', 'KernelTICA', 'SparseTICA', 'Nystroem', 'LandmarkNystroem']
