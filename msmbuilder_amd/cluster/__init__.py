"""Clusterers of the MSMBuilder hot path on MI355X (reference: msmbuilder/cluster/__init__.py)."""
from .base import MultiSequenceClusterMixin
from .kcenters import KCenters
from .kmeans import KMeans
from .minibatchkmeans import MiniBatchKMeans
from .regularspatial import RegularSpatial

__all__ = ['KCenters', 'KMeans', 'MiniBatchKMeans', 'RegularSpatial', 'MultiSequenceClusterMixin']
