"""Clusterers of the MSMBuilder hot path on MI355X (reference: msmbuilder/cluster/__init__.py)."""
from .agglomerative import LandmarkAgglomerative
from .base import MultiSequenceClusterMixin
from .kcenters import KCenters
from .kmeans import KMeans
from .kmedoids import KMedoids
from .minibatchkmeans import MiniBatchKMeans
from .minibatchkmedoids import MiniBatchKMedoids
from .regularspatial import RegularSpatial

__all__ = ['KCenters', 'KMeans', 'KMedoids', 'LandmarkAgglomerative', 'MiniBatchKMeans', 'MiniBatchKMedoids',
           'RegularSpatial', 'MultiSequenceClusterMixin']
