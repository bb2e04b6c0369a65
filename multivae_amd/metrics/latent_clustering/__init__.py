from .clustering_class import Clustering
from .clustering_config import ClusteringConfig
from .kmeans import DeviceKMeans

__all__ = ["Clustering", "ClusteringConfig", "DeviceKMeans"]
