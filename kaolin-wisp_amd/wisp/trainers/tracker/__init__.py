from .offline_renderer import OfflineRenderer

__all__ = ["OfflineRenderer"]
