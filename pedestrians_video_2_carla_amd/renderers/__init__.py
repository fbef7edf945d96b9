from .points_renderer import PointsRenderer, Renderer

__all__ = ['PointsRenderer', 'Renderer']
