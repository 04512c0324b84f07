"""``Correlation1d`` / ``Correlation1dFunction`` are exported here, loaded on first use: importing the 2-D layer
(``networks.correlation_package.correlation``) does not load the ``correlation1d_cuda`` extension."""
__all__ = ["Correlation1d", "Correlation1dFunction"]


def __getattr__(name):
    if name in __all__:
        from . import correlation1d
        return getattr(correlation1d, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
