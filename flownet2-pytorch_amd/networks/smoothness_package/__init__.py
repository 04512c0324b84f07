"""``SmoothnessFunction`` / ``smoothness_map`` / ``EdgeAwareSmoothness`` / ``SmoothnessLoss`` (``smoothness.py``), loaded on first use:
importing the package alone does not load the ``smoothness_cuda`` extension."""
_HOME = {"SmoothnessFunction": "smoothness", "smoothness_map": "smoothness", "EdgeAwareSmoothness": "smoothness",
         "SmoothnessLoss": "smoothness"}
__all__ = list(_HOME)


def __getattr__(name):
    if name in _HOME:
        import importlib
        return getattr(importlib.import_module("." + _HOME[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
