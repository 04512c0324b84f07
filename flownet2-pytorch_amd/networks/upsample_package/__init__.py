"""``ConvexUpsample`` / ``ConvexUpsampleFunction`` / ``upsample_flow`` (``convex_upsample.py``), loaded on first use: importing
the package alone does not load the ``convex_upsample_cuda`` extension."""
_HOME = {"ConvexUpsample": "convex_upsample", "ConvexUpsampleFunction": "convex_upsample", "upsample_flow": "convex_upsample"}
__all__ = list(_HOME)


def __getattr__(name):
    if name in _HOME:
        import importlib
        return getattr(importlib.import_module("." + _HOME[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
