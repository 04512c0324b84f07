"""``ForwardWarp`` / ``ForwardWarpFunction`` / ``softsplat`` / ``range_map`` (``forward_warp.py``), loaded on first use: importing
the package alone does not load the ``forward_warp_cuda`` extension."""
_HOME = {"ForwardWarp": "forward_warp", "ForwardWarpFunction": "forward_warp", "softsplat": "forward_warp", "range_map": "forward_warp"}
__all__ = list(_HOME)


def __getattr__(name):
    if name in _HOME:
        import importlib
        return getattr(importlib.import_module("." + _HOME[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
