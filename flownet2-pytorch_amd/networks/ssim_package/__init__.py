"""``SSIMFunction`` / ``ssim_distance`` / ``SSIM`` / ``SSIMLoss`` (``ssim.py``), loaded on first use: importing the package alone
does not load the ``ssim_cuda`` extension."""
_HOME = {"SSIMFunction": "ssim", "ssim_distance": "ssim", "SSIM": "ssim", "SSIMLoss": "ssim"}
__all__ = list(_HOME)


def __getattr__(name):
    if name in _HOME:
        import importlib
        return getattr(importlib.import_module("." + _HOME[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
