"""``Correlation1d`` / ``Correlation1dFunction`` and ``CorrLookup`` / ``CorrLookupFunction`` / ``AlternateCorrBlock`` are exported
here, loaded on first use: importing the 2-D layer (``networks.correlation_package.correlation``) loads neither the
``correlation1d_cuda`` nor the ``corr_lookup_cuda`` extension."""
_HOME = {"Correlation1d": "correlation1d", "Correlation1dFunction": "correlation1d",
         "CorrLookup": "corr_lookup", "CorrLookupFunction": "corr_lookup", "AlternateCorrBlock": "corr_lookup"}
__all__ = list(_HOME)


def __getattr__(name):
    if name in _HOME:
        import importlib
        return getattr(importlib.import_module("." + _HOME[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
