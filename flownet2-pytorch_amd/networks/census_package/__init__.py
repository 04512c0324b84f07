"""``CensusFunction`` / ``census_distance`` / ``TernaryCensus`` / ``CensusLoss`` (``census.py``), loaded on first use: importing the
package alone does not load the ``census_cuda`` extension."""
_HOME = {"CensusFunction": "census", "census_distance": "census", "TernaryCensus": "census", "CensusLoss": "census"}
__all__ = list(_HOME)


def __getattr__(name):
    if name in _HOME:
        import importlib
        return getattr(importlib.import_module("." + _HOME[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
