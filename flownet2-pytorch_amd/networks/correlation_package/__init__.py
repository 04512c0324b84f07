"""``Correlation1d`` / ``Correlation1dFunction``, ``CorrLookup`` / ``CorrLookupFunction`` / ``AlternateCorrBlock``, (preview)
``CorrBlock`` / ``CorrSample`` / ``corr_sample``, (incubating) ``CorrPyramid`` / ``CorrPyramidFunction`` / ``corr_pyramid`` and
(staging) ``CorrBlock1D`` / ``CorrSample1d`` / ``CorrSample1dFunction`` / ``corr_sample1d`` are exported here, loaded on first use:
importing the 2-D layer (``networks.correlation_package.correlation``) loads none of the ``correlation1d_cuda``,
``corr_lookup_cuda``, ``corr_sample_cuda``, ``corr_pyramid_cuda`` and ``corr_sample1d_cuda`` extensions, and each of the others
loads only its own."""
_HOME = {"Correlation1d": "correlation1d", "Correlation1dFunction": "correlation1d",
         "CorrLookup": "corr_lookup", "CorrLookupFunction": "corr_lookup", "AlternateCorrBlock": "corr_lookup",
         "CorrBlock": "corr_block", "CorrSample": "corr_block", "corr_sample": "corr_block",
         "CorrPyramid": "corr_pyramid", "CorrPyramidFunction": "corr_pyramid", "corr_pyramid": "corr_pyramid",
         "CorrBlock1D": "corr_block1d", "CorrSample1d": "corr_block1d", "CorrSample1dFunction": "corr_block1d",
         "corr_sample1d": "corr_block1d"}
__all__ = list(_HOME)


def __getattr__(name):
    if name in _HOME:
        import importlib
        return getattr(importlib.import_module("." + _HOME[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
