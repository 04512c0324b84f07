"""The door ``CorrBlock(fused_build=True)`` takes to corr_pyramid.py.  That module is callable (it shares its name with its main
function, see there), and ``torch.compile`` cannot hold a module of a class of its own: an import of it inside the traced
constructor breaks the graph.  Importing this plain module there runs the real import outside the trace and hands over a plain
function."""
from .corr_pyramid import corr_pyramid as build_pyramid  # noqa: F401
