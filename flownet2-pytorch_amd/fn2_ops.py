"""``torch.library`` operators of the HIP layers, namespace ``fn2``: what ``torch.compile``, ``torch.export`` and ``make_fx`` see in
place of the pybind builtins, which Dynamo cannot look into and a fake tensor cannot be passed to.

This module holds the namespace and the registration helper only; every operator is registered next to its wrapper
(networks/*_package/*.py), so importing one layer's package registers that layer's operators and imports that layer's extension,
no other.  An operator is functional (plain schema types, nothing mutated), and has

  * a CUDA-key implementation: the binding calls of the eager path, in the same order, on the current stream;
  * a fake implementation: shape, dtype, device and contiguity of the results from the arguments' alone -- no data, no ``int()``
    on a size, so symbolic shapes pass through -- which raises what the eager door raises where the shapes or parameters decide it;
  * an autograd formula: a forward operator's calls its backward operator; a backward operator's raises, because the backward of
    every layer is a HIP kernel with no derivative of its own (``create_graph=True``).

Eager calls do not come here: ``XFunction.apply`` goes to the C++ autograd node of its extension as before.  The static
``forward`` / ``backward`` of every Function call the operators while ``torch.compiler.is_compiling()``, which is how Dynamo, which
traces ``autograd.Function.apply`` through those two methods, reaches them.  (The MultiScale criterion has no Function on its GPU path:
there Dynamo is given a stand-in for the builtin, ``torch.compiler.substitute_in_graph``, in losses_fused.py.)

A layer's autograd logic therefore exists three times and the three must move together: the C++ node of its binding (what eager runs),
the static ``forward`` / ``backward`` with their ``is_compiling()`` branches, and the ``_setup`` / ``_grad`` formulas of its operators
(what a direct ``torch.ops.fn2.*`` call and ``opcheck`` run).  tests/test_gpu_compile.py holds the second and third to the first bit for
bit.  ``_fake_pair`` is written out in both correlation.py and correlation1d.py on purpose: a shared module beside them would be imported by
either, and this one must not know any layer.

Two private torch APIs are used, checked against torch 2.10 and liable to change without notice: ``Library._destroy()`` in ``define``
(re-registration) and ``torch._C._dispatch_get_all_op_names()`` in ``names`` (a listing for the tests; nothing at run time depends on it).
"""
import torch

NAMESPACE = "fn2"
_LIBS = {}   # operator name -> the library fragment its registrations hang on; lives as long as the process
_PREVIEW = set()   # qualified names of the operators of preview layers: outside the released record that ``names()`` lists
_INCUBATING = set()   # ... and of incubating layers (build.INCUBATING): outside the preview record as well
_STAGING = set()   # ... and of staging layers (build.STAGING): in none of the three listings above


def refuse(cond, *message):
    """TORCH_CHECK of the fake implementations: RuntimeError, as the bindings raise, unless ``cond``."""
    if not cond:
        raise RuntimeError("".join(str(m) for m in message))


def _not_twice(name):
    def backward(ctx, *grads):
        raise RuntimeError(f"fn2::{name}: the backward of this layer is a HIP kernel and not differentiable a second time "
                           "(create_graph=True)")
    return backward


def define(name, schema, impl, fake, backward=None, setup_context=None, preview=False, incubating=False, staging=False):
    """Register ``fn2::<name><schema>`` and return the operator.  ``backward`` / ``setup_context`` as ``torch.library.register_autograd``
    takes them; without ``backward`` (the backward operators) differentiating the operator raises.  ``preview``: the operator of a
    preview layer (build.PREVIEW): registered like any other, listed by ``names(preview=True)`` only; ``incubating``: the same for
    build.INCUBATING and ``names(incubating=True)``, ``staging`` for build.STAGING and ``names(staging=True)``."""
    qualname = f"{NAMESPACE}::{name}"
    if preview:
        _PREVIEW.add(qualname)
    if incubating:
        _INCUBATING.add(qualname)
    if staging:
        _STAGING.add(qualname)
    if name in _LIBS:   # the wrapper's module is executed a second time (importlib.reload, a deleted sys.modules entry): replace
        # (private API; without it a second execution raises "already defined" -- tests/test_harness_pin.py re-imports the package)
        _LIBS.pop(name)._destroy()
    lib = _LIBS[name] = torch.library.Library(NAMESPACE, "FRAGMENT")
    lib.define(name + schema)
    lib.impl(name, impl, "CUDA")
    torch.library.register_fake(qualname, fake, lib=lib)
    torch.library.register_autograd(qualname, backward or _not_twice(name), setup_context=setup_context, lib=lib)
    return getattr(getattr(torch.ops, NAMESPACE), name)


def names(preview=False, incubating=False, staging=False):
    """The operators of the released layers registered so far, sorted: ``['fn2::correlation', ...]``; with ``preview=True`` those of
    the preview layers instead, with ``incubating=True`` those of the incubating layers, with ``staging=True`` those of the staging
    layers (which none of the other three listings shows).  For the tests (private API, see the module
    docstring)."""
    prefix = NAMESPACE + "::"
    return sorted(n for n in torch._C._dispatch_get_all_op_names()
                  if n.startswith(prefix) and "." not in n[len(prefix):] and (n in _STAGING) == staging
                  and (n in _INCUBATING) == (incubating and not staging) and (n in _PREVIEW) == (preview and not incubating and not staging))
