"""CPU-side checks of every library of build.LIBRARIES, one case per entry: its ABI version, that it exports what its header
declares, what fn2_capi lists and the names written out here, that it links none of the other libraries, and that its prefix is
its own; and of every pybind module, that it links exactly the one library the table gives it."""
import os
import re
import subprocess
import sysconfig

import pytest

from conftest import PKG, ROOT

import build
import fn2_capi

# name of build.LIBRARIES -> (symbol prefix, ABI version, the exported names; a count for the main library, whose names
# tests/test_capi_host.py pins one by one)
EXPECTED = {
    "": ("fn2_", 3, 31),
    "ext": ("fn2x_", 1, ["fn2x_abi_version", "fn2x_correlation1d_backward", "fn2x_correlation1d_forward", "fn2x_correlation1d_output_shape"]),
    "lookup": ("fn2l_", 1, ["fn2l_abi_version", "fn2l_corr_lookup_backward", "fn2l_corr_lookup_forward"]),
    "upsample": ("fn2u_", 1, ["fn2u_abi_version", "fn2u_convex_upsample_backward", "fn2u_convex_upsample_backward_workspace_bytes",
                              "fn2u_convex_upsample_forward"]),
    "splat": ("fn2s_", 1, ["fn2s_abi_version", "fn2s_forward_warp_backward", "fn2s_forward_warp_forward", "fn2s_forward_warp_forward_det",
                           "fn2s_forward_warp_forward_det_workspace_bytes"]),
    "census": ("fn2c_", 1, ["fn2c_abi_version", "fn2c_census_backward", "fn2c_census_forward"]),
    "smooth": ("fn2m_", 1, ["fn2m_abi_version", "fn2m_smoothness_backward", "fn2m_smoothness_forward"]),
}


def _capi(name):
    """(loader, path, export list) of a library in fn2_capi: lib / LIB_PATH / EXPORTS, ext_lib / EXT_LIB_PATH / EXT_EXPORTS, ..."""
    stem = name.upper() + "_" if name else ""
    return getattr(fn2_capi, stem.lower() + "lib"), getattr(fn2_capi, stem + "LIB_PATH"), getattr(fn2_capi, stem + "EXPORTS")


def _declared(header, prefix):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, code)))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted({ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3})


def _needed(path):
    """The project libraries among the NEEDED entries of a shared object."""
    dyn = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
    return sorted(re.findall(r"\(NEEDED\).*\[(libflownet2_hip[^\]]*)\]", dyn))


def test_the_expectations_cover_the_table():
    assert list(EXPECTED) == list(build.LIBRARIES) and len(build.LIBRARIES) == 7


@pytest.mark.parametrize("name", list(build.LIBRARIES), ids=lambda n: n or "main")
def test_library_exports_what_its_header_declares(name):
    desc = build.LIBRARIES[name]
    prefix, abi, names = EXPECTED[name]
    loader, path, listed = _capi(name)
    assert os.path.samefile(path, os.path.join(PKG, "lib", "lib%s.so" % desc.link))
    header = open(os.path.join(ROOT, "include", desc.header)).read()
    macro = int(re.search(r"^#define %sABI_VERSION (\d+)$" % prefix.upper(), header, flags=re.M).group(1))
    assert getattr(loader(), prefix + "abi_version")() == abi == macro
    exported = _exported(path)
    assert exported == _declared(desc.header, prefix), set(exported) ^ set(_declared(desc.header, prefix))
    assert sorted(listed) == exported
    assert exported == names if isinstance(names, list) else len(exported) == names
    # self-contained: none of the other libraries is a dependency of it
    dyn = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
    assert "libflownet2_hip" not in dyn.replace("lib%s.so" % desc.link, "") and _needed(path) == []
    # and its prefix is its own: no other library, the debug twin of the main one included, exports a name under it
    others = [n for other in build.LIBRARIES if other != name for n in _capi(other)[2]] + (fn2_capi.DEBUG_EXPORTS if name else [])
    assert not any(n.startswith(prefix) for n in others)


@pytest.mark.parametrize("module", build.MODULES)
def test_module_links_the_one_library_the_table_gives_it(module):
    desc, = [lib for lib in build.LIBRARIES.values() if module in lib.modules]
    assert _needed(os.path.join(PKG, module + sysconfig.get_config_var("EXT_SUFFIX"))) == ["lib%s.so" % desc.link]
