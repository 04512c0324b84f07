"""The text a caller sees when the C ABI of a sibling library rejects a call, pinned for every library and code.  The pybind
modules reach it with GPU tensors only; csrc/binding/binding_status.h holds it without torch, so a stand-alone program prints it
here.  The expected strings are written out in full: three libraries have no wording for FN2_EDTYPE and say "unknown error"."""
import os
import subprocess

from conftest import PKG, ROOT

CODES = (-1, -2, -3, -4, 7, -9)   # FN2_EINVAL, FN2_EDTYPE, FN2_EALIGN, FN2_EUNSUPPORTED, a hipError_t, an unknown code

EXPECTED = {
    "STATUS_EXT": [
        "op: HIP call failed: flownet2_hip_ext: invalid shape or parameter (code -1)",
        "op: HIP call failed: flownet2_hip_ext: dtype not supported by this op (code -2)",
        "op: HIP call failed: flownet2_hip_ext: pointer not aligned to its element size (code -3)",
        "op: HIP call failed: flownet2_hip_ext: unsupported parameter combination (the backward needs stride1 == 1) (code -4)",
        "op: HIP call failed: flownet2_hip_ext: hipError_t from the launch (code 7)",
        "op: HIP call failed: flownet2_hip_ext: unknown error (code -9)"],
    "STATUS_LOOKUP": [
        "op: HIP call failed: flownet2_hip_lookup: invalid shape or parameter (radius must be 0 .. 8) (code -1)",
        "op: HIP call failed: flownet2_hip_lookup: dtype not supported by this op (float32 only) (code -2)",
        "op: HIP call failed: flownet2_hip_lookup: pointer not aligned to its element size (code -3)",
        "op: HIP call failed: flownet2_hip_lookup: unsupported size or selector (code -4)",
        "op: HIP call failed: flownet2_hip_lookup: hipError_t from the launch (code 7)",
        "op: HIP call failed: flownet2_hip_lookup: unknown error (code -9)"],
    "STATUS_UPSAMPLE": [
        "op: HIP call failed: flownet2_hip_upsample: invalid shape or parameter (factor must be 2, 4 or 8) (code -1)",
        "op: HIP call failed: flownet2_hip_upsample: dtype not supported by this op (mask: float32, float16 or bfloat16) (code -2)",
        "op: HIP call failed: flownet2_hip_upsample: pointer not aligned to its element size (code -3)",
        "op: HIP call failed: flownet2_hip_upsample: unsupported size (at most 4 flow channels) (code -4)",
        "op: HIP call failed: flownet2_hip_upsample: hipError_t from the launch (code 7)",
        "op: HIP call failed: flownet2_hip_upsample: unknown error (code -9)"],
    "STATUS_SPLAT": [
        "op: HIP call failed: flownet2_hip_splat: invalid shape, selector or workspace (code -1)",
        "op: HIP call failed: flownet2_hip_splat: unknown error (code -2)",
        "op: HIP call failed: flownet2_hip_splat: pointer not aligned to its element size (code -3)",
        "op: HIP call failed: flownet2_hip_splat: unsupported size (a plane of 2^31 elements or more, or too many planes) (code -4)",
        "op: HIP call failed: flownet2_hip_splat: hipError_t from the launch (code 7)",
        "op: HIP call failed: flownet2_hip_splat: unknown error (code -9)"],
    "STATUS_CENSUS": [
        "op: HIP call failed: flownet2_hip_census: invalid shape or parameter (code -1)",
        "op: HIP call failed: flownet2_hip_census: unknown error (code -2)",
        "op: HIP call failed: flownet2_hip_census: pointer not aligned to its element size (code -3)",
        "op: HIP call failed: flownet2_hip_census: unsupported size (a plane of 2^31 elements or more, or too many planes) (code -4)",
        "op: HIP call failed: flownet2_hip_census: hipError_t from the launch (code 7)",
        "op: HIP call failed: flownet2_hip_census: unknown error (code -9)"],
    "STATUS_SMOOTH": [
        "op: HIP call failed: flownet2_hip_smooth: invalid shape or parameter (code -1)",
        "op: HIP call failed: flownet2_hip_smooth: unknown error (code -2)",
        "op: HIP call failed: flownet2_hip_smooth: pointer not aligned to its element size (code -3)",
        "op: HIP call failed: flownet2_hip_smooth: unsupported size (a plane of 2^31 elements or more, or too many planes) (code -4)",
        "op: HIP call failed: flownet2_hip_smooth: hipError_t from the launch (code 7)",
        "op: HIP call failed: flownet2_hip_smooth: unknown error (code -9)"],
}

PROGRAM = """
#include <cstdio>
#include "binding_status.h"
int main()
{
    const fn2b::StatusText *libs[] = {%s};
    const int codes[] = {%s};
    for (const fn2b::StatusText *lib : libs)
        for (int rc : codes) std::puts(fn2b::status_message(*lib, "op", rc).c_str());
    return 0;
}
"""


def test_status_text_of_every_sibling_library_and_code(tmp_path):
    src, exe = tmp_path / "status.cpp", tmp_path / "status"
    src.write_text(PROGRAM % (", ".join("&fn2b::" + name for name in EXPECTED), ", ".join(map(str, CODES))))
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc", "binding"), "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    want = [line for name in EXPECTED for line in EXPECTED[name]]
    assert len(lines) == len(want) == 6 * len(CODES)
    for got, line in zip(lines, want):
        assert got == line


def test_every_sibling_module_uses_its_own_table():
    """One status table per sibling library, named in the module that links it and in no other; and no sibling module refers to
    fn2_strerror, which lives in the main library."""
    import sysconfig

    import build
    for name, desc in build.LIBRARIES.items():
        for module in desc.modules:
            text = open(os.path.join(PKG, "csrc", "binding", module + ".cpp")).read()
            assert [t for t in EXPECTED if t in text] == (["STATUS_" + name.upper()] if name else []), module
            undefined = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(PKG, module + sysconfig.get_config_var("EXT_SUFFIX"))],
                                       capture_output=True, text=True, check=True).stdout
            assert ("fn2_strerror" in undefined) == (name == ""), module
