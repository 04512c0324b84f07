"""Builds the HIP libraries and the pybind modules of this package, in-tree, without hipify.  LIBRARIES below is the one
description of what there is: per library its sources, its public header under include/, its version script and the pybind
modules that link it; PREVIEW is a second table of the same descriptor for libraries that are not released yet, INCUBATING a
third for libraries on their way into the preview, STAGING a fourth, open-ended one, where a new library lands.
libflownet2_hip.so (hand-written gfx950 kernels + C ABI) is the drop-in boundary; every other library is a sibling of its own,
self-contained, and none links another.

  python flownet2-pytorch_amd/build.py            # everything
  python flownet2-pytorch_amd/build.py --lib      # kernels + C ABI only (seconds)

hipcc cross-compiles for gfx950 without a GPU.  The pybind modules are plain C++ (g++) against
the ATen headers; they never see a kernel and are not run through torch's hipify pass.
"""
import argparse
import collections
import os
import subprocess
import sys
import sysconfig

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
INCLUDE = os.path.join(HERE, "..", "include")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
             "-munsafe-fp-atomics", "-fvisibility=hidden", "-Wall", "-Wno-unused-function"]
MAX_JOBS = 16

# One entry per library: lib<link>.so = libflownet2_hip[_<name>].so from `srcs` (csrc/), the same flags for all, its objects under
# lib/<name>/; `header` (include/) is its public C ABI, `vmap` (csrc/) its version script, `modules` the pybind modules
# (csrc/binding/) that link it -- each module links exactly one.  "" is the main library; its debug twin (build_lib(debug=True))
# has no entry of its own.
Library = collections.namedtuple("Library", "name link srcs header vmap modules")


def _library(name, srcs, modules, header_dir=""):
    suffix = "_" + name if name else ""
    return Library(name, "flownet2_hip" + suffix, srcs, header_dir + "flownet2_hip%s.h" % suffix, "exports%s.map" % suffix, modules)


LIBRARIES = {lib.name: lib for lib in (
    _library("", ["capi.hip", "channelnorm.hip", "resample2d.hip", "resample2d_lowp.hip", "correlation_direct.hip", "correlation_dense.hip",
                  "correlation_mfma.hip", "correlation_f16x2.hip", "correlation_f16x2_wide.hip", "correlation_f16_fwd.hip",
                  "correlation_f16_bwd.hip", "correlation_f16x2_bwd.hip", "correlation_fused_bwd.hip", "correlation_f16x2_bwd_wide.hip",
                  "correlation_mfma_bwd.hip", "correlation_mfma_f64.hip", "multiscale_loss.hip"],
             ["correlation_cuda", "resample2d_cuda", "channelnorm_cuda", "multiscale_loss_cuda"]),
    _library("ext", ["capi_ext.hip", "correlation_1d.hip"], ["correlation1d_cuda"]),     # layers outside the drop-in boundary
    _library("lookup", ["capi_lookup.hip", "corr_lookup.hip"], ["corr_lookup_cuda"]),
    _library("upsample", ["capi_upsample.hip", "convex_upsample.hip"], ["convex_upsample_cuda"]),
    _library("splat", ["capi_splat.hip", "forward_warp.hip"], ["forward_warp_cuda"]),
    _library("census", ["capi_census.hip", "census.hip"], ["census_cuda"]),
    _library("smooth", ["capi_smooth.hip", "smooth.hip"], ["smoothness_cuda"]),
)}
MODULES = [m for lib in LIBRARIES.values() for m in lib.modules]

# The preview stage: libraries built by the same code with the same flags and conventions, but not yet part of the released
# record above -- their headers live under include/preview/, their ABI version is 0 and may change until they move up into
# LIBRARIES.  Names here and in LIBRARIES are distinct.
PREVIEW = {lib.name: lib for lib in (
    _library("sample", ["capi_sample.hip", "corr_sample.hip"], ["corr_sample_cuda"], header_dir="preview/"),
)}
assert not set(PREVIEW) & set(LIBRARIES)

# The incubating stage: the same descriptor and the same build once more, for libraries that are in neither record above yet (both
# are pinned by the tests that released them).  Headers under include/preview/, ABI version 0.
INCUBATING = {lib.name: lib for lib in (
    _library("pyramid", ["capi_pyramid.hip", "corr_pyramid.hip"], ["corr_pyramid_cuda"], header_dir="preview/"),
)}
TABLES = (LIBRARIES, PREVIEW, INCUBATING)
assert sum(len(t) for t in TABLES) == len(set().union(*TABLES)), "the three tables are disjoint"

# The staging stage: where a new library lands.  The three tables above are closed -- the tests that released their entries pin
# their contents -- and this one is not: its tests name the entries they are about and never its size, so the next library is one
# more line here.  Headers under include/staging/, ABI version 0.
STAGING = {lib.name: lib for lib in (
    _library("ssim", ["capi_ssim.hip", "ssim.hip"], ["ssim_cuda"], header_dir="staging/"),
    _library("sample1d", ["capi_sample1d.hip", "corr_sample1d.hip"], ["corr_sample1d_cuda"], header_dir="staging/"),
)}
ALL_TABLES = TABLES + (STAGING,)
assert sum(len(t) for t in ALL_TABLES) == len(set().union(*ALL_TABLES)), "the tables are disjoint"
assert len({m for t in ALL_TABLES for lib in t.values() for m in lib.modules}) == sum(len(lib.modules) for t in ALL_TABLES for lib in t.values())


def _described(name):
    """The descriptor of a library of any of the tables."""
    for table in ALL_TABLES:
        if name in table:
            return table[name]
    raise KeyError(name)


def _newer(target, deps):
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        raise RuntimeError("build step failed: " + cmd[0])
    return r


def build_lib(force=False, debug=False, ext=False):
    """libflownet2_hip.so (the product: public C ABI only) or, with debug=True, libflownet2_hip_debug.so: the same kernels plus
    the fn2_debug_* entry points and the profiling instantiations they select (csrc/fn2_debug.h; scripts/ and ablation runs);
    with ext=NAME the sibling library libflownet2_hip_NAME.so (NAME of any of the tables, the same flags, its own version
    script); ext=True means "ext"."""
    desc = _described("ext" if ext is True else ext or "")
    twin = debug and not desc.name
    objdir = os.path.join(LIBDIR, "debug" if twin else desc.name) if twin or desc.name else LIBDIR
    lib = os.path.join(LIBDIR, "lib%s.so" % (desc.link + "_debug" if twin else desc.link))
    vmap = os.path.join(CSRC, desc.vmap)
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".h")]
    hdrs += [os.path.join(INCLUDE, h) for h in dict.fromkeys(("flownet2_hip.h", desc.header))]
    objs, jobs = [], []
    for src in desc.srcs:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        if force or not _newer(o, [s] + hdrs):
            jobs.append([HIPCC] + HIP_FLAGS + (["-DFN2_DEBUG_BUILD"] if debug else []) + ["-c", s, "-o", o])
        objs.append(o)
    if jobs:   # the translation units are independent: compile them side by side (each hipcc is single-threaded)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1, MAX_JOBS)) as pool:
            list(pool.map(_run, jobs))
    if force or not _newer(lib, objs + [vmap]):
        _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + vmap, "-o", lib] + objs)
    return lib


def build_modules(force=False):
    import torch
    tdir = os.path.dirname(torch.__file__)
    tinc = [os.path.join(tdir, "include"), os.path.join(tdir, "include", "torch", "csrc", "api", "include")]
    ext = sysconfig.get_config_var("EXT_SUFFIX")
    abi = int(torch._C._GLIBCXX_USE_CXX11_ABI)
    shared = [os.path.join(CSRC, "binding", "binding_common.h"), os.path.join(CSRC, "binding", "binding_status.h"),
              os.path.join(INCLUDE, "flownet2_hip.h")]   # (the sibling headers take their codes and dtype enums from flownet2_hip.h)
    outs, jobs = [], []
    for lib, m in ((lib, m) for table in ALL_TABLES for lib in table.values() for m in lib.modules):
        src = os.path.join(CSRC, "binding", m + ".cpp")
        out = os.path.join(HERE, m + ext)
        if force or not _newer(out, [src] + shared + [os.path.join(INCLUDE, lib.header)]):
            cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
                   "-DTORCH_EXTENSION_NAME=" + m, "-DTORCH_API_INCLUDE_EXTENSION_H",
                   "-D_GLIBCXX_USE_CXX11_ABI=%d" % abi, "-I" + INCLUDE,
                   "-I/opt/rocm/include", "-I" + sysconfig.get_paths()["include"]]
            cmd += ["-I" + i for i in tinc]
            cmd += [src, "-o", out, "-L" + os.path.join(tdir, "lib"), "-lc10", "-lc10_hip", "-ltorch", "-ltorch_cpu",
                    "-ltorch_hip", "-ltorch_python", "-L" + LIBDIR, "-l" + lib.link,
                    "-Wl,-rpath,$ORIGIN/lib", "-Wl,-rpath," + os.path.join(tdir, "lib")]
            jobs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        outs.append(out)
    for cmd, pr in jobs:  # the modules' translation units compile concurrently
        log, _ = pr.communicate()
        if pr.returncode != 0:
            sys.stderr.write(" ".join(cmd) + "\n" + log)
            raise RuntimeError("build step failed: g++")
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="store_true", help="only the kernel library")
    ap.add_argument("--no-debug", action="store_true", help="skip libflownet2_hip_debug.so (profiling entry points)")
    ap.add_argument("--force", action="store_true")
    a = ap.parse_args()
    # the libraries share no object files: compile them side by side
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=8) as pool:
        futs = [pool.submit(build_lib, a.force, ext=name) for table in ALL_TABLES for name in table]
        if not a.no_debug:
            futs.append(pool.submit(build_lib, a.force, True))
        for f in futs:
            print(f.result())
    if not a.lib:
        for o in build_modules(a.force):
            print(o)


if __name__ == "__main__":
    main()
