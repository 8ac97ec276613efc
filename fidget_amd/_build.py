"""Where libfidget_hip.so lives, what it is built from, and the recipe that builds it.  Imports nothing of the package.

`_SOURCES` - the files whose modification times decide whether build() finds the library stale - is not kept by hand: it is what the
quoted `#include "..."` lines lead to from csrc/capi.hip, and the few build inputs that no #include names (`_UNINCLUDED`)."""
import os
import re
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("FHIP_LIB") or os.path.join(_CSRC, "libfidget_hip.so")     # (FHIP_LIB: a variant build, tools/build_lib_variant.py - A/B runs)

# the build inputs that no #include names: the generators, and the two files that are compiled on their own
_UNINCLUDED = ("gen_asm.py", "gen_interp.py", "gen_tiles.py", "gen_tilesv.py", "gen_normals.py", "gen_prune.py", "gen_ubench.py", "gen_trans.py",
               "offsets.cpp", "trans_funcs.hip")
_INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def _sources():
    """capi.hip and every file its quoted includes reach, as paths relative to csrc ("contour/contour.hpp",
    "../../include/fidget_hip.h"), then `_UNINCLUDED`.  A name that does not exist is listed and not read: build() fails on it."""
    seen, todo = [], ["capi.hip"]
    while todo:
        name = todo.pop()
        if name in seen:
            continue
        seen.append(name)
        path = os.path.join(_CSRC, name)
        if os.path.exists(path):
            with open(path) as f:
                todo += [os.path.relpath(os.path.join(os.path.dirname(path), inc), _CSRC) for inc in _INCLUDE.findall(f.read())]
    return seen + [s for s in _UNINCLUDED if s not in seen]


_SOURCES = _sources()


def build(force=False, verbose=False):
    """Compile libfidget_hip.so for gfx950 (cross-compiles without a GPU): the assembly
    interpreters (gen_interp.py -> .s -> code object, embedded in the library) and the HIP
    kernels + C ABI (capi.hip)."""
    srcs = [os.path.join(_CSRC, s) for s in _sources()]
    if os.environ.get("FHIP_LIB"):
        return LIB_PATH         # (a variant built elsewhere: never rebuilt from here)
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(s) <= os.path.getmtime(LIB_PATH) for s in srcs):
        return LIB_PATH
    gen = os.path.join(_CSRC, "_gen")
    os.makedirs(gen, exist_ok=True)
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
    co = os.path.join(gen, "interp_gfx950.co")

    def run(cmd, **kw):
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd, **kw)

    run(["g++", "-std=c++17", "-I", _CSRC, os.path.join(_CSRC, "offsets.cpp"), "-o", os.path.join(gen, "offsets")])
    with open(os.path.join(gen, "offsets.json"), "w") as f:
        subprocess.check_call([os.path.join(gen, "offsets")], stdout=f)
    # the transcendental routines the assembly interpreters call: trans_funcs.hip through LLVM IR, where the functions are limited to
    # 8 scalar registers + vcc / the return address ("amdgpu-num-sgpr": clang takes that attribute on kernels only; the handlers
    # that call them have ten free) -> llc -> assembly, embedded by gen_trans.py
    ll = os.path.join(gen, "trans_funcs.ll")
    run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "-emit-llvm", "--cuda-device-only", "-I", _CSRC,
         "-o", ll, os.path.join(_CSRC, "trans_funcs.hip")])
    ir = open(ll).read()
    groups = set()
    for fn in ("fh_t_sin", "fh_t_atan2", "fh_t_mod", "fh_t_sin4", "fh_t_ln4"):
        m = re.search(rf"^define [^\n]*@{fn}\([^\n]*\) (#\d+)", ir, re.M)
        assert m, f"trans_funcs.ll: {fn} not found"
        groups.add(m.group(1))
    for g in groups:
        ir, n = re.subn(rf"^attributes {g} = {{ ", f'attributes {g} = {{ "amdgpu-num-sgpr"="18" ', ir, flags=re.M)
        assert n == 1
    with open(ll, "w") as f:
        f.write(ir)
    run([os.path.join(llvm, "llc"), "-mtriple=amdgcn-amd-amdhsa", "-mcpu=gfx950", "-O3", "-o", os.path.join(gen, "trans_funcs.s"), ll])
    run([sys.executable, os.path.join(_CSRC, "gen_interp.py"), os.path.join(gen, "offsets.json"),
         os.path.join(gen, "interp_gfx950.s"), os.path.join(gen, "trans_funcs.s")])
    run([os.path.join(llvm, "clang"), "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950", "-c",
         os.path.join(gen, "interp_gfx950.s"), "-o", os.path.join(gen, "interp_gfx950.o")])
    run([os.path.join(llvm, "ld.lld"), "-shared", os.path.join(gen, "interp_gfx950.o"), "-o", co])
    run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
         f'-DFH_INTERP_CO="{co}"', "-o", LIB_PATH, os.path.join(_CSRC, "capi.hip")])
    return LIB_PATH
