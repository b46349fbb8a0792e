"""Build libdtsim.so (HIP, gfx950) in-tree; hipcc cross-compiles without a GPU, lib/ is git-ignored.

    python gym-duckietown_amd/build.py [--force]                      -> lib/libdtsim.so
    python gym-duckietown_amd/build.py --variant NAME [-DFOO=1 ...]   -> lib/libdtsim_NAME.so (objects in lib/NAME/: the default build's stay)
    python gym-duckietown_amd/build.py --asm SRC.hip OUT.s [-D...]    -> the device assembly of one unit (any tree's copy of it)

UNITS is the one statement of the library's units and their flags: tools/isa_*.py, .sh and tools/build_variant.sh take them from here.
physics.hip and remap.hip (the camera_rand table builder, pinned to numpy) are compiled with contraction off (separately rounded ops, in
the reference's operation order); render.hip, render_setup.hip, render_exact.hip and render_v3.hip -- the units of a render pass -- with
contraction allowed (speed, f32), and render_views.hip as they, whose classify() and test_tri it shares (csrc/render_scene.h).
-Werror=unused-function: a helper nobody calls does not build.
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libdtsim.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"

UNITS = {"physics.hip": ["-ffp-contract=off"], "render.hip": ["-ffp-contract=fast"], "render_setup.hip": ["-ffp-contract=fast"],
         "render_exact.hip": ["-ffp-contract=fast"], "render_v3.hip": ["-ffp-contract=fast"],
         "render_views.hip": ["-ffp-contract=fast"], "observe.hip": [], "dtsim_api.hip": [], "remap.hip": ["-ffp-contract=off"]}
COMMON = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-Wall", "-Werror=unused-function", "-Wno-bitwise-instead-of-logical",
          "-I" + os.path.join(HERE, "..", "include")]


def compile_cmd(src: str, out: str, extra=(), asm: bool = False) -> list:
    """hipcc's command line for one unit (flags by its file name; src may be another tree's copy): an object, or its device assembly."""
    return [HIPCC] + COMMON + UNITS[os.path.basename(src)] + list(extra) + (["-S", "--cuda-device-only"] if asm else ["-c"]) + [src, "-o", out]


def _newer(src_list, target):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in src_list)


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def build(force: bool = False, verbose: bool = True, variant: str = "", defines=()) -> str:
    objdir = os.path.join(LIBDIR, variant) if variant else LIBDIR
    lib = os.path.join(LIBDIR, f"libdtsim_{variant}.so") if variant else LIB
    os.makedirs(objdir, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(HERE, "..", "include", "dtsim.h"))
    objs = [os.path.join(objdir, name.replace(".hip", ".o")) for name in UNITS]
    for name, obj in zip(UNITS, objs):
        src = os.path.join(CSRC, name)
        if force or variant or _newer([src] + headers, obj):      # (a variant's defines are in no time stamp: always compiled)
            _run(compile_cmd(src, obj, defines), verbose)
    if force or _newer(objs, lib):
        _run([HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", lib] + objs, verbose)
    return lib


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--asm"]:
        _run(compile_cmd(args[1], args[2], args[3:], asm=True), False)
    elif args[:1] == ["--variant"]:
        print(build(verbose=False, variant=args[1], defines=" ".join(args[2:]).split()))
    else:
        print(build(force="--force" in args))
