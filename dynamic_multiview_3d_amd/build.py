"""Builds libmv3d_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
import glob
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmv3d_hip.so")

# translation unit -> extra flags
UNITS = {
    "core.hip": [],
    "conv.hip": [],
    "hconv.hip": [],
    "bconv.hip": [],
    "cconv.hip": (["-DCC_TAP_STAMPS"] if os.environ.get("MV3D_CC_TAP_STAMPS") else []),
    "sconv.hip": [],
    "thin.hip": [],
    "wgrad_tile.hip": [],
    "fc.hip": [],
    "elem.hip": ["-ffp-contract=off"],
    "ema.hip": ["-ffp-contract=off"],
    "weight_decay.hip": ["-ffp-contract=off"],
    "grad_norm.hip": ["-ffp-contract=off"],
    "grad_accum.hip": ["-ffp-contract=off"],
    "resampler.hip": ["-ffp-contract=off"],
    "process_image.hip": ["-ffp-contract=off"],
    "color_augment.hip": ["-ffp-contract=off"],
    "geom_augment.hip": ["-ffp-contract=off"],
    "metrics.hip": ["-ffp-contract=off"],
    "ssim_loss.hip": ["-ffp-contract=off"],
    "census_loss.hip": ["-ffp-contract=off"],
    "flow_smooth.hip": ["-ffp-contract=off"],
    "multiscale_loss.hip": ["-ffp-contract=off"],
    "flow_consist.hip": ["-ffp-contract=off"],
    "flow_occlusion.hip": ["-ffp-contract=off"],
    "comm.hip": [],                     # RCCL resolved at run time (dlsym): no link-time dependency
    "tfrecord.hip": ["-msse4.2"],       # host code only: the input thread's record reader (hardware crc32c)
}
COMMON = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Wall", "-Wno-unused-function"]


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: libmv3d_hip.so cannot be built")
    return exe


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    hipcc = _hipcc()
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    # every object depends on every header: coarse, and no header can be forgotten
    headers = sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(HERE, "..", "include", "mv3d_hip.h")]
    objs = []
    for src, extra in UNITS.items():
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + headers):
            cmd = [hipcc] + COMMON + extra + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
    if force or _stale(LIB, objs):
        cmd = [hipcc, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", LIB] + objs + ["-ldl"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
