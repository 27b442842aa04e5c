"""Build libpsvo_hip.so (hand-written gfx950 HIP kernels + C ABI) in-tree with hipcc.

hipcc cross-compiles for gfx950 without a GPU; the built .so is git-ignored but travels to the
GPU box with the repo snapshot.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB = os.path.join(CSRC, "libpsvo_hip.so")
# (longest compiles first: with 8 parallel hipcc jobs the build then ends when the work does, not when a late-started
#  psvowr_bwd unit does; the *_l2 units are the same sources compiled with PSVO_L = 2 -- two hidden layers per particle MLP)
SOURCES = ["bsim_wobs.hip", "bsim_wobs_ms.hip", "bsim_cov.hip", "psvowr_bwd_l2.hip", "psvowr_bwd.hip", "bsim_bwd_dx4_l2.hip", "bsim_fwd_l2.hip", "bsim_fwd.hip",
           "bsim_bwd_dx2_l2.hip", "bsim_bwd_dx3_l2.hip", "psvowr_fwd.hip", "psvowr_fwd_l2.hip", "bsim_bwd_dx4.hip",
           "bsim_bwd_dx2.hip", "bsim_bwd_dx3.hip", "filter_bwd_l2.hip", "bsim_bwd2_dx2.hip", "filter_bwd.hip",
           "filter_fwd_l2.hip", "filter_cov.hip", "filter_wobs.hip", "filter_wobs_in.hip", "filter_wobs_inad.hip", "filter_fwd.hip", "bsim_bwd2_dx4.hip", "bsim_bwd2_dx3.hip", "mlp_grad.hip", "lstm_bwd.hip",
           "lstm.hip", "rows_mlp.hip", "bsim_bwd.hip", "api.hip", "dense.hip", "adam.hip", "ffbs.hip", "ffbsi.hip",
           "forecast.hip", "map_path.hip", "mlp_wgrad_rowbias.hip"]
HEADERS = ["common.h", "mlp2_valu.h", os.path.join("..", "..", "include", "psvo_hip.h")]      # every unit includes these
# headers only some units include (a change of bsim_bwd2_impl.h rebuilds 4 units, not 27)
UNIT_HEADERS = {"bsim_bwd_impl.h": ("bsim_bwd_dx", "bsim_bwd2_dx", "bsim_bwd.hip"),
                "bsim_bwd2_impl.h": ("bsim_bwd2_dx", "bsim_bwd.hip"),
                "ffbs_pair.h": ("ffbs.hip", "ffbsi.hip", "map_path.hip"),
                "filter_fwd_impl.h": ("filter_fwd",),
                "filter_bwd_impl.h": ("filter_bwd",),
                "filter_wobs_impl.h": ("filter_wobs.hip", "filter_wobs_in.hip", "filter_wobs_inad.hip"),
                "filter_wobs_args.h": ("filter_wobs.hip", "filter_wobs_in.hip", "filter_wobs_inad.hip"),
                "row_bias.h": ("filter_wobs_in.hip", "filter_wobs_inad.hip", "forecast.hip"),
                "wobs_common.h": ("filter_wobs.hip", "filter_wobs_in.hip", "filter_wobs_inad.hip", "bsim_wobs", "forecast.hip",
                                  "map_path.hip")}
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize"]
# Round 2 built the two-hidden-layer units with `-mllvm -vgpr-regalloc=basic`: their per-lane H x H layer held 2 H values per
# lane and under that pressure the default (greedy) allocator split live ranges around divergent regions, with hipcc 7.2 placing
# the copies of such a split ahead of the EXEC restore (tools/exec_restore_check.py).  Since round 3 the
# H x H layer runs on the matrix pipe (common.h: MlpLds<.., 2>) and needs ~80 registers; all units are built with the default
# allocator again and ALL kernels are held to the ISA check (tests/test_abi.py).  PSVO_L2_BASIC=1 restores the old flags.
L2_FLAGS = ["-mllvm", "-vgpr-regalloc=basic"] if os.environ.get("PSVO_L2_BASIC", "0") == "1" else []


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_lib(force=False, verbose=True):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    jobs = []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(CSRC, s.replace(".hip", ".o"))
        deps = [src] + hdrs
        if s.endswith("_l2.hip"):
            deps.append(os.path.join(CSRC, s.replace("_l2.hip", ".hip")))       # (#include "X.hip")
        if s.endswith("_ms.hip"):
            deps.append(os.path.join(CSRC, s.replace("_ms.hip", ".hip")))       # (likewise, with PSVO_MS = 1)
        if s.startswith("bsim_bwd_dx"):
            deps.append(os.path.join(CSRC, s.replace("_l2", "")))
        deps += [os.path.join(CSRC, h) for h, users in UNIT_HEADERS.items() if s.startswith(users)]
        if force or _stale(obj, deps):
            jobs.append([hipcc] + FLAGS + (L2_FLAGS if s.endswith("_l2.hip") else []) + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print("[psvo_amd.build]", " ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4)) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(CSRC, s.replace(".hip", ".o")) for s in SOURCES]
    if force or jobs or _stale(LIB, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    return LIB


if __name__ == "__main__":
    print(build_lib(force="--force" in sys.argv))
