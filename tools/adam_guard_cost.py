"""Cost of the gradient guard: device-event medians of psvo_adam_step alone against psvo_grad_sumsq + psvo_adam_step_guarded.

    python tools/adam_guard_cost.py [--lib this=psvo_amd/csrc/libpsvo_hip.so --lib parent=/path/to/older/libpsvo_hip.so]
                                    [--n 22426 1000000] [--out profiles/adam_guard_cost.json]

Every library named is opened with ctypes on its own (an older one, without the guard's symbols, gives the plain step only) and
the arms are timed alternately, round after round, in one process: a window is BATCH back-to-back calls between two events,
the figure the median over the rounds of window / BATCH -- the stream never drains inside a window, so this is what one more
call costs a training step whose launches are queued the same way, not the latency of a lone launch.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, ROUNDS, WARMUP = 50, 200, 5
C2_STEP_MS = 0.63          # the smallest training step of BASELINE.md (C2)

_P, _F, _LL, _I = ctypes.c_void_p, ctypes.c_float, ctypes.c_longlong, ctypes.c_int


def open_lib(path):
    import torch  # noqa: F401  (one HIP runtime: torch's, see psvo_amd/_lib.py)
    lib = ctypes.CDLL(path)
    lib.psvo_adam_step.restype = _I
    lib.psvo_adam_step.argtypes = [_P, _P, _P, _P, _LL, _F, _F, _F, _F, _LL, _F, _P]
    if hasattr(lib, "psvo_adam_step_guarded"):
        lib.psvo_grad_norm_blocks.restype = _I
        lib.psvo_grad_norm_blocks.argtypes = [_LL]
        lib.psvo_grad_sumsq.restype = _I
        lib.psvo_grad_sumsq.argtypes = [_P, _LL, _P, _P]
        lib.psvo_adam_step_guarded.restype = _I
        lib.psvo_adam_step_guarded.argtypes = [_P, _P, _P, _P, _LL, _F, _F, _F, _F, _LL, _F, _F, _I, _P, _P, _P]
    return lib


def arms(libs, n):
    import torch
    ptr = lambda t: _P(t.data_ptr())
    gen = torch.Generator().manual_seed(0)
    out = {}
    for tag, lib in libs.items():
        p, g = torch.randn(n, generator=gen).cuda(), torch.randn(n, generator=gen).cuda()
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        stream = _P(torch.cuda.current_stream().cuda_stream)

        def plain(lib=lib, p=p, g=g, m=m, v=v, stream=stream):
            assert lib.psvo_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), n, 3e-3, 0.9, 0.999, 1e-8, 1000, -1.0, stream) == 0
        out[tag + ":adam_step"] = plain
        if not hasattr(lib, "psvo_adam_step_guarded"):
            continue
        partial = torch.zeros(lib.psvo_grad_norm_blocks(n), device="cuda", dtype=torch.float64)
        state = torch.zeros(8, device="cuda", dtype=torch.float64)
        for name, clip in (("guarded_noclip", 1e30), ("guarded_clip", 10.0)):
            def guarded(lib=lib, p=p, g=g, m=m, v=v, stream=stream, partial=partial, state=state, clip=clip):
                assert lib.psvo_grad_sumsq(ptr(g), n, ptr(partial), stream) == 0
                assert lib.psvo_adam_step_guarded(ptr(p), ptr(g), ptr(m), ptr(v), n, 3e-3, 0.9, 0.999, 1e-8, 1000, -1.0, clip, 1,
                                                  ptr(partial), ptr(state), stream) == 0
            out[tag + ":" + name] = guarded
    return out


def measure(fns):
    import torch
    times = {k: [] for k in fns}
    for r in range(WARMUP + ROUNDS):
        for k, fn in fns.items():               # alternate the arms inside every round
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(BATCH):
                fn()
            b.record()
            b.synchronize()
            if r >= WARMUP:
                times[k].append(a.elapsed_time(b) * 1e3 / BATCH)      # microseconds per call
    return {k: {"median_us": statistics.median(t), "p10_us": sorted(t)[len(t) // 10], "p90_us": sorted(t)[len(t) * 9 // 10]}
            for k, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], help="tag=path (default: this=<the in-tree library>)")
    ap.add_argument("--n", type=int, nargs="+", default=[22426, 1000000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("adam_guard_cost.py measures on the GPU: none is visible")
    named = a.lib or ["this=" + os.path.join(ROOT, "psvo_amd", "csrc", "libpsvo_hip.so")]
    libs = {s.split("=", 1)[0]: open_lib(s.split("=", 1)[1]) for s in named}
    res = {"batch": BATCH, "rounds": ROUNDS, "device": torch.cuda.get_device_name(0), "n": {}}
    for n in a.n:
        r = measure(arms(libs, n))
        res["n"][str(n)] = r
        for k, v in r.items():
            base = r[k.split(":")[0] + ":adam_step"]["median_us"]
            print("n=%-8d %-22s median %7.2f us  (p10 %7.2f, p90 %7.2f)  +%6.2f us over adam_step = %.2f %% of a %.2f ms step"
                  % (n, k, v["median_us"], v["p10_us"], v["p90_us"], v["median_us"] - base,
                     100.0 * (v["median_us"] - base) / (C2_STEP_MS * 1e3), C2_STEP_MS), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
