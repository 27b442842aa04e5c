"""Time of the wide-observation backward simulation (psvo_bsim_forward_wobs, psvo_bsim_backward_wobs) beside the plain kernels
(psvo_bsim_forward, psvo_bsim_backward + psvo_bsim_backward_fold) at the same shape with Dy = 2, device events.

    python tools/wobs_bsim_timing.py [--out profiles/wobs_bsim_timing.json] [--shape B T N M Dx Dy H]

Both arms run on the same random filter outputs (Fm, logW, lse = logsumexp logW) and small random weights.  Every native launch
is bracketed by two events through ops.set_timing_hook, as bench.py does; the arms alternate round after round, and the figure
of an entry point is the median over the rounds (tools/ffbsi_timing.py: warm-up rounds first), with minimum and maximum.
Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, ROUNDS = 3, 15


def arm(B, T, N, M, Dx, Dy, H, wide):
    import torch
    from psvo_amd import ops
    g = torch.Generator().manual_seed(0)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    mlp = lambda din, dout: (rn(din, H, scale=0.3), rn(H, scale=0.1), rn(H, dout, scale=0.3), rn(dout, scale=0.1))
    sig = lambda d: (0.5 + torch.rand(d, generator=g)).cuda()
    desc = ops.make_desc(B, T, N, M, Dx, Dy, H)
    logW = rn(T, B, N)
    filt = {"Fm": rn(T, B, Dx, N), "logW": logW, "lse": torch.logsumexp(logW, -1).contiguous()}
    filt["X"] = filt["Fm"]
    args = (desc, filt, mlp(Dx, Dx), mlp(Dx, Dy), mlp(Dx, Dx), sig(Dx), sig(Dy), sig(Dx), sig(Dx), rn(T, B, Dx), rn(B, Dx),
            sig(Dx), rn(B, Dx), sig(Dx), rn(T, B, Dy), rn(T, B, Dx, N, M))
    u_b, dscore = torch.rand(T, B, N, generator=g).cuda(), rn(B, N)
    fwd = ops.bsim_forward_wobs if wide else ops.bsim_forward
    bwd = ops.bsim_backward_wobs if wide else ops.bsim_backward

    def run():
        bs = fwd(*args, u_b=u_b, save=True)
        return bwd(*args, bs, dscore)
    return run


def measure(arms):
    import torch
    from psvo_amd import ops
    marks, times = [], {}

    def hook(name, phase, stream):
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        marks.append((name, phase, e))
    for r in range(WARMUP + ROUNDS):
        for run in arms:                # alternate the arms inside every round
            del marks[:]
            ops.set_timing_hook(hook)
            try:
                run()
            finally:
                ops.set_timing_hook(None)
            torch.cuda.synchronize()
            if r >= WARMUP:
                per = {}
                for (n0, p0, e0), (n1, p1, e1) in zip(marks[0::2], marks[1::2]):
                    assert n0 == n1 and (p0, p1) == (0, 1)
                    per[n0] = per.get(n0, 0.0) + e0.elapsed_time(e1)
                for k, v in per.items():
                    times.setdefault(k, []).append(v)
    return {k: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for k, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=7, default=[8, 100, 64, 16, 3, 10, 32], metavar=("B", "T", "N", "M", "Dx", "Dy", "H"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("wobs_bsim_timing.py measures on the GPU: none is visible")
    B, T, N, M, Dx, Dy, H = a.shape
    r = measure([arm(B, T, N, M, Dx, Dy, H, True), arm(B, T, N, M, Dx, 2, H, False)])
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "shape": dict(B=B, T=T, N=N, M=M, Dx=Dx, Dy=Dy, H=H),
           "plain_Dy": 2, "launches": r}
    for k, v in sorted(r.items()):
        print("%-28s median %8.4f ms  (min %8.4f, max %8.4f)" % (k, v["median_ms"], v["min_ms"], v["max_ms"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
