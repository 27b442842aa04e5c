"""Time of the marginal particle smoother (psvo_ffbs_smooth) beside the forward filter that feeds it, device events.

    python tools/ffbs_timing.py [--out profiles/ffbs_timing.json] [--shape B T N Dx] ...

Per shape: a forward filter (bootstrap wiring with two proposals, H = 32, Dy = 1, random small weights) fills X, Fm, logW; then
the filter launch and the smoother launch (constant scale, uniforms, every output) are timed alternately, round after round:
a window is BATCH back-to-back launches between two events, the figure the median over the rounds of window / BATCH.  With
--cov the smoother also runs with per-particle scales (a synthetic Fs: the plain filter has none).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(16, 200, 64, 2), (32, 200, 128, 2), (64, 1000, 512, 4)]       # AESMC C2; C*'s batch and particles; the largest
WARMUP, ROUNDS = 3, 15


def arms(B, T, N, Dx, H=32, Dy=1):
    import torch
    from psvo_amd import ops
    g = torch.Generator().manual_seed(0)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    mlp = lambda din, dout: (rn(din, H, scale=0.3), rn(H, scale=0.1), rn(H, dout, scale=0.3), rn(dout, scale=0.1))
    desc = ops.make_desc(B, T, N, 1, Dx, Dy, H)
    q1, gm = mlp(Dx, Dx), mlp(Dx, Dy)
    sig = lambda d: (0.5 + torch.rand(d, generator=g)).cuda()
    sq1, sq2, sg, s0 = sig(Dx), sig(Dx), sig(Dy), sig(Dx)
    mu2, m0, obs = rn(T, B, Dx), rn(B, Dx), rn(T, B, Dy)
    eps, u = rn(T, B, Dx, N), torch.rand(T, B, N, generator=g).cuda()

    def filt():
        return ops.filter_forward(desc, q1, None, gm, sq1, sq2, None, sg, mu2, m0, s0, m0, s0, obs, eps, u=u)
    f = filt()
    us = torch.rand(T, B, N, generator=g).cuda()
    fcov = dict(f, Fs=(sq1.view(1, 1, Dx, 1) * (0.5 + torch.rand(T, B, Dx, N, generator=g).cuda())).contiguous())
    out = {"filter_forward": filt,
           "ffbs_smooth": lambda: ops.ffbs_smooth(desc, f, sig_f=sq1, u=us),
           "ffbs_smooth_nodraw": lambda: ops.ffbs_smooth(desc, f, sig_f=sq1, want_draws=False),
           "ffbs_smooth_cov": lambda: ops.ffbs_smooth(desc, fcov, u=us)}
    ess = ops.ffbs_smooth(desc, f, sig_f=sq1, u=us)["ess"]
    torch.cuda.synchronize()
    return out, float(ess.mean()), float(ess.min())


def measure(fns, batch):
    import torch
    times = {k: [] for k in fns}
    for r in range(WARMUP + ROUNDS):
        for k, fn in fns.items():               # alternate the arms inside every round
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(batch):
                fn()
            b.record()
            b.synchronize()
            if r >= WARMUP:
                times[k].append(a.elapsed_time(b) / batch)      # milliseconds per launch
    return {k: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for k, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, action="append", metavar=("B", "T", "N", "Dx"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ffbs_timing.py measures on the GPU: none is visible")
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "shapes": {}}
    for B, T, N, Dx in (a.shape or SHAPES):
        fns, ess_mean, ess_min = arms(B, T, N, Dx)
        batch = 20 if T * N <= 200 * 128 else 3
        r = measure(fns, batch)
        res["shapes"]["B%d T%d N%d Dx%d" % (B, T, N, Dx)] = dict(r, batch=batch, ess_mean=ess_mean, ess_min=ess_min)
        for k, v in r.items():
            print("B%-3d T%-5d N%-4d Dx%d  %-20s median %8.4f ms  (min %8.4f, max %8.4f)  %7.1f ns per step"
                  % (B, T, N, Dx, k, v["median_ms"], v["min_ms"], v["max_ms"], v["median_ms"] * 1e6 / T), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
