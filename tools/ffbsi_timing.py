"""Time of the backward sampler (psvo_ffbs_sample) beside the marginal smoother (psvo_ffbs_smooth) and the forward filter that
feeds both, device events.

    python tools/ffbsi_timing.py [--out profiles/ffbsi_timing.json] [--shape B T N Dx] ...

Per shape the particle system is the one of tools/ffbs_timing.py (a forward filter in the bootstrap wiring with two proposals,
H = 32, Dy = 1, random small weights).  The filter launch, the smoother launch (constant scale, uniforms, every output) and the
sampler launches (constant scale with uniforms; teacher-forced indices, which skip the draw phase; per-particle scales from a
synthetic Fs) are timed alternately, round after round: a window is BATCH back-to-back launches between two events, the figure
the median over the rounds of window / BATCH, reported with its minimum and maximum.  Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ffbs_timing as FT          # noqa: E402  (the shapes, the particle system and the measuring loop)


def arms(B, T, N, Dx):
    import torch
    from psvo_amd import ops
    base, _, _ = FT.arms(B, T, N, Dx)
    f = base["filter_forward"]()
    desc = ops.make_desc(B, T, N, 1, Dx, 1, 32)
    g = torch.Generator().manual_seed(1)
    sig = (0.5 + torch.rand(Dx, generator=g)).cuda()
    up = torch.rand(T, B, N, generator=g).cuda()
    fcov = dict(f, Fs=(sig.view(1, 1, Dx, 1) * (0.5 + torch.rand(T, B, Dx, N, generator=g).cuda())).contiguous())
    first = ops.ffbs_sample(desc, f, sig_f=sig, u=up)
    out = {"filter_forward": base["filter_forward"],
           "ffbs_smooth": lambda: ops.ffbs_smooth(desc, f, sig_f=sig, u=up),
           "ffbs_sample": lambda: ops.ffbs_sample(desc, f, sig_f=sig, u=up),
           "ffbs_sample_forced": lambda: ops.ffbs_sample(desc, f, sig_f=sig, idx_in=first["idx"]),
           "ffbs_sample_cov": lambda: ops.ffbs_sample(desc, fcov, u=up)}
    distinct = first["distinct"].float()
    torch.cuda.synchronize()
    return out, float(distinct.mean()), float(distinct.min())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, action="append", metavar=("B", "T", "N", "Dx"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ffbsi_timing.py measures on the GPU: none is visible")
    res = {"device": torch.cuda.get_device_name(0), "rounds": FT.ROUNDS, "shapes": {}}
    for B, T, N, Dx in (a.shape or FT.SHAPES):
        fns, d_mean, d_min = arms(B, T, N, Dx)
        batch = 20 if T * N <= 200 * 128 else 3
        r = FT.measure(fns, batch)
        res["shapes"]["B%d T%d N%d Dx%d" % (B, T, N, Dx)] = dict(r, batch=batch, distinct_mean=d_mean, distinct_min=d_min)
        for k, v in r.items():
            print("B%-3d T%-5d N%-4d Dx%d  %-20s median %8.4f ms  (min %8.4f, max %8.4f)  %7.1f ns per step"
                  % (B, T, N, Dx, k, v["median_ms"], v["min_ms"], v["max_ms"], v["median_ms"] * 1e6 / T), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
