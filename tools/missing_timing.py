"""Time of the missing-observation filter kernels (psvo_filter_forward_wobs_missing, psvo_filter_backward_wobs_missing) beside their
static twins (psvo_filter_forward_wobs, psvo_filter_backward_wobs), device events.

    python tools/missing_timing.py [--out profiles/missing_timing.json] [--shape B T N Dx H] [--Dy 3 10 20 32]

Four arms per width on identical weights, noise and observations: the static wide pair twice (two arms of the same code: what
they differ by is the spread of the measurement), the missing pair on the same all-observed rows, and the missing pair with 30 %
of the entries NaN.  Bootstrap wiring with q2, resampling on, the shapes of profiles/wobs_filter.md.  Every native launch is
bracketed by two events through ops.set_timing_hook, as bench.py does; the arms alternate round after round and the figure of an
entry point is the median over the rounds (tools/wobs_bsim_timing.py: warm-up rounds first), with minimum and maximum.  The
reverse wrappers also launch the weight gradients, which are the same kernels in every arm and are listed under their own names.
Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARMS = ("static", "static_again", "missing_all_observed", "missing_30pct")


def arms(B, T, N, Dx, Dy, H):
    import torch
    from psvo_amd import ops
    g = torch.Generator().manual_seed(0)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    mlp = lambda din, dout: (rn(din, H, scale=0.3), rn(H, scale=0.1), rn(H, dout, scale=0.3), rn(dout, scale=0.1))
    sig = lambda d: (0.5 + torch.rand(d, generator=g)).cuda()
    q1, gnet = mlp(Dx, Dx), mlp(Dx, Dy)
    sig_q1, sig_q2, sig_g = sig(Dx), sig(Dx), sig(Dy)
    mu2, m0, sig0 = rn(T, B, Dx), rn(B, Dx), sig(Dx)
    obs = rn(T, B, Dy, scale=1.5)
    gaps = obs.masked_fill(torch.rand(T, B, Dy, generator=g).cuda() < 0.3, float("nan"))
    eps, u = rn(T, B, Dx, N), torch.rand(T, B, N, generator=g).cuda()
    dlse = rn(T, B)
    desc = ops.make_desc(B, T, N, 1, Dx, Dy, H)

    def make(y, missing):
        fargs = (desc, q1, None, gnet, sig_q1, sig_q2, None, sig_g, mu2, m0, sig0, m0, sig0, y, eps)
        fwd = ops.filter_forward_wobs_missing if missing else ops.filter_forward_wobs
        bwd = ops.filter_backward_wobs_missing if missing else ops.filter_backward_wobs

        def run():
            filt = fwd(*fargs, u=u)
            return bwd(*fargs, filt, dlse=dlse)
        return run
    return [make(obs, False), make(obs, False), make(obs, True), make(gaps, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=5, default=[32, 200, 128, 3, 32], metavar=("B", "T", "N", "Dx", "H"))
    ap.add_argument("--Dy", type=int, nargs="+", default=[3, 10, 20, 32])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("missing_timing.py measures on the GPU: none is visible")
    from count_timing import measure_arms
    from wobs_bsim_timing import ROUNDS, measure
    B, T, N, Dx, H = a.shape
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "shape": dict(B=B, T=T, N=N, Dx=Dx, H=H), "Dy": {}}
    for Dy in a.Dy:
        per = dict(zip(ARMS, measure_arms(measure, arms(B, T, N, Dx, Dy, H))))
        # the arms launch entry points of different names: key the filter kernels by direction
        rows = {}
        for name, r in per.items():
            for k, v in r.items():
                key = "forward" if "filter_forward" in k else "reverse" if "filter_backward" in k else k
                rows.setdefault(key, {})[name] = v
        res["Dy"][str(Dy)] = rows
        for key in sorted(rows):
            base = rows[key]["static"]["median_ms"]
            print("Dy %2d %-22s " % (Dy, key) + "   ".join(
                "%s %.4f (%.4f, %.4f) x%.3f" % (n, rows[key][n]["median_ms"], rows[key][n]["min_ms"], rows[key][n]["max_ms"],
                                                rows[key][n]["median_ms"] / base) for n in ARMS if n in rows[key]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
