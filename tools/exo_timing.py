"""Time of the input-driven filter kernels (psvo_filter_forward_wobs_input, psvo_filter_backward_wobs_input) and of
psvo_mlp_wgrad_rowbias beside the missing-observation pair and psvo_mlp_wgrad, device events.

    python tools/exo_timing.py [--out profiles/exo_timing.json] [--shapes small bench] [--separate_f]

Three arms per shape on identical weights, noise and observations: the missing-observation pair twice (two arms of the same code:
what they differ by is the spread of the measurement) and the input pair with bias rows hb of standard normals.  Bootstrap wiring
with q2 (or a separate f: two bias rows per step and two weight-gradient launches), resampling on, Dy >= 3 so that MLP_g's weight
gradient has a name of its own.  Every native launch is bracketed by two events through ops.set_timing_hook, as bench.py does; the
arms alternate round after round and the figure of an entry point is the median over the rounds (tools/wobs_bsim_timing.py:
warm-up rounds first), with minimum and maximum.  Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARMS = ("missing", "missing_again", "input")
SHAPES = {"small": (8, 50, 32, 2, 3, 16), "bench": (64, 200, 128, 3, 10, 32)}       # B, T, N, Dx, Dy, H
KEY = {"psvo_filter_forward_wobs_missing": "forward", "psvo_filter_forward_wobs_input": "forward",
       "psvo_filter_backward_wobs_missing": "reverse", "psvo_filter_backward_wobs_input": "reverse",
       "psvo_mlp_wgrad": "wgrad_q1_f", "psvo_mlp_wgrad_rowbias": "wgrad_q1_f"}


def arms(B, T, N, Dx, Dy, H, separate_f):
    import torch
    from psvo_amd import ops
    g = torch.Generator().manual_seed(0)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    mlp = lambda din, dout: (rn(din, H, scale=0.3), rn(H, scale=0.1), rn(H, dout, scale=0.3), rn(dout, scale=0.1))
    sig = lambda d: (0.5 + torch.rand(d, generator=g)).cuda()
    q1, gnet = mlp(Dx, Dx), mlp(Dx, Dy)
    f = mlp(Dx, Dx) if separate_f else None
    sig_q1, sig_q2, sig_g = sig(Dx), sig(Dx), sig(Dy)
    sig_f = sig(Dx) if separate_f else None
    mu2, m0, sig0 = rn(T, B, Dx), rn(B, Dx), sig(Dx)
    obs = rn(T, B, Dy, scale=1.5)
    eps, u = rn(T, B, Dx, N), torch.rand(T, B, N, generator=g).cuda()
    dlse = rn(T, B)
    hb = (rn(T, B, H), rn(T, B, H) if separate_f else None)
    desc = ops.make_desc(B, T, N, 1, Dx, Dy, H, bootstrap=not separate_f)
    fargs = (desc, q1, f, gnet, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, m0, sig0, obs, eps)

    def make(with_input):
        def run():
            if with_input:
                filt = ops.filter_forward_wobs_input(*fargs, u=u, hb=hb)
                return ops.filter_backward_wobs_input(*fargs, filt, dlse=dlse, hb=hb)
            filt = ops.filter_forward_wobs_missing(*fargs, u=u)
            return ops.filter_backward_wobs_missing(*fargs, filt, dlse=dlse)
        return run
    return [make(False), make(False), make(True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["small", "bench"], choices=sorted(SHAPES))
    ap.add_argument("--separate_f", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("exo_timing.py measures on the GPU: none is visible")
    from count_timing import measure_arms
    from wobs_bsim_timing import ROUNDS, measure
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "separate_f": a.separate_f, "shapes": {}}
    for name in a.shapes:
        B, T, N, Dx, Dy, H = SHAPES[name]
        per = dict(zip(ARMS, measure_arms(measure, arms(B, T, N, Dx, Dy, H, a.separate_f))))
        rows = {}
        for arm, r in per.items():
            for k, v in r.items():
                rows.setdefault(KEY.get(k, k), {})[arm] = v
        res["shapes"][name] = {"shape": dict(B=B, T=T, N=N, Dx=Dx, Dy=Dy, H=H), "launches": rows}
        for key in sorted(rows):
            base = rows[key]["missing"]["median_ms"]
            print("%-5s %-24s " % (name, key) + "   ".join(
                "%s %.4f (%.4f, %.4f) x%.3f" % (n, rows[key][n]["median_ms"], rows[key][n]["min_ms"], rows[key][n]["max_ms"],
                                                rows[key][n]["median_ms"] / base) for n in ARMS if n in rows[key]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
