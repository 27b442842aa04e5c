"""Time of the adaptive missing-observation filter kernels (psvo_filter_forward_wobs_missing_adaptive and its reverse) beside the
missing pair and the adaptive wide pair, and of psvo_particle_forecast_missing beside psvo_particle_forecast, device events.

    python tools/missing_adaptive_timing.py [--out profiles/missing_adaptive_timing.json] [--shape B T N Dx H] [--Dy 3 10 20 32]

Filter arms per width, on identical weights, noise and observations (bootstrap wiring with q2, threshold 0.5, the shapes of
profiles/missing_obs.md and profiles/wobs_adaptive.md):
    missing_30pct          psvo_filter_*_wobs_missing, 30 % of the entries NaN                    (parent kernel)
    msad_30pct             the new pair on the same rows
    adaptive_all_observed  psvo_filter_*_wobs_adaptive on the all-observed rows (Dy >= 3)         (parent kernel)
    msad_all_observed      the new pair on the same rows
Forecast arms (K = 8 horizons on the filter's shape, equal weights, transition noise):
    forecast               psvo_particle_forecast on the all-observed rows                       (parent kernel)
    forecast_ms_observed   psvo_particle_forecast_missing on the same rows
    forecast_ms_30pct      ... with 30 % of the entries NaN
Every native launch is bracketed by two events through ops.set_timing_hook, as bench.py does; the arms alternate round after
round and the figure of an entry point is the median over the rounds (tools/wobs_bsim_timing.py: warm-up rounds first), with
minimum and maximum.  The adaptive arms resample where the weights say so, which differs between all-observed and gappy rows:
compare an arm with the parent kernel on the SAME rows only.  The reverse wrappers also launch the weight gradients, which are
the same kernels in every arm and are listed under their own names.  Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FILTER_ARMS = ("missing_30pct", "msad_30pct", "adaptive_all_observed", "msad_all_observed")
FORECAST_ARMS = ("forecast", "forecast_ms_observed", "forecast_ms_30pct")
TAU, K = 0.5, 8


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
    X, eps_p = rn(T, B, Dx, N), rn(K, T, B, Dx, N)
    desc = ops.make_desc(B, T, N, 1, Dx, Dy, H)

    def filt_arm(y, fwd, bwd, **route):
        fargs = (desc, q1, None, gnet, sig_q1, sig_q2, None, sig_g, mu2, m0, sig0, m0, sig0, y, eps)

        def run():
            filt = fwd(*fargs, u=u, **route)
            return bwd(*fargs, filt, dlse=dlse)
        return run

    def fc_arm(y, missing):
        return lambda: ops.particle_forecast(desc, K, q1, gnet, sig_q1, sig_g, X, obs=y, eps=eps_p, missing=missing)
    msad = (ops.filter_forward_wobs_missing_adaptive, ops.filter_backward_wobs_missing_adaptive)
    out = [("missing_30pct", filt_arm(gaps, ops.filter_forward_wobs_missing, ops.filter_backward_wobs_missing)),
           ("msad_30pct", filt_arm(gaps, *msad, ess_frac=TAU))]
    if Dy >= 3:
        out.append(("adaptive_all_observed", filt_arm(obs, ops.filter_forward_wobs_adaptive, ops.filter_backward_wobs_adaptive,
                                                      ess_frac=TAU)))
    out += [("msad_all_observed", filt_arm(obs, *msad, ess_frac=TAU)),
            ("forecast", fc_arm(obs, False)), ("forecast_ms_observed", fc_arm(obs, True)), ("forecast_ms_30pct", fc_arm(gaps, True))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=5, default=[32, 200, 128, 3, 32], metavar=("B", "T", "N", "Dx", "H"))
    ap.add_argument("--Dy", type=int, nargs="+", default=[3, 10, 20, 32])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("missing_adaptive_timing.py measures on the GPU: none is visible")
    from count_timing import measure_arms
    from wobs_bsim_timing import ROUNDS, measure
    B, T, N, Dx, H = a.shape
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "shape": dict(B=B, T=T, N=N, Dx=Dx, H=H), "tau": TAU, "K": K,
           "Dy": {}}
    for Dy in a.Dy:
        named = arms(B, T, N, Dx, Dy, H)
        per = dict(zip([n for n, _ in named], measure_arms(measure, [r for _, r in named])))
        rows = {}
        for name, r in per.items():
            for k, v in r.items():
                key = ("forward" if "filter_forward" in k else "reverse" if "filter_backward" in k
                       else "forecast" if "particle_forecast" in k else k)
                rows.setdefault(key, {})[name] = v
        res["Dy"][str(Dy)] = rows
        for key in sorted(rows):
            print("Dy %2d %-22s " % (Dy, key) + "   ".join(
                "%s %.4f (%.4f, %.4f)" % (n, rows[key][n]["median_ms"], rows[key][n]["min_ms"], rows[key][n]["max_ms"])
                for n in FILTER_ARMS + FORECAST_ARMS if n in rows[key]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
