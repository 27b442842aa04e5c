"""Time of the two input-driven additions beside the kernels they are built on, device events around every native launch:

  * psvo_particle_forecast_input beside psvo_particle_forecast_missing (twice: two arms of the same code, what they differ by is
    the spread of the measurement), on one cloud, one set of weights and one set of injected normals;
  * psvo_filter_forward_wobs_input_adaptive / psvo_filter_backward_wobs_input_adaptive beside the input pair (twice, likewise),
    at a threshold of one half on identical weights, noise, observations and bias rows.

    python tools/exo_forecast_timing.py [--out profiles/exo_forecast_timing.json] [--shape B T N Dx Dy H] [--K 30]

Every launch is bracketed by two events through ops.set_timing_hook, as bench.py does; the arms alternate round after round and
the figure of an entry point is the median over the rounds (tools/wobs_bsim_timing.py: warm-up rounds first), with minimum and
maximum.  Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPE = (64, 200, 128, 2, 1, 32)       # B, T, N, Dx, Dy, H


def forecast_arms(B, T, N, Dx, Dy, H, K):
    import torch
    from psvo_amd import ops
    g = torch.Generator().manual_seed(0)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    mlp = lambda din, dout: (rn(din, H, scale=0.3), rn(H, scale=0.1), rn(H, dout, scale=0.3), rn(dout, scale=0.1))
    sig = lambda d: (0.5 + torch.rand(d, generator=g)).cuda()
    f, gnet, sig_f, sig_g = mlp(Dx, Dx), mlp(Dx, Dy), sig(Dx), sig(Dy)
    X, obs, eps, hb = rn(T, B, Dx, N), rn(T, B, Dy, scale=1.5), rn(K, T, B, Dx, N), rn(T + K, B, H)
    desc = ops.make_desc(B, T, N, 1, Dx, Dy, H)

    def make(**kw):
        return lambda: ops.particle_forecast(desc, K, f, gnet, sig_f, sig_g, X, obs=obs, eps=eps, **kw)
    return [make(missing=True), make(missing=True), make(hb_f=hb)]


def filter_arms(B, T, N, Dx, Dy, H):
    import torch
    from psvo_amd import ops
    g = torch.Generator().manual_seed(0)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    mlp = lambda din, dout: (rn(din, H, scale=0.3), rn(H, scale=0.1), rn(H, dout, scale=0.3), rn(dout, scale=0.1))
    sig = lambda d: (0.5 + torch.rand(d, generator=g)).cuda()
    q1, gnet = mlp(Dx, Dx), mlp(Dx, Dy)
    sig_q1, sig_q2, sig_g = sig(Dx), sig(Dx), sig(Dy)
    mu2, m0, sig0 = rn(T, B, Dx), rn(B, Dx), sig(Dx)
    obs, eps, u, dlse = rn(T, B, Dy, scale=1.5), rn(T, B, Dx, N), torch.rand(T, B, N, generator=g).cuda(), rn(T, B)
    hb = (rn(T, B, H), None)
    desc = ops.make_desc(B, T, N, 1, Dx, Dy, H, bootstrap=True)
    fargs = (desc, q1, None, gnet, sig_q1, sig_q2, None, sig_g, mu2, m0, sig0, m0, sig0, obs, eps)

    def make(adaptive):
        def run():
            if adaptive:
                filt = ops.filter_forward_wobs_input_adaptive(*fargs, u=u, hb=hb, ess_frac=0.5)
                return ops.filter_backward_wobs_input_adaptive(*fargs, filt, dlse=dlse, hb=hb)
            filt = ops.filter_forward_wobs_input(*fargs, u=u, hb=hb)
            return ops.filter_backward_wobs_input(*fargs, filt, dlse=dlse, hb=hb)
        return run
    share = float((ops.filter_forward_wobs_input_adaptive(*fargs, u=u, hb=hb, ess_frac=0.5)["rs"] != 0).float().mean())
    return [make(False), make(False), make(True)], share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=6, default=list(SHAPE), metavar=("B", "T", "N", "Dx", "Dy", "H"))
    ap.add_argument("--K", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("exo_forecast_timing.py measures on the GPU: none is visible")
    from count_timing import measure_arms
    from wobs_bsim_timing import ROUNDS, measure
    B, T, N, Dx, Dy, H = a.shape
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "shape": dict(B=B, T=T, N=N, Dx=Dx, Dy=Dy, H=H, K=a.K)}
    fc = dict(zip(("missing", "missing_again", "input"), measure_arms(measure, forecast_arms(B, T, N, Dx, Dy, H, a.K))))
    arms, share = filter_arms(B, T, N, Dx, Dy, H)
    fl = dict(zip(("input", "input_again", "input_adaptive"), measure_arms(measure, arms)))
    res["forecast"], res["filter"], res["resampled_share"] = fc, fl, share
    for title, per in (("forecast", fc), ("filter", fl)):
        for arm, r in per.items():
            for k, v in sorted(r.items()):
                print("%-8s %-15s %-44s median %8.4f ms  (min %8.4f, max %8.4f)"
                      % (title, arm, k, v["median_ms"], v["min_ms"], v["max_ms"]), flush=True)
    print("adaptive arm: resampled at %.1f %% of the (step, sequence) pairs" % (100 * share))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
