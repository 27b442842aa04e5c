"""Time of the adaptive wide-observation filter kernels (psvo_filter_forward_wobs_adaptive, psvo_filter_backward_wobs_adaptive)
beside their static twins (psvo_filter_forward_wobs, psvo_filter_backward_wobs, resample = 1), device events.

    python tools/wobs_adaptive_timing.py [--out profiles/wobs_adaptive_timing.json] [--shape B T N Dx Dy H] [--tau 0.5]
                                         [--emission 0]

Five arms on identical inputs and weights, alternating inside every round: the static pair, the adaptive pair free running at
--tau, the adaptive pair with every decision forced to 1 (the static filter's work plus the bookkeeping), with every decision
forced to 0 (no step inherits its draw; the reverse pass skips every walk over the children), and the static pair once more --
the distance between the first and the last line is the run-to-run spread of the session.  Each arm times the forward kernel and
the reverse kernel alone (the weight-gradient launches behind the reverse kernel are the same in every arm and are left out).
Every native launch is bracketed by two events through ops.set_timing_hook, as bench.py does; the figure of an entry point is
the median over the rounds (tools/wobs_bsim_timing.py: warm-up rounds first), with minimum and maximum.  The free-running arm's
resampling rate is printed with it.  Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARMS = ("static (first)", "adaptive, free running", "adaptive, forced 1", "adaptive, forced 0", "static (last)")


def arms(B, T, N, Dx, Dy, H, tau, emission):
    import torch
    from psvo_amd import ops
    g = torch.Generator().manual_seed(0)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    mlp = lambda din, dout: (rn(din, H, scale=0.3), rn(H, scale=0.1), rn(H, dout, scale=0.3), rn(dout, scale=0.1))
    sig = lambda d: (0.5 + torch.rand(d, generator=g)).cuda()
    q1, gnet = mlp(Dx, Dx), mlp(Dx, Dy)
    sig_q1, sig_q2 = sig(Dx), sig(Dx)
    sig_g = torch.ones(Dy).cuda() if emission == 2 else (2.0 + 2.0 * torch.rand(Dy, generator=g)).cuda()
    mu2, m0, sig0 = rn(T, B, Dx), rn(B, Dx), sig(Dx)
    if emission == 2:
        obs = torch.poisson(4.0 * torch.rand(T, B, Dy, generator=g), generator=g).cuda()
    else:
        obs = rn(T, B, Dy)
    eps, u = rn(T, B, Dx, N), torch.rand(T, B, N, generator=g).cuda()
    dlse = rn(T, B)
    desc = ops.make_desc(B, T, N, 1, Dx, Dy, H, emission=emission)         # bootstrap wiring with q2, resampling on
    fargs = (desc, q1, None, gnet, sig_q1, sig_q2, None, sig_g, mu2, m0, sig0, m0, sig0, obs, eps)
    ones = torch.ones(T, B, dtype=torch.int32).cuda()
    zeros = torch.zeros(T, B, dtype=torch.int32).cuda()
    seen = {}

    def static():
        filt = ops.filter_forward_wobs(*fargs, u=u)
        return ops.filter_backward_wobs(*fargs, filt, dlse=dlse, defer_wgrad=True)

    def adaptive(rs_in, key):
        def run():
            filt = ops.filter_forward_wobs_adaptive(*fargs, u=u, ess_frac=tau, rs_in=rs_in)
            seen[key] = filt["rs"]
            return ops.filter_backward_wobs_adaptive(*fargs, filt, dlse=dlse, defer_wgrad=True)
        return run
    return [static, adaptive(None, "free"), adaptive(ones, "ones"), adaptive(zeros, "zeros"), static], seen


def measure_arms(measure, runs):
    """tools/count_timing.py::measure_arms: each arm's launches are recorded under its own names (name + '#' + arm index)"""
    from psvo_amd import ops
    tagged = []
    for i, run in enumerate(runs):
        def wrapped(run=run, i=i):
            inner = ops._HOOK
            ops.set_timing_hook(lambda name, phase, stream: inner("%s#%d" % (name, i), phase, stream))
            try:
                return run()
            finally:
                ops.set_timing_hook(inner)
        tagged.append(wrapped)
    r = measure(tagged)
    return [{k.split("#")[0]: v for k, v in r.items() if k.endswith("#%d" % i)} for i in range(len(runs))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=6, default=[32, 200, 128, 3, 10, 32], metavar=("B", "T", "N", "Dx", "Dy", "H"))
    ap.add_argument("--tau", type=float, default=0.5)
    ap.add_argument("--emission", type=int, default=0, choices=(0, 1, 2))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("wobs_adaptive_timing.py measures on the GPU: none is visible")
    from wobs_bsim_timing import ROUNDS, measure
    B, T, N, Dx, Dy, H = a.shape
    runs, seen = arms(B, T, N, Dx, Dy, H, a.tau, a.emission)
    per = measure_arms(measure, runs)
    rate = float((seen["free"] != 0).float().mean())
    assert bool((seen["ones"] == 1).all()) and bool((seen["zeros"] == 0).all())
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "shape": dict(B=B, T=T, N=N, Dx=Dx, Dy=Dy, H=H),
           "tau": a.tau, "emission": a.emission, "free_running_rate": rate, "arms": dict(zip(ARMS, per))}
    print("shape B %d T %d N %d Dx %d Dy %d H %d, emission %d, tau %g: free-running resampling rate %.3f" % (
        B, T, N, Dx, Dy, H, a.emission, a.tau, rate))
    for name, p in zip(ARMS, per):
        for k in sorted(p):
            v = p[k]
            print("%-26s %-38s median %8.4f ms  (min %8.4f, max %8.4f)" % (name, k, v["median_ms"], v["min_ms"], v["max_ms"]),
                  flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
