"""Time of the count emission (psvo_desc.emission = 2) beside the Gaussian one (emission = 0) in the four wide-observation kernels,
device events.

    python tools/count_timing.py [--out profiles/count_timing.json] [--shape B T N M Dx H] [--Dy 3 10 32]

Two arms per width on identical inputs and weights: the wide forward filter (psvo_filter_forward_wobs), the wide reverse filter
(psvo_filter_backward_wobs with its weight gradients), the wide backward simulation forward and reverse
(psvo_bsim_forward_wobs, psvo_bsim_backward_wobs).  Observations are counts poisson(4 U[0, 1)) in both arms and sig_g is ones in
both, so that the arms differ in the emission alone.  Every native launch is bracketed by two events through
ops.set_timing_hook, as bench.py does; the arms alternate round after round, and the figure of an entry point is the median over
the rounds (tools/wobs_bsim_timing.py: warm-up rounds first), with minimum and maximum.  Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def arm(B, T, N, M, Dx, Dy, H, emission):
    import torch
    from psvo_amd import ops
    g = torch.Generator().manual_seed(0)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    mlp = lambda din, dout: (rn(din, H, scale=0.3), rn(H, scale=0.1), rn(H, dout, scale=0.3), rn(dout, scale=0.1))
    sig = lambda d: (0.5 + torch.rand(d, generator=g)).cuda()
    q1, gnet, q1inv = mlp(Dx, Dx), mlp(Dx, Dy), mlp(Dx, Dx)
    sig_q1, sig_q2, sig_g = sig(Dx), sig(Dx), torch.ones(Dy).cuda()
    mu2, m0, sig0 = rn(T, B, Dx), rn(B, Dx), sig(Dx)
    obs = torch.poisson(4.0 * torch.rand(T, B, Dy, generator=g), generator=g).cuda()
    eps, u = rn(T, B, Dx, N), torch.rand(T, B, N, generator=g).cuda()
    dlse = rn(T, B)
    bargs = (sig(Dx), sig_g, sig(Dx), sig(Dx), rn(T, B, Dx), rn(B, Dx), sig(Dx), rn(B, Dx), sig(Dx), obs, rn(T, B, Dx, N, M))
    u_b, dscore = torch.rand(T, B, N, generator=g).cuda(), rn(B, N)
    fdesc = ops.make_desc(B, T, N, 1, Dx, Dy, H, emission=emission)         # bootstrap wiring with q2, resampling on
    bdesc = ops.make_desc(B, T, N, M, Dx, Dy, H, emission=emission)
    fargs = (fdesc, q1, None, gnet, sig_q1, sig_q2, None, sig_g, mu2, m0, sig0, m0, sig0, obs, eps)

    def run():
        filt = ops.filter_forward(*fargs, u=u, entry="psvo_filter_forward_wobs")
        ops.filter_backward(*fargs, filt, dlse=dlse, wobs=True)
        bs = ops.bsim_forward_wobs(bdesc, filt, q1, gnet, q1inv, *bargs, u_b=u_b, save=True)
        return ops.bsim_backward_wobs(bdesc, filt, q1, gnet, q1inv, *bargs, bs, dscore)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=6, default=[32, 200, 128, 16, 3, 32], metavar=("B", "T", "N", "M", "Dx", "H"))
    ap.add_argument("--Dy", type=int, nargs="+", default=[3, 10, 32])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("count_timing.py measures on the GPU: none is visible")
    from wobs_bsim_timing import ROUNDS, measure
    B, T, N, M, Dx, H = a.shape
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "shape": dict(B=B, T=T, N=N, M=M, Dx=Dx, H=H), "Dy": {}}
    for Dy in a.Dy:
        per = {}
        per["gaussian"], per["count"] = measure_arms(measure, [arm(B, T, N, M, Dx, Dy, H, 0), arm(B, T, N, M, Dx, Dy, H, 2)])
        res["Dy"][str(Dy)] = per
        for k in sorted(per["gaussian"]):
            g_, c_ = per["gaussian"][k], per["count"][k]
            print("Dy %2d %-30s gaussian %8.4f ms (min %8.4f, max %8.4f)   count %8.4f ms (min %8.4f, max %8.4f)   x%.3f" % (
                Dy, k, g_["median_ms"], g_["min_ms"], g_["max_ms"], c_["median_ms"], c_["min_ms"], c_["max_ms"],
                c_["median_ms"] / g_["median_ms"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def measure_arms(measure, arms):
    """tools/wobs_bsim_timing.py::measure keys its samples by entry point; both arms here launch the same entry points.  Each arm
    is wrapped so that its launches are recorded under its own names: the hook sees name + '#' + arm index."""
    from psvo_amd import ops
    tagged = []
    for i, run in enumerate(arms):
        def wrapped(run=run, i=i):
            inner = ops._HOOK
            ops.set_timing_hook(lambda name, phase, stream: inner("%s#%d" % (name, i), phase, stream))
            try:
                return run()
            finally:
                ops.set_timing_hook(inner)
        tagged.append(wrapped)
    r = measure(tagged)
    return tuple({k.split("#")[0]: v for k, v in r.items() if k.endswith("#%d" % i)} for i in range(len(arms)))


if __name__ == "__main__":
    main()
