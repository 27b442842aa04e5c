"""Time of the missing-observation backward simulation (psvo_bsim_forward_wobs_missing, psvo_bsim_backward_wobs_missing) beside its
static twin (psvo_bsim_forward_wobs, psvo_bsim_backward_wobs), and of psvo_filter_backward_wobs_missing_ext beside
psvo_filter_backward_wobs_ext, device events; with --errors, the fp32-against-fp64 errors of both routes on the shapes of
tests/test_gpu_missing_bsim.py.

    python tools/missing_bsim_timing.py [--out profiles/missing_bsim_timing.json] [--shape B T N M Dx H] [--Dy 3 10 32] [--errors]

Four arms per width on identical filter outputs, weights, noise and observations: the static wide pair twice (two arms of the
same code: what they differ by is the spread of the measurement), the missing pair on the same all-observed rows, and the missing
pair with 30 % of the entries NaN.  The reverse filter runs behind each backward simulation on its d Fm / d logW (the EXT
kernels).  Every native launch is bracketed by two events through ops.set_timing_hook, as bench.py does; the arms alternate round
after round and the figure of an entry point is the median over the rounds (tools/wobs_bsim_timing.py: warm-up rounds first),
with minimum and maximum.  The weight gradients are the same kernels in every arm and are listed under their own names.
Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARMS = ("static", "static_again", "missing_all_observed", "missing_30pct")


def arms(B, T, N, M, Dx, Dy, H):
    import torch
    from psvo_amd import ops
    g = torch.Generator().manual_seed(0)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    mlp = lambda din, dout: (rn(din, H, scale=0.3), rn(H, scale=0.1), rn(H, dout, scale=0.3), rn(dout, scale=0.1))
    sig = lambda d: (0.5 + torch.rand(d, generator=g)).cuda()
    q1, gnet, q1inv = mlp(Dx, Dx), mlp(Dx, Dy), mlp(Dx, Dx)
    sig_q1, sig_q2, sig_g = sig(Dx), sig(Dx), sig(Dy)
    mu2, m0, sig0 = rn(T, B, Dx), rn(B, Dx), sig(Dx)
    obs = rn(T, B, Dy, scale=1.5)
    gaps = obs.masked_fill(torch.rand(T, B, Dy, generator=g).cuda() < 0.3, float("nan"))
    eps, u = rn(T, B, Dx, N), torch.rand(T, B, N, generator=g).cuda()
    bs_rest = (sig(Dx), sig_g, sig(Dx), sig(Dx), rn(T, B, Dx), rn(B, Dx), sig(Dx), m0, sig0)
    eps_b, u_b, dscore = rn(T, B, Dx, N, M), torch.rand(T, B, N, generator=g).cuda(), rn(B, N)
    fdesc, bdesc = ops.make_desc(B, T, N, 1, Dx, Dy, H), ops.make_desc(B, T, N, M, Dx, Dy, H)

    def make(y, missing):
        fargs = (fdesc, q1, None, gnet, sig_q1, sig_q2, None, sig_g, mu2, m0, sig0, m0, sig0, y, eps)
        # (the filter's forward pass is the same in the arms of a kind and is not what this tool is about: run once)
        filt = (ops.filter_forward_wobs_missing if missing else ops.filter_forward_wobs)(*fargs, u=u)
        bargs = (bdesc, filt, q1, gnet, q1inv) + bs_rest + (y, eps_b)
        fwd = ops.bsim_forward_wobs_missing if missing else ops.bsim_forward_wobs
        bwd = ops.bsim_backward_wobs_missing if missing else ops.bsim_backward_wobs

        def run():
            bs = fwd(*bargs, u_b=u_b, save=True)
            r = bwd(*bargs, bs, dscore)
            return ops.filter_backward(*fargs, filt, dlse=r["dlse"], dFm=r["dFm"], dlogW=r["dlogW"], wobs=True, missing=missing)
        return run
    return [make(obs, False), make(obs, False), make(obs, True), make(gaps, True)]


def _key(name):
    for word, key in (("bsim_forward", "bsim forward"), ("bsim_backward", "bsim reverse"), ("filter_backward", "filter reverse (EXT)")):
        if word in name:
            return key
    return name


def errors():
    """fp32 against fp64 on the parity cases of tests/test_gpu_missing_bsim.py (seed 3), and at the same shapes with Dy >= 3 the
    static wide route against the unmodified oracle: the largest absolute error of every compared quantity"""
    import torch
    from tests import helpers as Hh
    from tests import missing_bsim_reference as MB
    from tests import test_gpu_missing_bsim as TG
    rows = []
    e = lambda a, b: float((a - b).abs().max())

    def row(route, case, z, log, z_ref, ref):
        bs = log["bsim"]
        rows.append(dict(route=route, case="-".join(map(str, case)),
                         bwX=e(Hh.part_to_ref(bs["bwX"]), ref["bw_Xs"]), flp=e(Hh.w_to_ref(bs["flp"]), ref["f_log_probs"]),
                         glp=e(Hh.w_to_ref(bs["glp"]), ref["g_log_probs"]), Omega=e(Hh.w_to_ref(bs["Omega"]), ref["bw_log_Omegas"]),
                         elbo_rel=abs(float(z) - float(z_ref)) / abs(float(z_ref))))
    for case in TG.CASES:
        FLAGS, model, smc, obs, noise, _, _ = TG._case(case, 3)
        z_ref, ref = MB.run_oracle(model, FLAGS, obs, noise)
        with torch.no_grad():
            z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=MB.hip_noise(noise, MB.teacher(ref)))
        row("missing", case, z, log, z_ref, ref)
        if case[2] >= 3 and case[5] != TG.COUNT:        # (the count reference of the static route is tests/count_reference.py's)
            FLAGS, model, smc, obs, noise, _, _ = TG._case(case, 3, mask=False, flags=dict(BSim_wide_obs=True))
            z_ref, ref = Hh.run_oracle(model, FLAGS, "PSVO", obs, noise)
            with torch.no_grad():
                z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=MB.hip_noise(noise, MB.teacher(ref)))
            row("static", case, z, log, z_ref, ref)
    torch.cuda.synchronize()
    for r in rows:
        print("%-8s %-28s bwX %.3e flp %.3e glp %.3e Omega %.3e ELBO rel %.3e"
              % (r["route"], r["case"], r["bwX"], r["flp"], r["glp"], r["Omega"], r["elbo_rel"]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=6, default=[8, 100, 64, 16, 3, 32], metavar=("B", "T", "N", "M", "Dx", "H"))
    ap.add_argument("--Dy", type=int, nargs="+", default=[3, 10, 32])
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("missing_bsim_timing.py measures on the GPU: none is visible")
    from count_timing import measure_arms
    from wobs_bsim_timing import ROUNDS, measure
    B, T, N, M, Dx, H = a.shape
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "shape": dict(B=B, T=T, N=N, M=M, Dx=Dx, H=H), "Dy": {}}
    for Dy in a.Dy:
        per = dict(zip(ARMS, measure_arms(measure, arms(B, T, N, M, Dx, Dy, H))))
        rows = {}
        for name, r in per.items():
            for k, v in r.items():
                rows.setdefault(_key(k), {})[name] = v
        res["Dy"][str(Dy)] = rows
        for key in sorted(rows):
            base = rows[key]["static"]["median_ms"]
            print("Dy %2d %-22s " % (Dy, key) + "   ".join(
                "%s %.4f (%.4f, %.4f) x%.3f" % (n, rows[key][n]["median_ms"], rows[key][n]["min_ms"], rows[key][n]["max_ms"],
                                                rows[key][n]["median_ms"] / base) for n in ARMS if n in rows[key]), flush=True)
    if a.errors:
        res["errors"] = errors()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
