"""PSVO on wide observations (3 <= Dy <= 32, FLAGS.BSim_wide_obs) on the GPU: psvo_bsim_forward_wobs, psvo_bsim_backward_wobs
(psvo_amd/csrc/bsim_wobs.hip) and psvo_filter_backward_wobs_ext against the fp64 oracle.

Cases are the smallest shapes that reach each way the kernels can go wrong (see CASES).  Tolerances are those of the plain
path: values as tests/test_gpu_parity.py::test_teacher_forced_parity, draws as ::test_free_running_indices (a differing draw is
reported through helpers.replay_with_hip_indices with its distance from the CDF edge), gradients under the rule of
tests/test_gpu_wobs.py::test_every_gradient.  Seeds: model seed 3 for values and draws, 5 for gradients, as there and for the
reason its docstring gives.  With those seeds the fp32 oracle stays, against its own fp64 values, at or below 3.1e-5 in flp /
glp / Omega, 6.5e-5 in logW, 2.2e-6 in bwX, 1.5e-7 relative in the ELBO and 9.6e-4 of a tensor's largest entry in every
gradient on all ten cases, so a failure here is the kernel's, not the model's."""
import math
import os

import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests.test_gpu_instantiations import K32
from tests.test_gpu_large import EDGE_TOL
from tests.test_gpu_parity import _oracle_grads, _pairs, _setup
from tests.test_gpu_wobs import _run_main

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
WIDE = dict(BSim_wide_obs=True)

CASES = [
    # (objective, B, T, N, M, Dx, Dy, H, bootstrap, two_q), extra flags
    (("PSVO", 2, 5, 16, 4, 2, 3, 16, True, True), {}),                # smallest wide Dy; N M = one wave
    (("PSVO", 2, 6, 40, 8, 3, 10, 32, False, True), {}),              # Lorenz widths; separate f; N no multiple of the chains per workgroup
    (("PSVO", 2, 6, 32, 16, 2, 20, 32, True, True), {}),              # vind widths; default M
    (("PSVO", 1, 5, 24, 32, 3, 32, 64, True, True), {}),              # widest Dy, H and M; partly filled workgroup
    (("PSVO", 2, 5, 130, 4, 4, 17, 64, False, True), {}),             # Dx 4; odd Dy; several workgroups per sequence, tile padding
    (("PSVO", 2, 5, 24, 8, 2, 5, 32, True, False), {}),               # no q2
    (("PSVO", 2, 5, 16, 8, 2, 10, 32, True, True), dict(poisson_emission=True)),
    (("PSVO", 2, 5, 16, 4, 3, 10, 32, True, True), dict(BSim_use_single_RNN=True)),     # forward-only encoder
    (("PSVO", 1, 60, 32, 4, 3, 10, 32, True, True), {}),              # long recurrence
    (("PSVO", 1, 4, 512, 4, 4, 32, 32, False, True), {}),             # every limit at once
]
NEW_PREFIXES = ("g.", "q1_inv.", "BSim_q2.", "BSim_q_init.")          # what the backward simulation feeds


def _id(v):
    if isinstance(v, tuple):
        return "-".join(map(str, v))
    return ",".join(sorted(v)) or "plain"


def _wide(case, extra, seed):
    FLAGS, model, smc, obs, noise = _setup(*case, seed=seed, **{**WIDE, **extra})
    assert smc.wide_obs and smc.uses_backward_simulation
    return FLAGS, model, smc, obs, noise


def _teacher(ref):
    return {"idx_f": ref["idx_f"], "idx_b": ref["idx_b"]}


def _hip_noise(noise, teacher):
    nz = Hh.noise_to_hip({**noise, **teacher}, "cuda")
    if "idx_f" in nz:
        nz.pop("u_f", None)
    if "sel_b" in nz:
        nz.pop("u_b", None)
    return nz


@pytest.mark.parametrize("case,extra", CASES, ids=_id)
def test_teacher_forced_values(built_lib, case, extra):
    """filter outputs, bwX, flp, glp, Omega, Xs and the ELBO against the fp64 oracle; idx_f and idx_b teacher-forced"""
    obj = case[0]
    FLAGS, model, smc, obs, noise = _wide(case, extra, 3)
    z_ref, ref = Hh.run_oracle(model, FLAGS, obj, obs, noise)
    nz = _hip_noise(noise, _teacher(ref))
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
    torch.cuda.synchronize()
    filt, bs = log["filter"], log["bsim"]
    assert set(bs) == {"score", "bwX", "flp", "glp", "Omega", "sel"}
    err = lambda a, b: float((a - b).abs().max())
    print("max abs err: X %.3e logW %.3e bwX %.3e flp %.3e glp %.3e Omega %.3e ELBO rel %.3e" % (
        err(Hh.part_to_ref(filt["X"]), ref["X_prevs"]), err(Hh.w_to_ref(filt["logW"]), ref["log_Ws"]),
        err(Hh.part_to_ref(bs["bwX"]), ref["bw_Xs"]), err(Hh.w_to_ref(bs["flp"]), ref["f_log_probs"]),
        err(Hh.w_to_ref(bs["glp"]), ref["g_log_probs"]), err(Hh.w_to_ref(bs["Omega"]), ref["bw_log_Omegas"]),
        abs(float(z) - float(z_ref)) / abs(float(z_ref))))
    assert torch.allclose(Hh.part_to_ref(filt["X"]), ref["X_prevs"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.part_to_ref(filt["Xanc"]), ref["X_ancestors"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.w_to_ref(filt["logW"]), ref["log_Ws"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(filt["lse"].double().cpu(), torch.logsumexp(ref["log_Ws"], 1), atol=5e-4, rtol=1e-5)
    assert torch.allclose(Hh.part_to_ref(bs["bwX"]), ref["bw_Xs"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.w_to_ref(bs["flp"]), ref["f_log_probs"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(Hh.w_to_ref(bs["glp"]), ref["g_log_probs"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(Hh.w_to_ref(bs["Omega"]), ref["bw_log_Omegas"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(log["Xs"].double().cpu(), ref["Xs"], atol=2e-4, rtol=1e-5)
    assert abs(float(z) - float(z_ref)) <= 1e-4 * abs(float(z_ref))


@pytest.mark.parametrize("case,extra", CASES, ids=_id)
def test_free_running_draws(built_lib, case, extra):
    """in-kernel draws of the filter and of the sub-particle pick against the oracle's definition: no index differs"""
    obj = case[0]
    FLAGS, model, smc, obs, noise = _wide(case, extra, 3)
    z_ref, ref = Hh.run_oracle(model, FLAGS, obj, obs, noise)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=Hh.noise_to_hip(noise, "cuda"))
    torch.cuda.synchronize()
    idx = log["filter"]["idx"].permute(0, 2, 1).cpu().long()
    sel = log["bsim"]["sel"].permute(0, 2, 1).cpu().long()
    differ = int((idx != ref["idx_f"]).sum()) + int((sel != ref["idx_b"]).sum())
    if differ:
        _, _, st = Hh.replay_with_hip_indices(model, FLAGS, obj, obs, noise, log)
        print("draws=%d differing=%d flipped=%d worst edge distance=%.3e" % (st["draws"], differ, st["off"], st["worst"]))
        assert st["worst"] <= EDGE_TOL, "a draw that is not on a CDF edge: %s" % st
    assert differ == 0, "%d draws differ from the oracle's (edge flips: see the printed distances)" % differ
    assert abs(float(z) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    assert torch.allclose(log["Xs"].double().cpu(), ref["Xs"], atol=2e-4, rtol=1e-5)


@pytest.mark.parametrize("case,extra", CASES, ids=_id)
def test_every_gradient(built_lib, case, extra):
    """d log_ZSMC / d(every parameter), teacher-forced indices, against fp64 autograd of the oracle"""
    obj = case[0]
    FLAGS, model, smc, obs, noise = _wide(case, extra, 5)
    _, ref0 = Hh.run_oracle(model, FLAGS, obj, obs, noise)
    teacher = _teacher(ref0)
    z_ref, P = _oracle_grads(model, FLAGS, obj, obs, noise, teacher)
    nz = _hip_noise(noise, teacher)
    model.zero_grad()
    z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
    z.backward()
    torch.cuda.synchronize()
    assert abs(float(z.detach()) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    rows = []
    for name, p, ref in _pairs(model, P):
        g = torch.zeros_like(ref) if p.grad is None else p.grad.detach().double().cpu()
        r = torch.zeros_like(ref) if ref.grad is None else ref.grad
        rows.append((name, float((g - r).abs().max()), max(float(r.abs().max()), 1e-6)))
    names = [n for n, _, _ in rows]
    for prefix in NEW_PREFIXES:
        assert any(n.startswith(prefix) for n in names), prefix
    worst = max(rows, key=lambda r: r[1] / r[2])
    print("worst gradient error / largest entry: %s %.3e" % (worst[0], worst[1] / worst[2]))
    over = [r for r in rows if r[1] > 2e-3 * r[2] + 1e-6]
    if over:        # the second clause: the fp32 oracle's own error on the same tensor (computed only when it is needed)
        _, P32 = _oracle_grads(model, FLAGS, obj, obs, noise, teacher, dtype=torch.float32)
        err32 = {}
        for (name, _, ref), (_, _, ref32) in zip(_pairs(model, P), _pairs(model, P32)):
            r = torch.zeros_like(ref) if ref.grad is None else ref.grad
            r32 = torch.zeros_like(ref) if ref32.grad is None else ref32.grad.double()
            err32[name] = float((r32 - r).abs().max())
        bad = [(n, e, s, err32[n]) for n, e, s in over if e > K32 * err32[n]]
        assert not bad, "gradient mismatch (name, max abs err, own scale, fp32 oracle's own err): %s" % bad


@pytest.mark.parametrize("case,extra", [CASES[1], CASES[4]], ids=_id)
def test_two_passes_are_bit_identical(built_lib, case, extra):
    """forward + backward twice in one process, deterministic mode off: the ELBO and every .grad bit for bit"""
    from psvo_amd import ops
    assert not ops.deterministic()
    FLAGS, model, smc, obs, noise = _wide(case, extra, 5)
    nz = Hh.noise_to_hip(noise, "cuda")
    res = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
        z.backward()
        torch.cuda.synchronize()
        res.append((z.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 8
    for n, g in res[0][1].items():
        assert torch.isfinite(g).all() and torch.equal(g, res[1][1][n]), n


# ---- the two entry points on their own -------------------------------------------------------------------------------------
# A restatement of the contract in include/psvo_hip.h (psvo_bsim_forward) in fp64 torch: random filter outputs, every tensor in
# the library's own layout.  It localises a failure to the kernels, not the wiring.
def _mlp(w, x):
    return torch.relu(x @ w[0] + w[1]) @ w[2] + w[3]


def _lognorm(x, mu, sig):
    z = (x - mu) / sig
    return (-0.5 * z * z - torch.log(sig) - 0.5 * math.log(2 * math.pi)).sum(-1)


def _bsim_restated(p, u_b, poisson):
    Fm, logW, lse, eps_b, obs = p["Fm"], p["logW"], p["lse"], p["eps_b"], p["obs"]
    T, B, Dx, N = Fm.shape
    M = eps_b.shape[-1]
    i1, i2 = 1 / p["sig_q1inv"], 1 / p["sig_bq2"]
    c = 1 / (i1 + i2)
    out = {k: [None] * T for k in ("bwX", "flp", "glp", "Omega", "sel")}
    xp, score = None, 0.0
    for t in range(T - 1, -1, -1):
        eps = eps_b[t].permute(0, 2, 3, 1)                              # (B, N, M, Dx)
        if t == T - 1:
            mu, s = p["minit"][:, None, None, :].expand(B, N, M, Dx), p["sig_init"]
        else:
            m1 = _mlp(p["q1_inv"], xp)                                  # (B, N, Dx)
            mu, s = c * (i1 * m1[:, :, None, :] + i2 * p["bmu2"][t][:, None, None, :]), c
        x = mu + s * eps
        q_lp = _lognorm(x, mu, s)
        phi = _lognorm(xp[:, :, None, :], _mlp(p["f"], x), p["sig_f"]) if t < T - 1 else torch.zeros_like(q_lp)
        gm = _mlp(p["g"], x)
        if poisson:
            gm = torch.nn.functional.softplus(gm) + 1e-6
        g_lp = _lognorm(obs[t][:, None, None, :], gm, p["sig_g"])
        if t > 0:
            Fj = Fm[t - 1].permute(0, 2, 1)                             # (B, N, Dx)
            Wn = logW[t - 1] - lse[t - 1][:, None]
            pair = _lognorm(x[:, :, :, None, :], Fj[:, None, None, :, :], p["sig_f"]) + Wn[:, None, None, :]
            lam = torch.logsumexp(pair, -1)
        else:
            lam = _lognorm(x, p["imean"][:, None, None, :], p["isig"])
        om_raw = lam + phi + g_lp - q_lp                                # (B, N, M)
        omega = om_raw - torch.logsumexp(om_raw, -1, keepdim=True)
        w = torch.exp(om_raw - om_raw.max(-1, keepdim=True).values).detach()
        cdf = torch.cumsum(w, -1)
        sel = (cdf <= u_b[t][:, :, None] * cdf[..., -1:]).sum(-1).clamp(max=M - 1)
        pick = lambda v: v.gather(2, sel[:, :, None]).squeeze(2)
        xs = x.gather(2, sel[:, :, None, None].expand(B, N, 1, Dx)).squeeze(2)
        Om = pick(omega) + pick(q_lp) + math.log(M)
        out["bwX"][t], out["glp"][t], out["Omega"][t], out["sel"][t] = xs.permute(0, 2, 1), pick(g_lp), Om, sel
        if t < T - 1:
            out["flp"][t + 1] = pick(phi)
        if t == 0:
            out["flp"][0] = pick(lam)
        score = score + pick(g_lp) - Om + (pick(phi) if t < T - 1 else 0.0) + (pick(lam) if t == 0 else 0.0)
        xp = xs
    res = {k: torch.stack(v) for k, v in out.items()}
    res["score"] = score
    return res


ENTRY_SHAPES = [(Dx, M, (3, 17, 32)[(i + j) % 3], (16, 32, 64)[(i + 2 * j) % 3])
                for i, Dx in enumerate((2, 3, 4)) for j, M in enumerate((4, 8, 16, 32))]


@pytest.mark.parametrize("Dx,M,Dy,H", ENTRY_SHAPES, ids=lambda v: str(v))
def test_entry_points_alone(built_lib, Dx, M, Dy, H):
    """ops.bsim_forward_wobs / ops.bsim_backward_wobs on random filter outputs: B 2, T 4, N 20 (no multiple of the chains per
    workgroup; two workgroups per sequence at M = 32), Poisson emission on every third shape"""
    from psvo_amd import ops
    B, T, N = 2, 4, 20
    poisson = (Dx + M) % 3 == 0
    g = torch.Generator().manual_seed(1000 * Dx + 10 * M + Dy)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    mlp = lambda i, o: [rn(i, H) / i ** 0.5, 0.3 * rn(H), rn(H, o) / H ** 0.5, 0.3 * rn(o)]
    sig = lambda n: 0.5 + torch.rand(n, generator=g, dtype=torch.float64)
    logW = rn(T, B, N)
    p = {"Fm": rn(T, B, Dx, N), "logW": logW, "lse": torch.logsumexp(logW, -1) + 0.1 * rn(T, B),
         "f": mlp(Dx, Dx), "g": mlp(Dx, Dy), "q1_inv": mlp(Dx, Dx),
         "sig_f": sig(Dx), "sig_g": torch.ones(Dy, dtype=torch.float64) if poisson else sig(Dy), "sig_q1inv": sig(Dx),
         "sig_bq2": sig(Dx), "bmu2": rn(T, B, Dx), "minit": rn(B, Dx), "sig_init": sig(Dx), "imean": rn(B, Dx), "isig": sig(Dx),
         "obs": 1.5 * rn(T, B, Dy), "eps_b": rn(T, B, Dx, N, M)}
    u_b = torch.rand(T, B, N, generator=g, dtype=torch.float64)
    dscore = rn(B, N)
    leaves = {}
    for k, v in p.items():
        if k in ("obs", "eps_b") or (poisson and k == "sig_g"):
            continue
        if isinstance(v, list):
            for i, t in enumerate(v):
                leaves["%s.%d" % (k, i)] = t.requires_grad_(True)
        else:
            leaves[k] = v.requires_grad_(True)
    ref = _bsim_restated(p, u_b, poisson)
    grads = dict(zip(leaves, torch.autograd.grad((dscore * ref["score"]).sum(), list(leaves.values()))))

    dev = lambda t: t.detach().float().cuda().contiguous()
    desc = ops.make_desc(B, T, N, M, Dx, Dy, H, emission=int(poisson))
    w = {k: tuple(dev(t) for t in p[k]) for k in ("f", "g", "q1_inv")}
    filt = {k: dev(p[k]) for k in ("Fm", "logW", "lse")}
    filt["X"] = filt["Fm"]
    args = (desc, filt, w["f"], w["g"], w["q1_inv"]) + tuple(
        dev(p[k]) for k in ("sig_f", "sig_g", "sig_q1inv", "sig_bq2", "bmu2", "minit", "sig_init", "imean", "isig", "obs", "eps_b"))
    bs = ops.bsim_forward_wobs(*args, u_b=dev(u_b), save=True)
    r = ops.bsim_backward_wobs(*args, bs, dev(dscore))
    ops.sum_chain_rows(r, T, B, Dx)
    torch.cuda.synchronize()
    assert torch.equal(bs["sel"].cpu().long(), ref["sel"]), "a sub-particle pick differs from the contract's"
    for k, tol in (("bwX", 2e-4), ("flp", 5e-4), ("glp", 5e-4), ("Omega", 5e-4), ("score", 2e-3)):
        e = float((bs[k].double().cpu() - ref[k].detach()).abs().max())
        print("%s max abs err %.3e" % (k, e))
        assert e <= tol + 1e-5 * float(ref[k].detach().abs().max()), k
    got = {"Fm": r["dFm"], "logW": r["dlogW"], "lse": r["dlse"], "sig_f": r["dsig_f"], "sig_g": r["dsig_g"],
           "sig_q1inv": r["dsig_q1inv"], "sig_bq2": r["dsig_bq2"], "bmu2": r["dbmu2"], "minit": r["dminit"],
           "sig_init": r["dsig_init"], "imean": r["dimean"], "isig": r["disig"]}
    for k, key in (("f", "gf"), ("g", "gg"), ("q1_inv", "gq1inv")):
        Dout = Dy if k == "g" else Dx
        for i, t in enumerate(ops.split_mlp_grad(r[key], Dx, H, Dout)):
            got["%s.%d" % (k, i)] = t
    assert set(got) >= set(grads)
    # d lse is a difference of sums that cancel (psvo_hip.h): it is held to the scale of d logW, whose row sum it negates
    scale_of = lambda k: float(grads["logW" if k == "lse" else k].abs().max())
    for k, ref_g in grads.items():
        e = float((got[k].double().cpu() - ref_g).abs().max())
        print("d %s: max abs err %.3e of largest entry %.3e" % (k, e, scale_of(k)))
        assert e <= 2e-3 * scale_of(k) + 1e-6, k


# ---- the wide reverse filter with upstream gradients of Fm / logW -----------------------------------------------------------
def _filter_of(case, extra, seed):
    """case's wide filter run under autograd: (model, FLAGS, obs, noise, teacher, the filter's output dict, its autograd node)"""
    FLAGS, model, smc, obs, noise = _wide(case, extra, seed)
    _, ref0 = Hh.run_oracle(model, FLAGS, case[0], obs, noise)
    teacher = {"idx_f": ref0["idx_f"]}
    nz = Hh.noise_to_hip({**noise, **teacher}, "cuda")
    nz.pop("u_f", None)
    B, T = case[1], case[2]
    smc.Dx, smc.batch_size, smc.time = model.Dx, B, T
    smc._release()
    smc._sigmas = model.sigmas()
    filt = smc.SMC(None, obs.float().cuda(), noise=nz)
    return model, FLAGS, obs, noise, teacher, filt, filt["Fm"].grad_fn


def test_filter_backward_wobs_ext(built_lib):
    """NULL external gradients: the outputs of psvo_filter_backward_wobs bit for bit.  Random ones, nparts 1 (through autograd)
    against fp64 autograd of the oracle's filter under the surrogate loss sum dFm Fm + sum dlogW logW + sum dlse lse, and
    nparts 3 against the same oracle gradients (the three parts sum to the gradients of the nparts 1 run)"""
    from oracle import psvo_oracle as O
    from psvo_amd import ops
    case, extra = CASES[1]
    obj, B, T, N, M, Dx = case[:6]
    model, FLAGS, obs, noise, teacher, filt, node = _filter_of(case, extra, 5)
    q1, f, g, rest, obs_TB, eps = node.saved
    g_ = torch.Generator().manual_seed(11)
    dlse, dlogW, dFm = (torch.randn(*s, generator=g_).cuda() for s in ((T, B), (T, B, N), (T, B, Dx, N)))
    call = lambda **kw: ops.filter_backward(node.desc, q1, f, g, *rest, obs_TB, eps, node.filt, wobs=True, **kw)
    keys = ("dP", "dF", "dG", "dmu2", "dm0", "dfm0", "dsig_q1", "dsig_q2", "dsig_f", "dsig_g", "dsig0", "dfsig0", "gq1", "gf", "gg")
    plain, ext = call(dlse=dlse), call(dlse=dlse, ext=True)
    torch.cuda.synchronize()
    for k in keys:
        assert (plain[k] is None and ext[k] is None) or torch.equal(plain[k], ext[k]), k
    # nparts = 3: three random parts whose sums are dFm / dlogW, so that the oracle gradients below are the reference of both
    pF, pW = torch.randn(T, B, 3, Dx, N, generator=g_).cuda(), torch.randn(T, B, 3, N, generator=g_).cuda()
    pF[:, :, 2] = dFm - pF[:, :, 0] - pF[:, :, 1]
    pW[:, :, 2] = dlogW - pW[:, :, 0] - pW[:, :, 1]
    three = call(dlse=dlse, dFm=pF.contiguous(), dlogW=pW.contiguous(), nparts=3)
    one = call(dlse=dlse, dFm=dFm, dlogW=dlogW)
    torch.cuda.synchronize()
    for k in keys:      # (the parts sum to the single part up to fp32 rounding of the three-term sums)
        if one[k] is not None:
            assert torch.allclose(three[k], one[k], rtol=1e-4, atol=1e-4 * float(one[k].abs().max()) + 1e-7), k
    # nparts = 1 through the autograd node, against the oracle
    model.zero_grad()
    ((dFm * filt["Fm"]).sum() + (dlogW * filt["logW"]).sum() + (dlse * filt["lse"]).sum()).backward()
    torch.cuda.synchronize()
    P = model.export_reference_layout(torch.float64)
    leaves = []

    def req(x):
        if torch.is_tensor(x):
            leaves.append(x.requires_grad_(True))
        elif isinstance(x, dict):
            [req(v) for v in x.values()]
        elif isinstance(x, (list, tuple)):
            [req(v) for v in x]
    req(P)
    o = O.OBJECTIVES[obj](P, Hh.oracle_flags(FLAGS, obj))
    Xs, _, log_Ws = o.SMC(obs, {**noise, **teacher})                   # (T, N, B, Dx), (T, N, B)
    Fm_ref = o.f.mean(Xs)
    to_ref = lambda t: t.double().cpu()
    (((to_ref(dFm).permute(0, 3, 1, 2)) * Fm_ref).sum() + (to_ref(dlogW).permute(0, 2, 1) * log_Ws).sum()
     + (to_ref(dlse) * torch.logsumexp(log_Ws, 1)).sum()).backward()

    def against_oracle(what, grad_of):
        bad = []
        for name, p, ref in _pairs(model, P):
            got = grad_of(name, p)
            if ref.grad is None and got is None:
                continue
            gg = torch.zeros_like(ref) if got is None else got.detach().double().cpu().reshape(ref.shape)
            r = torch.zeros_like(ref) if ref.grad is None else ref.grad
            e, s = float((gg - r).abs().max()), max(float(r.abs().max()), 1e-6)
            print("%s %s: max abs err %.3e of largest entry %.3e" % (what, name, e, s))
            if e > 2e-3 * s + 1e-6:
                bad.append((name, e, s))
        assert not bad, (what, bad)
    against_oracle("nparts=1", lambda name, p: p.grad)
    # nparts = 3 against the same oracle gradients, for what the kernel call returns whole: the weight gradients of MLP_q1 and
    # MLP_g, which only the particles evaluate (MLP_f also runs hoisted on the X0 feature, so its total is autograd's)
    H_, Dy_ = node.desc.H, node.desc.Dy
    direct = {}
    for key, net, Dout in (("gq1", "q1", Dx), ("gg", "g", Dy_)):
        W1, b1, W2, b2 = ops.split_mlp_grad(three[key], Dx, H_, Dout)
        direct.update({net + ".W0": W1, net + ".b0": b1, net + ".Wmu": W2, net + ".bmu": b2})
    checked = []

    def grad3(name, p):
        if name in direct:
            checked.append(name)
            return direct[name]
        return p.grad           # (not returned by the kernel call itself: compared as above)
    against_oracle("nparts=3", grad3)
    assert sorted(checked) == sorted(direct) and len(direct) == 8


# ---- the training step ---------------------------------------------------------------------------------------------------
def test_step_replays_from_hipgraph(built_lib):
    """one local training step at the Lorenz-width case, eager and captured into a GraphedStep: a replay equals the eager step
    bit for bit (the wide kernels sum in fixed orders), and rewrites every gradient itself"""
    from psvo_amd.graph import GraphedStep
    from psvo_amd.optim import FlatParams
    case, extra = CASES[1]
    FLAGS, model, smc, obs, noise = _wide(case, extra, 3)
    nz = Hh.noise_to_hip(noise, "cuda")
    flat = FlatParams(model)
    obs_c = obs.float().cuda()

    def local():
        flat.zero_grad()
        z, _ = smc.get_log_ZSMC(obs_c, None, noise=nz)
        z.backward()
        return z.detach()
    z_e = local().clone()
    g_e = flat.grad.clone()
    torch.cuda.synchronize()
    assert torch.isfinite(z_e) and torch.isfinite(g_e).all() and float(g_e.abs().max()) > 0
    step = GraphedStep(local)
    for _ in range(2):
        flat.grad.fill_(float("nan"))
        z_g = step()
        torch.cuda.synchronize()
        assert torch.equal(z_g, z_e)
        assert torch.equal(flat.grad, g_e)


def _trajectories(work):
    """shapes of the trajectories the trainer saved (trajectory_<epoch>.p: {"Xs": ...})"""
    import glob
    import pickle
    shapes = []
    for path in glob.glob(str(work / "rslts" / "**" / "trajectory_*.p"), recursive=True):
        with open(path, "rb") as fh:
            shapes.append(np.asarray(pickle.load(fh)["Xs"]).shape)
    assert shapes, "no trajectory file was written"
    return shapes


def test_runner_on_the_lorenz_slice(built_lib, tmp_path, monkeypatch):
    d = np.load(os.path.join(GOLDEN, "lorenz_slice.npz"))
    data = {"Ytrain": d["Ytrain"], "Yvalid": d["Yvalid"]}
    FLAGS, hist, work = _run_main(tmp_path, monkeypatch, "lorenz", data,
                                  ["--PSVO", "--BSim_wide_obs", "--n_particles=16", "--n_particles_for_BSim_proposal=4",
                                   "--batch_size=4"], 3, 10)
    assert FLAGS.PSVO and FLAGS.BSim_wide_obs and (FLAGS.n_train, FLAGS.n_test, FLAGS.time) == (8, 4, 100)
    for s in _trajectories(work):
        assert s[-3:] == (100, 16, 3), s


def test_runner_on_the_vind_slice(built_lib, tmp_path, monkeypatch):
    d = np.load(os.path.join(GOLDEN, "vind_slice.npz"))
    data = {"Ytrain": d["Ytrain"], "Yvalid": d["Yvalid"], "Xtrain": d["Xtrain"], "Xtest": d["Xvalid"]}
    FLAGS, hist, work = _run_main(tmp_path, monkeypatch, "vind", data,
                                  ["--PSVO", "--BSim_wide_obs", "--n_particles=16", "--n_particles_for_BSim_proposal=8",
                                   "--batch_size=4"], 2, 20)
    assert FLAGS.PSVO and FLAGS.BSim_wide_obs and (FLAGS.n_train, FLAGS.n_test, FLAGS.time) == (8, 4, 30)
    for s in _trajectories(work):
        assert s[-3:] == (30, 16, 2), s


# ---- what stays refused ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,extra,word", [
    (("PSVO", 2, 5, 16, 4, 2, 3, 32, True, True), {}, r"Dy = 3 with PSVO / PSVOwR.*Dy <= 2"),
    (("PSVOwR", 2, 5, 16, 4, 2, 3, 32, True, True), {}, r"Dy = 3 with PSVO / PSVOwR.*Dy <= 2"),
    (("PSVOwR", 2, 5, 16, 4, 2, 3, 32, True, True), WIDE, "PSVOwR"),
    (("PSVO", 2, 5, 16, 4, 2, 3, 32, True, True), dict(output_cov=True, diag_cov=True, **WIDE), "output_cov"),
    (("PSVO", 2, 5, 16, 4, 2, 3, 32, True, True), dict(q1_layers="32,32", g_layers="32,32", **WIDE), "one hidden layer"),
    (("PSVO", 2, 5, 16, 4, 2, 33, 32, True, True), WIDE, r"Dy = 33.*3 <= Dy <= 32"),
    (("PSVO", 2, 5, 16, 4, 2, 33, 32, True, True), dict(output_cov=True, diag_cov=True, **WIDE), r"Dy = 33.*3 <= Dy <= 32"),
], ids=["PSVO", "PSVOwR", "PSVOwR-flag", "output_cov", "two-layers", "Dy33", "Dy33-first"])
def test_refusals(built_lib, case, extra, word):
    with pytest.raises(ValueError, match=word):
        _setup(*case, **extra)


def test_flag_without_effect(built_lib):
    """the flag with Dy <= 2, or with a filter objective, changes nothing"""
    for case in (("PSVO", 2, 5, 16, 4, 2, 2, 32, True, True), ("AESMC", 2, 5, 16, 1, 2, 3, 32, True, True)):
        res = []
        for extra in ({}, WIDE):
            FLAGS, model, smc, obs, noise = _setup(*case, seed=3, **extra)
            with torch.no_grad():
                z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=Hh.noise_to_hip(noise, "cuda"))
            res.append((smc.wide_obs, z.clone()))
        assert res[0][0] == res[1][0] == (case[6] > 2) and torch.equal(res[0][1], res[1][1])


def test_plain_entry_points_still_refuse_wide_observations(built_lib):
    """psvo_bsim_forward keeps answering PSVO_ERR_UNSUPPORTED for Dy = 3 (nothing is launched)"""
    from psvo_amd import ops
    B, T, N, M, Dx, Dy, H = 1, 3, 8, 4, 2, 3, 16
    z = lambda *s: torch.zeros(*s, device="cuda")
    mlp = lambda o: (z(Dx, H), z(H), z(H, o), z(o))
    filt = {"X": z(T, B, Dx, N), "Fm": z(T, B, Dx, N), "logW": z(T, B, N), "lse": z(T, B)}
    one = lambda n: torch.ones(n, device="cuda")
    with pytest.raises(ValueError, match=r"psvo_bsim_forward failed: unsupported"):
        ops.bsim_forward(ops.make_desc(B, T, N, M, Dx, Dy, H), filt, mlp(Dx), mlp(Dy), mlp(Dx), one(Dx), one(Dy), one(Dx),
                         one(Dx), z(T, B, Dx), z(B, Dx), one(Dx), z(B, Dx), one(Dx), z(T, B, Dy), z(T, B, Dx, N, M),
                         u_b=z(T, B, N))
