"""bsim_fwd_kernel (the forward backward simulation) requests the inputs of step t - 1 and the forward tile of step t - 2 at
the top of step t, through bases that move by a constant per step, and waits for them in one place, the rotation that ends
the step.  These cases are the smallest shapes at which a word moved across a wait can be consumed before it has landed, or
a load can read the wrong step:

  T = 2 (only the two peeled steps, and the tile staged in front of the loop), 3 (one ordinary step), 4 (both tile buffers
  restaged inside the loop), 5.  T = 1 is refused by the ABI (tests/test_gpu_bsim_bwd2_prefetch.py pins that);
  N = 3 (a partial tile: the entry index clamps), 16, 17, 128 (several workgroups), and 300, 600 and 800 at M = 4 (the tile's
  entries beyond the first 256 travel through the second, third and fourth register set of a thread).  The filter kernels
  stop at N = 512, so N = 600 and 800 cannot come through a model: those cases call psvo_bsim_forward (with its optional
  saves) and psvo_bsim_backward on random filter outputs and hold values and every gradient to the fp64 restatement of the
  contract in tests/test_gpu_wobs_bsim.py and its autograd, with that test's tolerances;
  M = 4, 8, 16, 32 (chains per wave, and with them the tail of lanes without a chain);
  (Dx, Dy) = (2, 1), (2, 2), (3, 1), (3, 2), and one Dx = 4 shape: the only width whose time loop is not peeled;
  B = 2 everywhere, so the sequence offset is not zero; two shapes with two hidden layers (the l2 build of the same source);
  one shape with B N M = 131072, the smallest the launcher runs with one lane per (chain, m) instead of two half-chains:
  forward values only, so that the fp64 oracle's (M, N, N, B) tile stays small (N = 32).

GRID crosses N and T and walks (Dx, Dy) and M along both, so that each of the sixteen (width, M) pairs occurs once.  Every
case runs teacher-forced (the oracle's indices go in), values and every gradient against the fp64 oracle with the tolerances
of tests/test_gpu_parity.py and tests/test_gpu_large.py.  The free-running arm (uniforms in, the one the benchmark runs) and
the teacher-forced arm read their word through the same base: three shapes run with uniforms, then with the run's own
indices fed back, then with the uniforms again, and every output and gradient must be byte-equal in all three."""
import pytest
import torch

from tests import helpers as Hh
from tests.test_gpu_large import _compare, _hip_noise, _teacher
from tests.test_gpu_parity import _check_grads, _oracle_grads, _setup

pytestmark = pytest.mark.gpu

_NS, _TS = (3, 16, 17, 128), (2, 3, 4, 5)
_WIDTHS = [(2, 1), (2, 2), (3, 1), (3, 2)]
_MS = (4, 8, 16, 32)
_TWO = dict(q1_layers="32,32", g_layers="32,32")
# objective, B, T, N, M, Dx, Dy, H, bootstrap, two_q.  (i + j, 2 i + j) mod 4 is a bijection of the 4 x 4 grid
GRID = [(("PSVO", 2, t, n, _MS[(2 * i + j) % 4]) + _WIDTHS[(i + j) % 4] + (32, True, True), {})
        for i, n in enumerate(_NS) for j, t in enumerate(_TS)]
# more than 256 tile entries: two register sets per thread
GRID += [(("PSVO", 2, 2, 300, 4, 2, 1, 32, True, True), {}), (("PSVO", 2, 4, 300, 4, 3, 2, 32, True, True), {})]
# more than 512 and more than 768: three and four (B, T, N, M, Dx, Dy, H), at the entry points
MANY_SETS = [(2, 3, 600, 4, 2, 2, 32), (2, 2, 600, 4, 3, 1, 32), (2, 3, 800, 4, 2, 1, 32)]
# Dx = 4: the unpeeled time loop
GRID += [(("PSVO", 2, 4, 17, 8, 4, 1, 32, True, True), {})]
# two hidden layers
GRID += [(("PSVO", 2, 3, 17, 4, 2, 1, 32, True, True), _TWO), (("PSVO", 2, 2, 16, 8, 3, 2, 32, True, True), _TWO)]
# B N M = 131072: one lane per (chain, m)
WHOLE_CHAIN = ("PSVO", 128, 3, 32, 32, 2, 1, 32, True, True)
FREE = [("PSVO", 2, 3, 17, 4, 2, 1, 32, True, True), ("PSVO", 2, 5, 128, 16, 3, 2, 32, True, True),
        ("PSVO", 2, 4, 16, 8, 4, 1, 32, True, True)]


def _id(p):
    case, extra = p
    return "-".join(map(str, case)) + ("-2L" if extra else "")


def _pass(model, smc, obs, nz):
    model.zero_grad()
    z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
    z.backward()
    torch.cuda.synchronize()
    return z.detach(), log


@pytest.mark.parametrize("case,extra", GRID, ids=map(_id, GRID))
def test_prefetch_shapes(built_lib, case, extra):
    obj = case[0]
    FLAGS, model, smc, obs, noise = _setup(*case, seed=47, **extra)
    z_ref, ref = Hh.run_oracle(model, FLAGS, obj, obs, noise)
    teacher = _teacher(ref, obj)
    z, log = _pass(model, smc, obs, _hip_noise(noise, teacher))
    _compare(obj, log, ref, z, z_ref)
    zg, P = _oracle_grads(model, FLAGS, obj, obs, noise, teacher)
    assert abs(float(z) - float(zg)) <= 1e-4 * abs(float(zg))
    _check_grads(model, P)


def test_prefetch_whole_chain_lanes(built_lib):
    """the HS = 1 instantiation, reached by size: forward values against the oracle"""
    obj = WHOLE_CHAIN[0]
    assert WHOLE_CHAIN[1] * WHOLE_CHAIN[3] * WHOLE_CHAIN[4] == 131072
    FLAGS, model, smc, obs, noise = _setup(*WHOLE_CHAIN, seed=49)
    z_ref, ref = Hh.run_oracle(model, FLAGS, obj, obs, noise)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip_noise(noise, _teacher(ref, obj)))
    torch.cuda.synchronize()
    _compare(obj, log, ref, z, z_ref)


@pytest.mark.parametrize("shape", MANY_SETS, ids=lambda c: "-".join(map(str, c)))
def test_prefetch_many_register_sets(built_lib, shape):
    """N = 600 / 800: psvo_bsim_forward with its optional saves on random filter outputs, values against the restated
    contract, then psvo_bsim_backward on those saves, every gradient against autograd of the restatement (the scheme and
    the tolerances of tests/test_gpu_wobs_bsim.py::test_entry_points_alone)"""
    from psvo_amd import ops
    from tests.test_gpu_wobs_bsim import _bsim_restated
    B, T, N, M, Dx, Dy, H = shape
    g = torch.Generator().manual_seed(53 + Dx + N)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    mlp = lambda i, o: [rn(i, H) / i ** 0.5, 0.3 * rn(H), rn(H, o) / H ** 0.5, 0.3 * rn(o)]
    sig = lambda n: 0.5 + torch.rand(n, generator=g, dtype=torch.float64)
    logW = rn(T, B, N)
    p = {"Fm": rn(T, B, Dx, N), "logW": logW, "lse": torch.logsumexp(logW, -1) + 0.1 * rn(T, B),
         "f": mlp(Dx, Dx), "g": mlp(Dx, Dy), "q1_inv": mlp(Dx, Dx),
         "sig_f": sig(Dx), "sig_g": sig(Dy), "sig_q1inv": sig(Dx), "sig_bq2": sig(Dx), "bmu2": rn(T, B, Dx),
         "minit": rn(B, Dx), "sig_init": sig(Dx), "imean": rn(B, Dx), "isig": sig(Dx), "obs": 1.5 * rn(T, B, Dy),
         "eps_b": rn(T, B, Dx, N, M)}
    u_b = torch.rand(T, B, N, generator=g, dtype=torch.float64)
    dscore = rn(B, N)
    leaves = {}
    for k, v in p.items():
        if k in ("obs", "eps_b"):
            continue
        if isinstance(v, list):
            for i, t in enumerate(v):
                leaves["%s.%d" % (k, i)] = t.requires_grad_(True)
        else:
            leaves[k] = v.requires_grad_(True)
    ref = _bsim_restated(p, u_b, False)
    grads = dict(zip(leaves, torch.autograd.grad((dscore * ref["score"]).sum(), list(leaves.values()))))

    dev = lambda t: t.detach().float().cuda().contiguous()
    filt = {k: dev(p[k]) for k in ("Fm", "logW", "lse")}
    filt["X"] = filt["Fm"]
    args = (ops.make_desc(B, T, N, M, Dx, Dy, H), filt) + tuple(tuple(dev(t) for t in p[k]) for k in ("f", "g", "q1_inv")) + tuple(
        dev(p[k]) for k in ("sig_f", "sig_g", "sig_q1inv", "sig_bq2", "bmu2", "minit", "sig_init", "imean", "isig", "obs", "eps_b"))
    bs = ops.bsim_forward(*args, sel_in=ref["sel"].to(torch.int32).cuda().contiguous(), save=True)
    torch.cuda.synchronize()
    assert torch.equal(bs["sel"].cpu().long(), ref["sel"])
    for k, tol in (("bwX", 2e-4), ("flp", 5e-4), ("glp", 5e-4), ("Omega", 5e-4), ("score", 2e-3)):
        e = float((bs[k].double().cpu() - ref[k].detach()).abs().max())
        print("%s max abs err %.3e" % (k, e))
        assert e <= tol + 1e-5 * float(ref[k].detach().abs().max()), k
    r = ops.bsim_backward(*args, bs, dev(dscore))
    ops.sum_chain_rows(r, T, B, Dx)
    torch.cuda.synchronize()
    got = {"Fm": r["dFm"], "logW": r["dlogW"], "lse": r["dlse"], "sig_f": r["dsig_f"], "sig_g": r["dsig_g"],
           "sig_q1inv": r["dsig_q1inv"], "sig_bq2": r["dsig_bq2"], "bmu2": r["dbmu2"], "minit": r["dminit"],
           "sig_init": r["dsig_init"], "imean": r["dimean"], "isig": r["disig"]}
    for k, key in (("f", "gf"), ("g", "gg"), ("q1_inv", "gq1inv")):
        for i, t in enumerate(ops.split_mlp_grad(r[key], Dx, H, Dy if k == "g" else Dx)):
            got["%s.%d" % (k, i)] = t
    assert set(got) >= set(grads)
    # d lse is a difference of sums that cancel (psvo_hip.h): it is held to the scale of d logW, whose row sum it negates
    scale_of = lambda k: float(grads["logW" if k == "lse" else k].abs().max())
    for k, ref_g in grads.items():
        e = float((got[k].double().cpu() - ref_g).abs().max())
        print("d %s: max abs err %.3e of largest entry %.3e" % (k, e, scale_of(k)))
        assert e <= 2e-3 * scale_of(k) + 1e-6, k


def _outputs(model, smc, obs, nz):
    z, log = _pass(model, smc, obs, nz)
    out = {"z": z.cpu().clone(), "Xs": log["Xs"].detach().cpu().clone()}
    for part, keys in (("filter", ("X", "Xanc", "Fm", "logW", "idx", "lse")), ("bsim", ("bwX", "flp", "glp", "Omega", "sel"))):
        out.update({part + "." + k: log[part][k].detach().cpu().clone() for k in keys})
    out.update({"grad." + n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None})
    return out, log["bsim"]["sel"].detach().clone()


def _differing(x, y):
    assert x.keys() == y.keys() and len(x) > 8
    raw = lambda t: t.contiguous().reshape(-1).view(torch.uint8)
    return [k for k in x if x[k].dtype != y[k].dtype or not torch.equal(raw(x[k]), raw(y[k]))]


@pytest.mark.parametrize("case", FREE, ids=lambda c: "-".join(map(str, c)))
def test_prefetch_free_running(built_lib, case):
    """uniforms in; the run's own indices fed back; the uniforms again: one result, byte for byte (a word consumed before
    its load has landed, in either arm, does not repeat)"""
    FLAGS, model, smc, obs, noise = _setup(*case, seed=51)
    nz = Hh.noise_to_hip(noise, "cuda")
    assert "u_b" in nz and "sel_b" not in nz
    free, sel = _outputs(model, smc, obs, nz)
    assert sel.dtype == torch.int32
    fed = {k: v for k, v in nz.items() if k != "u_b"}
    fed["sel_b"] = sel.contiguous()
    forced, _ = _outputs(model, smc, obs, fed)
    again, _ = _outputs(model, smc, obs, nz)
    assert not _differing(free, forced), _differing(free, forced)
    assert not _differing(free, again), _differing(free, again)
