"""The particle forecast (psvo_particle_forecast, --particle_forecast) on the GPU: the kernel directly on synthetic systems, through
the objectives, beside training, and through runner.main.

Direct launches use the systems of tests/forecast_reference.cases(): the smallest shapes at which the kernel can still go wrong
(sub-wave N, K > T, three waves with T = 1, the count emission at N = 512, N = 1 with K = 0 and Dy = 32, particles of weight zero,
noise-free propagation).  Every output is judged against the fp64 restatement (tests/forecast_reference.py) by the project's rule,
with the yardstick err_32 = what the same restatement costs in fp32 on the CPU:
    err_hip <= K_TOL[output] err_32 + 8 2^-24 max|ref_64|.
K_TOL is twice the worst ratio err_hip / err_32 measured on these cases, rounded up to a power of two
(profiles/particle_forecast.md records the ratios).  Figures are printed before every assertion (pytest -s shows them).
"""
import glob
import pickle

import pytest
import torch

from tests import forecast_reference as R
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

# worst ratios measured on the direct launches: ymean 1.71, yvar 1.89, xmean 1.00, lpd 3.36 (N = 1, Dy = 32: 32 squared residuals
# summed in a different order than torch sums them; every other case stays below 1.9)
K_TOL = {"ymean": 4, "yvar": 4, "xmean": 2, "lpd": 8}
ULP = 2.0 ** -24
CASES = R.cases()
_params = pytest.mark.parametrize("shape,weights,noisy", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
_ids = lambda s: "-".join(map(str, s))


def _cuda(v):
    return None if v is None else tuple(_cuda(u) for u in v) if isinstance(v, tuple) else v.cuda()


def _launch(shape, c, **over):
    from psvo_amd import ops
    T, B, Dx, Dy, H, N, K, emission = shape
    desc = ops.make_desc(B, T, N, 1, Dx, Dy, H, emission=emission)
    a = {k: _cuda(c[k]) for k in ("f", "g", "sig_f", "sig_g", "X", "logW", "obs", "eps")}
    a.update(over)
    out = ops.particle_forecast(desc, K, a["f"], a["g"], a["sig_f"], a["sig_g"], a["X"], logW=a["logW"], obs=a["obs"], eps=a["eps"])
    torch.cuda.synchronize()
    assert set(out) == set(R.KEYS)
    assert out["ymean"].shape == (K + 1, T, B, Dy) and out["yvar"].shape == (K + 1, T, B, Dy)
    assert out["xmean"].shape == (K + 1, T, B, Dx) and (out["lpd"] is None or out["lpd"].shape == (K + 1, T, B))
    return out


def _judge(tag, out, c, keys=R.KEYS):
    """the project's rule for every output, figures first"""
    ref64, ref32, valid = c["ref64"], c["ref32"], c["valid"]
    cpu = {k: out[k].cpu() for k in keys}
    lines, bad = [], []
    for k in keys:
        assert torch.isfinite(cpu[k]).all(), k
        err_hip, biggest = R.error(cpu, ref64, k, valid)
        err_32, _ = R.error(ref32, ref64, k, valid)
        floor = 8 * ULP * biggest
        lines.append("forecast-yardstick %s %s err_hip %.3e err_32 %.3e ratio %.3f floor %.3e"
                     % (tag, k, err_hip, err_32, err_hip / err_32 if err_32 > 0 else float("inf"), floor))
        if not err_hip <= K_TOL[k] * err_32 + floor:
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, bad


@_params
def test_direct_launch(built_lib, shape, weights, noisy):
    T, B, Dx, Dy, H, N, K, emission = shape
    c = R.case(shape, weights, noisy)
    out = _launch(shape, c)
    assert (out["lpd"].cpu()[~c["valid"]] == 0).all()          # exactly 0 where t + k >= T
    assert (out["yvar"] > 0).all()
    _judge(_ids(shape) + "-" + weights + ("" if noisy else "-noisefree"), out, c)
    # without observations: no log-density, the moments unchanged bit for bit
    bare = _launch(shape, c, obs=None)
    assert bare["lpd"] is None
    for k in ("ymean", "yvar", "xmean"):
        assert torch.equal(bare[k], out[k]), k


@_params
def test_two_launches_are_bit_identical(built_lib, shape, weights, noisy):
    from psvo_amd import _lib
    c = R.case(shape, weights, noisy)
    a, b = _launch(shape, c), _launch(shape, c)
    with Hh.tuning(_lib.PSVO_TUNE_DETERMINISTIC, 1):
        d1, d2 = _launch(shape, c), _launch(shape, c)
    for k in R.KEYS:
        assert torch.equal(a[k], b[k]) and torch.equal(d1[k], d2[k]) and torch.equal(a[k], d1[k]), k


@pytest.mark.parametrize("shape,weights,noisy", [c[1:] for c in CASES if c[2] == "none"],
                         ids=[c[0] for c in CASES if c[2] == "none"])
def test_equal_log_weights_are_no_weights(built_lib, shape, weights, noisy):
    """equal-valued finite logW: the outputs of logW = NULL, to the same tolerance"""
    T, B, N = shape[0], shape[1], shape[5]
    c = R.case(shape, weights, noisy)
    out = _launch(shape, c, logW=torch.full((T, B, N), -2.5, device="cuda"))
    _judge(_ids(shape) + "-equal-logW", out, c)


def test_op_refuses_bad_arguments(built_lib):
    from psvo_amd import ops
    shape = (3, 2, 2, 1, 16, 8, 2, 0)
    T, B, Dx, Dy, H, N, K, _ = shape
    c = {k: _cuda(v) if k in ("f", "g", "sig_f", "sig_g", "X", "logW", "obs", "eps") else v for k, v in R.system(*shape).items()}
    desc = ops.make_desc(B, T, N, 1, Dx, Dy, H)
    call = lambda **kw: ops.particle_forecast(desc, kw.pop("K", K), *[kw.pop(k, c[k]) for k in ("f", "g", "sig_f", "sig_g", "X")],
                                              **{**dict(obs=c["obs"], eps=c["eps"]), **kw})
    with pytest.raises(ValueError, match="X must have shape"):
        call(X=c["X"][:, :, :, :4].contiguous())
    with pytest.raises(ValueError, match="eps must have shape"):
        call(K=K + 1)
    with pytest.raises(ValueError, match="logW must have shape"):
        call(logW=torch.zeros(T, B, N + 1, device="cuda"))
    with pytest.raises(ValueError, match="obs must have shape"):
        call(obs=torch.zeros(T, B, Dy + 1, device="cuda"))
    with pytest.raises(ValueError, match="K >= 0"):
        call(K=-1, eps=None)
    with pytest.raises(ValueError, match="needs the transition scale"):
        call(sig_f=None)
    with pytest.raises(ValueError, match="count emission only"):
        call(sig_g=None)
    with pytest.raises(ValueError, match="g.W2 must have shape"):
        call(g=c["f"])
    with pytest.raises(ValueError, match="unsupported"):
        ops.particle_forecast(ops.make_desc(B, T, 600, 1, Dx, Dy, H), 0, c["f"], c["g"], c["sig_f"], c["sig_g"],
                              torch.zeros(T, B, Dx, 600, device="cuda"))
    with pytest.raises(ValueError, match="unsupported"):
        ops.particle_forecast(ops.make_desc(B, T, N, 1, Dx, Dy, H, layers=2), 0, c["f"], c["g"], c["sig_f"], c["sig_g"], c["X"])


# ---- through the model ---------------------------------------------------------------------------------------------------
def _setup(obj, B, T, N, M, Dx, Dy, H, bootstrap, two_q, seed=0, **extra):
    """a perturbed model, its objective and observations (counts under --count_emission)"""
    from psvo_amd.model import SSM
    from psvo_amd.SMC.AESMC import AESMC
    from psvo_amd.SMC.PSVO import PSVO
    from psvo_amd.SMC.SVO import SVO
    cls = {"SVO": SVO, "PSVO": PSVO, "AESMC": AESMC}[obj]
    hs = str(H)
    kw = dict(Dx=Dx, Dy=Dy, n_particles=N, n_particles_for_BSim_proposal=M, batch_size=B, time=T,
              q0_layers=hs, q1_layers=hs, q2_layers=hs, f_layers=hs, g_layers=hs,
              y_smoother_Dhs="8", X0_smoother_Dhs="8", use_bootstrap=bootstrap, use_2_q=two_q)
    kw.update(extra)
    FLAGS = Hh.make_flags(obj, **kw)
    torch.manual_seed(seed)
    model = Hh.perturb_(SSM(FLAGS)).cuda()
    g = torch.Generator().manual_seed(100 + seed)
    if extra.get("count_emission"):
        obs = torch.poisson(torch.full((B, T, Dy), 2.0), generator=g)
    else:
        obs = (torch.randn(B, T, Dy, generator=g, dtype=torch.float64) * 1.5).float()
    smc = cls(model, FLAGS)
    smc.generator = torch.Generator(device="cuda").manual_seed(7 + seed)
    return FLAGS, model, smc, obs.cuda()


def _model_case(smc, model, hidden, obs, K, eps):
    """the restatement's inputs for the cloud `hidden` (B,T,N,Dx) of an evaluation, and both references"""
    cpu = lambda v: tuple(cpu(u) for u in v) if isinstance(v, tuple) else v.detach().float().cpu().contiguous()
    f_tran, f_dist = (model.q1_tran, smc.q1) if model.use_bootstrap else (model.f_tran, smc.f)
    emission = 2 if getattr(model, "count_emission", False) else int(model.poisson_emission)
    c = dict(f=cpu(tuple(smc._mlp_params(f_tran))), g=cpu(tuple(smc._mlp_params(model.g_tran))), sig_f=cpu(f_dist.get_sigma()),
             sig_g=cpu(smc.g.get_sigma()), X=cpu(hidden.permute(1, 0, 3, 2)), logW=None, obs=cpu(obs.transpose(0, 1)),
             eps=None if eps is None else cpu(eps), K=K, emission=emission)
    c["ref64"], c["ref32"] = R.run(c, torch.float64), R.run(c, torch.float32)
    c["valid"] = R.valid_mask(hidden.shape[1], K)
    return c


def _kernel_layout(fc):
    return {"ymean": fc["y_mean"].permute(2, 1, 0, 3), "yvar": fc["y_var"].permute(2, 1, 0, 3),
            "xmean": fc["x_mean"].permute(2, 1, 0, 3), "lpd": fc["lpd"].permute(2, 1, 0)}


OBJECTIVES = [
    (("AESMC", 4, 12, 16, 1, 2, 1, 16, True, True), {}),
    (("SVO", 4, 12, 16, 1, 2, 2, 32, False, False), dict(FFBSi=True)),                      # whole paths; f has its own network
    (("PSVO", 4, 12, 16, 4, 2, 1, 32, True, True), {}),
    (("AESMC", 4, 12, 16, 1, 3, 10, 32, True, True), dict(count_emission=True)),            # wide observations, counts
]


@pytest.mark.parametrize("case,extra", OBJECTIVES, ids=lambda v: _ids(v) if isinstance(v, tuple) else ",".join(sorted(v)) or "plain")
def test_through_the_objectives(built_lib, case, extra):
    """smc.particle_forecast on the evaluation's own log["Xs"] is the restatement applied to the same cloud and the same eps_p"""
    obj, B, T, N, M, Dx, Dy = case[:7]
    K = 4
    FLAGS, model, smc, obs = _setup(*case, particle_forecast=True, **extra)
    assert smc.forecast is True
    eps = torch.randn(K, T, B, Dx, N, generator=torch.Generator().manual_seed(21)).cuda()
    with torch.no_grad():
        _, log = smc.get_log_ZSMC(obs, None)
        Xs = log["Xs"]
        fc = smc.particle_forecast(K, Xs, obs, noise={"eps_p": eps})
    torch.cuda.synchronize()
    assert Xs.shape == (B, T, N, Dx) and Xs.permute(1, 0, 3, 2).is_contiguous()      # (a view of a kernel-layout tensor)
    assert fc["y_mean"].shape == (B, T, K + 1, Dy) and fc["y_var"].shape == (B, T, K + 1, Dy)
    assert fc["x_mean"].shape == (B, T, K + 1, Dx) and fc["lpd"].shape == (B, T, K + 1)
    assert torch.equal(fc["valid"].cpu(), R.valid_mask(T, K).t())
    assert (fc["lpd"].permute(1, 2, 0)[~fc["valid"]] == 0).all()
    c = _model_case(smc, model, Xs, obs, K, eps)
    _judge(_ids(case), _kernel_layout(fc), c)
    # the objective's own draws: reproducible from its generator, different from the injected ones; none when switched off
    with torch.no_grad():
        smc.generator.manual_seed(5)
        a = smc.particle_forecast(K, Xs, obs)
        smc.generator.manual_seed(5)
        b = smc.particle_forecast(K, Xs, obs)
        smc.forecast_noise = False
        quiet = smc.particle_forecast(K, Xs, obs)
    assert torch.equal(a["y_mean"], b["y_mean"]) and torch.equal(a["lpd"], b["lpd"])
    assert not torch.equal(a["y_mean"][:, :, 1:], fc["y_mean"][:, :, 1:]) and torch.equal(a["y_mean"][:, :, 0], fc["y_mean"][:, :, 0])
    c0 = _model_case(smc, model, Xs, obs, K, None)
    _judge(_ids(case) + "-noisefree", _kernel_layout(quiet), c0)


def test_degenerate_cloud_is_the_point_forecast(built_lib):
    """N copies of one point, no transition noise, Gaussian emission: y_mean is n_step_prediction on that point (the bound
    tests/test_gpu_prediction.py uses for this arithmetic), y_var is sig_g^2 (N = 16: the weights 1 / 16 scale exactly and the
    wave sum of 16 equal terms is exact, so the spread of the cloud is exactly zero), lpd is the log-density of the single point"""
    case = ("AESMC", 3, 10, 16, 1, 3, 2, 32, True, True)
    obj, B, T, N, M, Dx, Dy = case[:7]
    K = 5
    FLAGS, model, smc, obs = _setup(*case, particle_forecast=True, forecast_noise=False)
    point = torch.randn(B, T, 1, Dx, generator=torch.Generator().manual_seed(13)).cuda() * 1.5
    hidden = point.expand(B, T, N, Dx)
    with torch.no_grad():
        fc = smc.particle_forecast(K, hidden, obs)
        y_hat, y = smc.n_step_prediction(K, hidden, obs)
        sig_g = smc.g.get_sigma().float()
    torch.cuda.synchronize()
    for k in range(K + 1):
        assert torch.allclose(fc["y_mean"][:, :T - k, k], y_hat[k], atol=2e-4, rtol=1e-5), k
    rel = ((fc["y_var"] - sig_g ** 2).abs() / sig_g ** 2).max()
    print("forecast-degenerate worst relative deviation of y_var from sig_g^2: %.3e" % float(rel))
    assert float(rel) <= 1e-6
    # the single point in the restatement (N = 1): the cloud's log-density is the point's
    c = _model_case(smc, model, point, obs, K, None)
    _judge("degenerate", _kernel_layout(fc), c)
    mu = fc["y_mean"].double().cpu()
    for k in range(K + 1):
        lp = R.log_g(obs[:, k:].double().cpu(), mu[:, :T - k, k], sig_g.double().cpu(), 0)
        err = float((fc["lpd"][:, :T - k, k].double().cpu() - lp).abs().max())
        assert err <= 8 * 8 * ULP * max(1.0, float(lp.abs().max())), (k, err)


def test_training_is_unaffected(built_lib, monkeypatch):
    """under autograd the kernel is never launched; ELBO and every parameter gradient are bit-identical with and without the flag"""
    from psvo_amd import ops
    case = ("AESMC", 2, 6, 16, 1, 2, 1, 32, True, True)
    FLAGS, model, smc, obs = _setup(*case, particle_forecast=True)
    noise = {"eps_f": torch.randn(6, 2, 2, 16, generator=torch.Generator().manual_seed(3)).cuda(),
             "u_f": torch.rand(6, 2, 16, generator=torch.Generator().manual_seed(4)).cuda()}

    def refuse(*a, **k):
        raise AssertionError("ops.particle_forecast was called under autograd")
    monkeypatch.setattr(ops, "particle_forecast", refuse)
    res = []
    for on in (True, False):
        smc = type(smc)(model, Hh.make_flags("AESMC", **{**FLAGS.as_dict(), "particle_forecast": on}))
        assert smc.forecast is on
        model.zero_grad(set_to_none=True)
        z, log = smc.get_log_ZSMC(obs, None, noise=noise)
        z.backward()
        torch.cuda.synchronize()
        res.append((z.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
        with pytest.raises(ValueError, match="no gradient"):
            smc.particle_forecast(2, log["Xs"], obs)
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 4
    for n, g in res[0][1].items():
        assert torch.equal(g, res[1][1][n]), n


def test_runner_end_to_end(built_lib, tmp_path, monkeypatch):
    """runner.main with --AESMC --particle_forecast for 2 epochs: the forecast_* keys are in metric_*.p, one number per horizon
    k = 0 .. MSE_steps; the saved y_hat files carry y_mean and y_var"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    argv = ["--noPSVO", "--AESMC", "--particle_forecast", "--generateTrainingData", "--time=12", "--n_train=4", "--n_test=4",
            "--batch_size=2", "--n_particles=16", "--epoch=2", "--MSE_steps=5"]
    monkeypatch.chdir(tmp_path)
    FLAGS = parse_flags(argv)
    runner.main(FLAGS)
    torch.cuda.synchronize()
    metrics = glob.glob(str(tmp_path / "rslts" / "epoch_data" / "**" / "metric_*.p"), recursive=True)
    assert metrics
    for path in metrics:
        with open(path, "rb") as fh:
            m = pickle.load(fh)
        for split in ("train", "test"):
            for stem in ("forecast_lpd_", "forecast_R_square_", "forecast_calibration_"):
                v = m[stem + split]
                assert v.shape == (6,) and bool((v == v).all()), (stem, split, v)
            assert (m["forecast_calibration_" + split] > 0).all()
    saved = glob.glob(str(tmp_path / "rslts" / "epoch_data" / "**" / "y_hat_*.p"), recursive=True)
    assert saved
    with open(saved[0], "rb") as fh:
        s = pickle.load(fh)
    n = min(FLAGS.saving_num, 4)
    assert s["y_mean"].shape == (n, 12, 6, FLAGS.Dy) and s["y_var"].shape == (n, 12, 6, FLAGS.Dy) and (s["y_var"] > 0).all()
