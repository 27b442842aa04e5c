"""The particle forecast under exogenous inputs (psvo_particle_forecast_input; --Di with --particle_forecast
--particle_forecast_inputs) on the GPU: the kernel directly on the cases of tests/exo_forecast_reference.py, through
SVO.particle_forecast, beside training, and through runner.main.

Direct launches: four one-wave origins per workgroup with a dead origin in the last one, K > T (most rows past Tv, both halves of
the row buffer reused), three waves at H = 64 with every future row given, the count emission on eight waves with future inputs
that end part-way, noise-free propagation, and NaN entries in obs.  Every output is judged against the fp64 restatement by the
project's rule with the fp32 restatement on the CPU as the yardstick,
    err_hip <= K_TOL[output] err_32 + 8 2^-24 max|ref_64|,
K_TOL being that of tests/test_gpu_forecast.py as it stands (the arithmetic is the same plus one add per hidden unit and horizon);
tests/test_exo_forecast_host.py asserts, in the reference alone, that zeroing or rolling the rows moves ymean by at least 100 times
the bound on every case.  Figures are printed before every assertion (profiles/exo_forecast.md records the ratios).  The exact
tests compare launches with each other bit for bit."""
import glob
import pickle

import pytest
import torch

from tests import exo_forecast_reference as XR
from tests import forecast_reference as R
from tests import helpers as Hh
from tests.test_gpu_forecast import _cuda, _judge, _kernel_layout, _setup

pytestmark = pytest.mark.gpu

_cases = pytest.mark.parametrize("name", list(XR.CASES))


def _launch(c, hb_f="own", K=None, eps="own", shape=None):
    """the input form on the case's system (hb_f = None: psvo_particle_forecast_missing on the same arguments)"""
    from psvo_amd import ops
    T, B, Dx, Dy, H, N, K0, emission = shape or c["shape"]
    K = K0 if K is None else K
    desc = ops.make_desc(B, T, N, 1, Dx, Dy, H, emission=emission)
    a = {k: _cuda(c[k]) for k in ("f", "g", "sig_f", "sig_g", "X", "logW", "obs", "eps")}
    if not isinstance(eps, str):
        a["eps"] = eps
    rows = c["hb_f"] if isinstance(hb_f, str) else hb_f
    kw = dict(missing=True) if rows is None else dict(hb_f=rows.cuda())
    out = ops.particle_forecast(desc, K, a["f"], a["g"], a["sig_f"], a["sig_g"], a["X"], logW=a["logW"], obs=a["obs"], eps=a["eps"],
                                **kw)
    torch.cuda.synchronize()
    assert set(out) == set(R.KEYS)
    assert out["ymean"].shape == (K + 1, T, B, Dy) and out["yvar"].shape == (K + 1, T, B, Dy)
    assert out["xmean"].shape == (K + 1, T, B, Dx) and out["lpd"].shape == (K + 1, T, B)
    return out


@_cases
def test_direct_launch(built_lib, name):
    c = XR.case(name)
    T, K = c["shape"][0], c["shape"][6]
    out = _launch(c)
    lpd = out["lpd"].cpu()
    assert bool((lpd[~R.valid_mask(T, K)] == 0).all())         # exactly 0 where t + k >= T
    assert bool((lpd[~c["valid"]] == 0).all())                 # ... and on target rows with nothing observed
    assert (out["yvar"] > 0).all()
    _judge("exo-" + name, out, c)


@_cases
def test_zero_rows_are_the_missing_form(built_lib, name):
    """hb_f = 0: psvo_particle_forecast_missing on all four outputs, bit for bit"""
    c = XR.case(name)
    a, b = _launch(c, hb_f=torch.zeros_like(c["hb_f"])), _launch(c, hb_f=None)
    own = _launch(c)
    for k in R.KEYS:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(own["ymean"][1:], b["ymean"][1:]) and torch.equal(own["ymean"][0], b["ymean"][0])


@_cases
def test_no_horizon_no_row(built_lib, name):
    """K = 0: no row is ever used -- an hb_f filled with NaN gives the bits of the missing form"""
    c = XR.case(name)
    a = _launch(c, hb_f=torch.full_like(c["hb_f"], float("nan")), K=0, eps=None)
    b = _launch(c, hb_f=None, K=0, eps=None)
    for k in R.KEYS:
        assert torch.isfinite(a[k]).all() and torch.equal(a[k], b[k]), k


@_cases
def test_two_launches_are_bit_identical(built_lib, name):
    from psvo_amd import _lib
    c = XR.case(name)
    a, b = _launch(c), _launch(c)
    with Hh.tuning(_lib.PSVO_TUNE_DETERMINISTIC, 1):
        d1, d2 = _launch(c), _launch(c)
    for k in R.KEYS:
        assert torch.equal(a[k], b[k]) and torch.equal(d1[k], d2[k]) and torch.equal(a[k], d1[k]), k


# (shape, Tv, t0, b0): N = 16 with four origins per workgroup, and three waves per origin; a row inside the data and a planned one
@pytest.mark.parametrize("shape,Tv,t0,b0", [((5, 3, 2, 1, 32, 16, 3, 0), 5, 2, 1), ((5, 3, 2, 1, 32, 16, 3, 0), 7, 5, 2),
                                            ((4, 2, 4, 3, 64, 192, 3, 1), 6, 2, 1), ((4, 2, 4, 3, 64, 192, 3, 1), 6, 4, 0)],
                         ids=["N16-inside", "N16-planned", "N192-inside", "N192-planned"])
def test_one_row_alignment(built_lib, shape, Tv, t0, b0):
    """hb_f non-zero in the single row (t0, b0): against the zero launch every (k, t, b) output is bit-equal unless b == b0 and
    t <= t0 < t + k -- origin t meets row t + j at the transition j -> j + 1 -- and an output that may differ does differ"""
    T, B, Dx, Dy, H, N, K, emission = shape
    c = R.system(*shape, weights="finite", noisy=True)
    rows = torch.zeros(Tv, B, H)
    rows[t0, b0] = XR.hb_rows(1, 1, H, seed=5)[0, 0]
    one, zero = _launch(c, hb_f=rows, shape=shape), _launch(c, hb_f=torch.zeros_like(rows), shape=shape)
    k, t, b = torch.meshgrid(torch.arange(K + 1), torch.arange(T), torch.arange(B), indexing="ij")
    may = (b == b0) & (t <= t0) & (t0 < t + k)
    assert bool(may.any()) and bool((~may).any())
    for key in R.KEYS:
        o, z = one[key].cpu(), zero[key].cpu()
        differs = (o != z) if o.dim() == 3 else (o != z).any(-1)
        assert not bool((differs & ~may).any()), (key, torch.nonzero(differs & ~may)[:4])
        if key != "lpd":        # (lpd is 0 by contract past the data on both sides)
            assert bool(differs[may].all()), (key, torch.nonzero(~differs & may)[:4])
    lpd_may = may & (t + k < T)
    assert bool(((one["lpd"].cpu() != zero["lpd"].cpu()) == lpd_may).all())


def test_op_refuses_bad_rows(built_lib):
    c = XR.case("four-origins")
    T, B, H = c["shape"][0], c["shape"][1], c["shape"][4]
    with pytest.raises(ValueError, match=r"hb_f must have shape .*Tv >= T"):
        _launch(c, hb_f=torch.zeros(T - 1, B, H))
    for bad in ((T, B, H + 1), (T, B + 1, H), (T * B, H)):
        with pytest.raises(ValueError, match="hb_f must have shape"):
            _launch(c, hb_f=torch.zeros(*bad))
    from psvo_amd import ops
    desc = ops.make_desc(B, T, 600, 1, 2, 1, H)
    with pytest.raises(ValueError, match="unsupported"):
        ops.particle_forecast(desc, 0, _cuda(c["f"]), _cuda(c["g"]), c["sig_f"].cuda(), c["sig_g"].cuda(),
                              torch.zeros(T, B, 2, 600, device="cuda"), hb_f=torch.zeros(T, B, H, device="cuda"))


# ---- through the model -----------------------------------------------------------------------------------------------------------
CASE = ("AESMC", 4, 12, 16, 1, 2, 1, 16, True, True)           # B = 4, T = 12, N = 16, Dx = 2, Dy = 1, H = 16
DI, K_MODEL = 2, 4


def _inputs(B, Tv, Di, seed=31):
    return torch.randn(B, Tv, Di, generator=torch.Generator().manual_seed(seed)).cuda()


def _model_case(smc, model, hidden, obs, v, K, eps):
    """the restatement's inputs for the cloud `hidden` (B,T,N,Dx) of an evaluation under the inputs v (B,Tv,Di) -- the rows as the
    objective makes them -- and both references"""
    cpu = lambda x: tuple(cpu(u) for u in x) if isinstance(x, tuple) else x.detach().float().cpu().contiguous()
    assert model.use_bootstrap
    fp = tuple(smc._mlp_params(model.q1_tran))
    obs_TB = cpu(obs.transpose(0, 1))
    c = dict(f=cpu(smc._state_rows(fp)), g=cpu(tuple(smc._mlp_params(model.g_tran))), sig_f=cpu(smc.q1.get_sigma()),
             sig_g=cpu(smc.g.get_sigma()), X=cpu(hidden.permute(1, 0, 3, 2)), logW=None, obs=obs_TB,
             eps=None if eps is None else cpu(eps), K=K, emission=0,
             hb_f=cpu(smc._input_share(v.transpose(0, 1).contiguous().float(), fp)))
    assert c["f"][0].shape[0] == model.Dx and c["hb_f"].shape == (v.shape[1], v.shape[0], c["f"][0].shape[1])
    c["ref64"], c["ref32"] = XR.run(c, torch.float64), XR.run(c, torch.float32)
    c["valid"] = XR.scored(obs_TB, hidden.shape[1], K)
    return c


@pytest.mark.parametrize("ahead", [0, K_MODEL], ids=["Tv=T", "Tv=T+K"])
def test_through_the_objective(built_lib, ahead):
    """smc.particle_forecast(K, log["Xs"], obs, noise={"eps_p": ..}, inputs=v) is the restatement on the same cloud"""
    obj, B, T, N, M, Dx, Dy = CASE[:7]
    K = K_MODEL
    FLAGS, model, smc, obs = _setup(*CASE, Di=DI, particle_forecast=True, particle_forecast_inputs=True)
    assert smc.forecast is True and smc.Di == DI and model.q1_tran.kernels[0].shape[0] == Dx + DI
    v = _inputs(B, T + ahead, DI)
    eps = torch.randn(K, T, B, Dx, N, generator=torch.Generator().manual_seed(21)).cuda()
    with torch.no_grad():
        _, log = smc.get_log_ZSMC(obs, None, inputs=v[:, :T].contiguous())
        fc = smc.particle_forecast(K, log["Xs"], obs, noise={"eps_p": eps}, inputs=v)
        short = smc.particle_forecast(K, log["Xs"], obs, noise={"eps_p": eps}, inputs=v[:, :T].contiguous())
        with pytest.raises(ValueError, match="pass inputs"):
            smc.particle_forecast(K, log["Xs"], obs)
    torch.cuda.synchronize()
    assert set(fc) == {"y_mean", "y_var", "x_mean", "lpd", "valid", "forecast"}
    assert fc["y_mean"].shape == (B, T, K + 1, Dy) and fc["x_mean"].shape == (B, T, K + 1, Dx) and fc["lpd"].shape == (B, T, K + 1)
    assert torch.equal(fc["valid"].cpu(), R.valid_mask(T, K).t())
    assert (fc["lpd"].permute(1, 2, 0)[~fc["valid"]] == 0).all()
    c = _model_case(smc, model, log["Xs"], obs, v, K, eps)
    _judge("exo-model-Tv=T+%d" % ahead, _kernel_layout(fc), c)
    # the planned rows are read: they change the forecasts that reach past the data, and those alone
    assert torch.equal(short["y_mean"], fc["y_mean"]) == (ahead == 0)
    assert torch.equal(short["y_mean"][:, :T - K], fc["y_mean"][:, :T - K])


def test_degenerate_cloud_is_the_point_forecast(built_lib):
    """N copies of one point, noise off: y_mean is n_step_prediction(..., inputs=v) on that point, at the bound
    tests/test_gpu_forecast.py uses for this arithmetic"""
    obj, B, T, N, M, Dx, Dy = CASE[:7]
    K = 5
    FLAGS, model, smc, obs = _setup(*CASE, Di=DI, particle_forecast=True, particle_forecast_inputs=True, forecast_noise=False)
    v = _inputs(B, T, DI)
    point = torch.randn(B, T, 1, Dx, generator=torch.Generator().manual_seed(13)).cuda() * 1.5
    hidden = point.expand(B, T, N, Dx)
    with torch.no_grad():
        fc = smc.particle_forecast(K, hidden, obs, inputs=v)
        y_hat, y = smc.n_step_prediction(K, hidden, obs, inputs=v)
        quiet = smc.particle_forecast(K, hidden, obs, inputs=torch.zeros_like(v))
    torch.cuda.synchronize()
    for k in range(K + 1):
        assert torch.allclose(fc["y_mean"][:, :T - k, k], y_hat[k], atol=2e-4, rtol=1e-5), k
    # (the check can tell: without the inputs the point forecast is another one)
    assert float((quiet["y_mean"][:, :T - 1, 1] - y_hat[1]).abs().max()) > 100 * 2e-4


def test_training_is_unaffected(built_lib, monkeypatch):
    """under autograd the op is never launched; ELBO and every parameter gradient are bit-identical with the flags on and off"""
    from psvo_amd import ops
    case = ("AESMC", 2, 6, 16, 1, 2, 1, 32, True, True)
    FLAGS, model, smc, obs = _setup(*case, Di=DI, particle_forecast=True, particle_forecast_inputs=True)
    v = _inputs(2, 6, DI)
    noise = {"eps_f": torch.randn(6, 2, 2, 16, generator=torch.Generator().manual_seed(3)).cuda(),
             "u_f": torch.rand(6, 2, 16, generator=torch.Generator().manual_seed(4)).cuda()}

    def refuse(*a, **k):
        raise AssertionError("ops.particle_forecast was called under autograd")
    monkeypatch.setattr(ops, "particle_forecast", refuse)
    res = []
    for on in (True, False):
        smc = type(smc)(model, Hh.make_flags("AESMC", **{**FLAGS.as_dict(), "particle_forecast": on, "particle_forecast_inputs": on}))
        assert smc.forecast is on and smc.Di == DI
        model.zero_grad(set_to_none=True)
        z, log = smc.get_log_ZSMC(obs, None, noise=noise, inputs=v)
        z.backward()
        torch.cuda.synchronize()
        res.append((z.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
        with pytest.raises(ValueError, match="no gradient"):
            smc.particle_forecast(2, log["Xs"], obs, inputs=v)
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 4
    for n, g in res[0][1].items():
        assert torch.equal(g, res[1][1][n]), n


def test_runner_end_to_end(built_lib, tmp_path, monkeypatch):
    """runner.main with --AESMC --Di=1 --particle_forecast --particle_forecast_inputs for two epochs: the forecast_* keys are in
    metric_*.p, one finite number per horizon k = 0 .. MSE_steps"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    argv = ["--noPSVO", "--AESMC", "--Di=1", "--particle_forecast", "--particle_forecast_inputs", "--generateTrainingData",
            "--time=12", "--n_train=4", "--n_test=4", "--batch_size=2", "--n_particles=16", "--epoch=2", "--MSE_steps=5"]
    monkeypatch.chdir(tmp_path)
    runner.main(parse_flags(argv))
    torch.cuda.synchronize()
    metrics = glob.glob(str(tmp_path / "rslts" / "epoch_data" / "**" / "metric_*.p"), recursive=True)
    assert metrics
    for path in metrics:
        with open(path, "rb") as fh:
            m = pickle.load(fh)
        for split in ("train", "test"):
            for stem in ("forecast_lpd_", "forecast_R_square_", "forecast_calibration_"):
                v = m[stem + split]
                assert v.shape == (6,) and bool((v == v).all()) and bool(abs(v).max() < float("inf")), (stem, split, v)
            assert (m["forecast_calibration_" + split] > 0).all()
