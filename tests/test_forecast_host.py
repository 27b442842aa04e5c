"""The particle forecast (--particle_forecast) as far as it can be checked without a GPU: the reference restatement the GPU tests
compare against (tests/forecast_reference.py) against closed-form Gaussian moments and against itself in fp32, the flags, every
refusal, and the trainer's metrics with the op stubbed by the restatement."""
import glob
import math
import pickle

import numpy as np
import pytest
import torch

from tests import forecast_reference as R
from tests import helpers as Hh

CASES = R.cases()


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _linear_as_mlp(A, b):
    """x A + b as a one-hidden-layer relu MLP: x = relu(x) - relu(-x), H = 2 Din"""
    Din = A.shape[0]
    eye = torch.eye(Din, dtype=A.dtype)
    return torch.cat([eye, -eye], 1), torch.zeros(2 * Din, dtype=A.dtype), torch.cat([A, -A], 0), b


def test_restatement_against_closed_form_gaussian_moments():
    """linear f and g, a Gaussian cloud of N = 4096 equally weighted particles: y_mean and y_var at k = 0..3 agree with the
    moments of the linear-Gaussian recursion within 6 analytic standard errors -- sqrt(s2 / N) for a mean of variance s2,
    s2 sqrt(2 / N) for the variance of a Gaussian sample (its bias, s2 / N, is far inside that)"""
    T, B, Dx, Dy, N, K = 2, 2, 2, 2, 4096, 3
    gen = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    A = torch.tensor([[0.9, 0.2], [-0.3, 0.7]], dtype=torch.float64)
    C = torch.tensor([[1.0, -0.5], [0.4, 0.8]], dtype=torch.float64)
    d = torch.tensor([0.3, -0.2], dtype=torch.float64)
    sig_f = torch.tensor([0.3, 0.5], dtype=torch.float64)
    sig_g = torch.tensor([0.4, 0.7], dtype=torch.float64)
    m0 = torch.tensor([1.0, -2.0], dtype=torch.float64)
    L0 = torch.tensor([[0.8, 0.0], [0.3, 0.5]], dtype=torch.float64)
    X = (m0 + rn(T, B, N, Dx) @ L0.t()).permute(0, 1, 3, 2).contiguous()
    eps = rn(K, T, B, Dx, N)
    out = R.forecast(X, _linear_as_mlp(A, torch.zeros(Dx, dtype=torch.float64)), _linear_as_mlp(C, d), sig_f, sig_g, K, 0, eps=eps)
    m, P = m0, L0 @ L0.t()
    for k in range(K + 1):
        s2 = torch.diagonal(C.t() @ P @ C)                      # variance of the emission mean over the cloud
        se_mean, se_var = torch.sqrt(s2 / N), s2 * math.sqrt(2.0 / N)
        zm = ((out["ymean"][k] - (m @ C + d)).abs() / se_mean).max()
        zv = ((out["yvar"][k] - (s2 + sig_g ** 2)).abs() / se_var).max()
        zx = ((out["xmean"][k] - m).abs() / torch.sqrt(torch.diagonal(P) / N)).max()
        print("forecast-closed-form k %d: worst deviation in standard errors: ymean %.2f yvar %.2f xmean %.2f" % (k, zm, zv, zx))
        assert zm <= 6 and zv <= 6 and zx <= 6, k
        m, P = m @ A, A.t() @ P @ A + torch.diag(sig_f ** 2)


@pytest.mark.parametrize("shape,weights,noisy", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_restatement_fp32_against_fp64(shape, weights, noisy):
    """the systems of the GPU tests: finite fp64 log-densities at the valid entries, exact zeros elsewhere, positive variances
    (asserted by case() itself), and fp32 close to fp64 (the GPU tests' yardstick err_32, printed)"""
    T, B, Dx, Dy, H, N, K, emission = shape
    c = R.case(shape, weights, noisy)
    assert c["ref64"]["ymean"].shape == (K + 1, T, B, Dy) and c["ref64"]["xmean"].shape == (K + 1, T, B, Dx)
    assert c["ref64"]["lpd"].shape == (K + 1, T, B) and c["valid"].shape == (K + 1, T)
    assert (c["eps"] is not None) == (noisy and K > 0) and (c["logW"] is not None) == (weights != "none")
    if emission == 2:
        assert (c["obs"] >= 0).all() and (c["obs"] == c["obs"].floor()).all()
    for key in R.KEYS:
        err, biggest = R.error(c["ref32"], c["ref64"], key, c["valid"])
        print("forecast-reference %s %s err_32 %.3e max|ref_64| %.3f" % ("-".join(map(str, shape)), key, err, biggest))
        assert err <= 1e-3 * max(1.0, biggest), key
    # equal finite log-weights are no weights
    if weights == "none":
        a = R._as(c, torch.float64)
        same = R.forecast(a["X"], a["f"], a["g"], a["sig_f"], a["sig_g"], K, emission, logW=torch.full((T, B, N), -2.5,
                          dtype=torch.float64), obs=a["obs"], eps=a["eps"])
        for key in R.KEYS:
            assert float((same[key] - c["ref64"][key]).abs().max()) <= 1e-12 * max(1.0, float(c["ref64"][key].abs().max())), key


# ---- flags and refusals -------------------------------------------------------------------------------------------------------
def test_flags():
    from psvo_amd.flags import Flags, parse_flags
    assert Flags().particle_forecast is False and Flags().forecast_noise is True
    assert parse_flags([]).particle_forecast is False and parse_flags([]).forecast_noise is True
    F = parse_flags(["--particle_forecast"])
    assert F.particle_forecast is True and F.forecast_noise is True
    F = parse_flags(["--particle_forecast", "--noforecast_noise"])
    assert F.particle_forecast is True and F.forecast_noise is False
    assert parse_flags(["--forecast_noise=false"]).forecast_noise is False
    assert parse_flags(["--particle_forecast", "--noparticle_forecast"]).particle_forecast is False
    assert Flags(particle_forecast=True).as_dict()["particle_forecast"] is True


def test_objectives_carry_the_flags():
    from psvo_amd.SMC.SVO import SVO

    class _Model:
        q0_dist = q1_dist = q2_dist = f_dist = g_dist = None
    smc = SVO(_Model(), Hh.make_flags("SVO", particle_forecast=True, forecast_noise=False))
    assert smc.forecast is True and smc.forecast_noise is False
    smc = SVO(_Model(), Hh.make_flags("SVO"))
    assert smc.forecast is False and smc.forecast_noise is True
    F = Hh.make_flags("SVO")
    del F.particle_forecast, F.forecast_noise
    smc = SVO(_Model(), F)
    assert smc.forecast is False and smc.forecast_noise is True


def _model(obj="AESMC", **kw):
    from psvo_amd.model import SSM
    base = dict(Dx=2, Dy=1, n_particles=8, batch_size=2, time=6, q0_layers="16", q1_layers="16", q2_layers="16", f_layers="16",
                g_layers="16", y_smoother_Dhs="8", X0_smoother_Dhs="8")
    base.update(kw)
    FLAGS = Hh.make_flags(obj, **base)
    torch.manual_seed(0)
    return FLAGS, Hh.perturb_(SSM(FLAGS))


@pytest.mark.parametrize("kw,match", [
    (dict(output_cov=True, diag_cov=True), "state-independent scales"),
    (dict(q1_layers="16,16", g_layers="16,16"), "one hidden layer"),
    (dict(g_layers="16,16"), "one hidden layer"),
], ids=["output_cov", "two-layers", "two-layer-g"])
def test_objective_refuses_what_the_kernel_does_not_cover(kw, match):
    from psvo_amd.SMC.AESMC import AESMC
    from psvo_amd.SMC.PSVO import PSVO
    for obj, cls in (("AESMC", AESMC), ("PSVO", PSVO)):
        FLAGS, model = _model(obj, particle_forecast=True, **kw)
        with pytest.raises(ValueError, match=match):
            cls(model, FLAGS)
        FLAGS.particle_forecast = False
        try:
            smc = cls(model, FLAGS)                    # flag off: nothing new is refused
        except ValueError as exc:                      # (what the objective itself refuses stays refused)
            assert "particle_forecast" not in str(exc)
            continue
        with pytest.raises(ValueError, match=match):   # ... and the method refuses by itself
            with torch.no_grad():
                smc.particle_forecast(2, torch.zeros(2, 6, 8, 2), torch.zeros(2, 6, 1))


def test_route_refuses_wide_dy():
    from psvo_amd.SMC.SVO import SVO

    class _Wide:
        Dy, output_cov = 33, False
    with pytest.raises(ValueError, match="1 <= Dy <= 32"):
        SVO._route_forecast(_Wide(), True)
    assert SVO._route_forecast(_Wide(), False) is False
    _Wide.Dy = 32
    assert SVO._route_forecast(_Wide(), True) is True


def test_method_refuses_autograd():
    from psvo_amd.SMC.AESMC import AESMC
    FLAGS, model = _model(particle_forecast=True)
    smc = AESMC(model, FLAGS)
    with pytest.raises(ValueError, match="no gradient"):
        smc.particle_forecast(2, torch.zeros(2, 6, 8, 2), torch.zeros(2, 6, 1))


# ---- the objective's method and the trainer, with the op stubbed by the restatement ------------------------------------------------
def _stub_op(calls):
    def particle_forecast(desc, K, f, g, sig_f, sig_g, X, logW=None, obs=None, eps=None):
        calls.append(dict(desc=desc, K=K, X=X, eps=eps, obs=obs, logW=logW))
        assert X.is_contiguous() and tuple(X.shape) == (desc.T, desc.B, desc.Dx, desc.N)
        return R.forecast(X, f, g, sig_f, sig_g, K, desc.emission, logW=logW, obs=obs, eps=eps)
    return particle_forecast


def test_method_layouts_and_noise(monkeypatch):
    from psvo_amd import ops
    from psvo_amd.SMC.AESMC import AESMC
    B, T, N, Dx, Dy, K = 2, 6, 8, 2, 1, 7
    FLAGS, model = _model(particle_forecast=True)
    calls = []
    monkeypatch.setattr(ops, "particle_forecast", _stub_op(calls))
    smc = AESMC(model, FLAGS)
    gen = torch.Generator().manual_seed(1)
    X = torch.randn(T, B, Dx, N, generator=gen)
    hidden = X.permute(1, 0, 3, 2)                      # what log["Xs"] is: a view of a kernel-layout tensor
    obs = torch.randn(B, T, Dy, generator=gen)
    eps = torch.randn(K, T, B, Dx, N, generator=gen)
    with torch.no_grad():
        out = smc.particle_forecast(K, hidden, obs, noise={"eps_p": eps})
    assert calls[-1]["X"].data_ptr() == X.data_ptr()    # permuted back without a copy
    assert calls[-1]["eps"] is eps and calls[-1]["logW"] is None and calls[-1]["desc"].layers == 1
    assert out["y_mean"].shape == (B, T, K + 1, Dy) and out["y_var"].shape == (B, T, K + 1, Dy)
    assert out["x_mean"].shape == (B, T, K + 1, Dx) and out["lpd"].shape == (B, T, K + 1) and out["valid"].shape == (T, K + 1)
    assert torch.equal(out["valid"], R.valid_mask(T, K).t())
    assert (out["lpd"].permute(1, 2, 0)[~out["valid"]] == 0).all() and torch.isfinite(out["lpd"]).all()
    assert torch.equal(out["x_mean"][:, :, 0], hidden.mean(2))
    # bootstrap wiring: f is q1's network and scale -- the noise-free one-step mean of a degenerate cloud is q1's mean
    with torch.no_grad():
        one = smc.particle_forecast(1, hidden[:, :, :1].expand(B, T, N, Dx), obs, noise={"eps_p": torch.zeros(1, T, B, Dx, N)})
        want = model.q1_dist.mean(hidden[:, :, 0])
    assert torch.allclose(one["x_mean"][:, :, 1], want, atol=1e-5)
    # the objective's own draws (reproducible from its generator), and none with --noforecast_noise
    with torch.no_grad():
        smc.generator = torch.Generator().manual_seed(3)
        a = smc.particle_forecast(K, hidden, obs)
        smc.generator.manual_seed(3)
        b = smc.particle_forecast(K, hidden, obs)
        assert tuple(calls[-1]["eps"].shape) == (K, T, B, Dx, N)
        assert torch.equal(a["y_mean"], b["y_mean"]) and not torch.equal(a["y_mean"], out["y_mean"])
        smc.forecast_noise = False
        smc.particle_forecast(K, hidden, obs)
        assert calls[-1]["eps"] is None


class _Recorder:
    """trainer.evaluate with the fetch lists it was asked for kept"""

    def __init__(self, tr):
        self.fetches, self.inner = [], tr.evaluate
        tr.evaluate = self

    def __call__(self, fetches, *a, **kw):
        self.fetches.append(list(fetches) if isinstance(fetches, list) else fetches)
        return self.inner(fetches, *a, **kw)


def _trainer(monkeypatch, tmp_path, on):
    """a trainer on the CPU around an AESMC whose filter is replaced by a fixed cloud; ops.particle_forecast is the restatement"""
    from psvo_amd import ops
    from psvo_amd.SMC.AESMC import AESMC
    from psvo_amd.trainer import trainer
    B, T, N, Dx, Dy, K = 2, 6, 8, 2, 1, 3
    FLAGS, model = _model(particle_forecast=on, MSE_steps=K, saving_num=2)
    calls = []
    monkeypatch.setattr(ops, "particle_forecast", _stub_op(calls))

    class _Fixed(AESMC):
        def get_log_ZSMC(self, obs, hidden, noise=None):
            seed = int(obs.abs().sum() * 1000) % 1000
            gen = torch.Generator().manual_seed(seed)
            self.generator.manual_seed(seed)          # (the forecast's own draws: the same whenever a batch is evaluated again)
            return torch.tensor(-1.5), {"Xs": torch.randn(T, obs.shape[0], Dx, N, generator=gen).permute(1, 0, 3, 2)}
    smc = _Fixed(model, FLAGS)
    smc.generator = torch.Generator().manual_seed(2)
    tr = trainer(model, smc, FLAGS)
    tr.init_data_saving(str(tmp_path / "rslts" / "run") + "/")
    gen = torch.Generator().manual_seed(4)
    tr.obs_train, tr.obs_test = torch.randn(4, T, Dy, generator=gen).numpy(), torch.randn(2, T, Dy, generator=gen).numpy()
    tr.hidden_train, tr.hidden_test = np.zeros((4, T, Dx)), np.zeros((2, T, Dx))
    return tr, calls, (B, T, N, Dx, Dy, K)


def test_trainer_metrics_keys_and_shapes(monkeypatch, tmp_path, capsys):
    tr, calls, (B, T, N, Dx, Dy, K) = _trainer(monkeypatch, tmp_path, True)
    rec = _Recorder(tr)
    tr.evaluate_and_save_metrics(0)
    assert rec.fetches == [["log_ZSMC", "y_hat", "y", "forecast_y_mean", "forecast_y_var", "forecast_lpd"]] * 2
    assert len(calls) == 3                                       # two training batches, one held-out batch
    with open(glob.glob(tr.epoch_data_DIR + "metric_1.p")[0], "rb") as fh:
        m = pickle.load(fh)
    for split in ("train", "test"):
        for stem in ("forecast_lpd_", "forecast_R_square_", "forecast_calibration_"):
            v = m[stem + split]
            assert isinstance(v, np.ndarray) and v.shape == (K + 1,) and np.isfinite(v).all(), stem + split
        assert (m["forecast_calibration_" + split] > 0).all() and (m["forecast_R_square_" + split] <= 1).all()
        assert m["R_square_" + split].shape == (K + 1,)
    printed = capsys.readouterr().out
    assert "particle forecast" in printed and "calibration" in printed
    # the numbers are those of the definition, from the fetched arrays
    ym, yv, lpd = tr.evaluate(["forecast_y_mean", "forecast_y_var", "forecast_lpd"], {tr.obs: tr.obs_test, tr.hidden: tr.hidden_test})
    assert ym.shape == (2, T, K + 1, Dy) and yv.shape == ym.shape and lpd.shape == (2, T, K + 1)
    for k in range(K + 1):
        y = tr.obs_test[:, k:]
        assert np.isclose(m["forecast_lpd_test"][k], lpd[:, :T - k, k].mean())
        assert np.isclose(m["forecast_calibration_test"][k], (np.square(y - ym[:, :T - k, k]) / yv[:, :T - k, k]).mean())
        assert (lpd[:, T - k:, k] == 0).all()
    # the saved sequences gain the predictive moments
    tr._save_epoch_samples(1, tr.obs_test, tr.hidden_test, True)
    with open(tr.epoch_data_DIR + "y_hat_1.p", "rb") as fh:
        saved = pickle.load(fh)
    assert set(saved) == {"y_hat", "y_mean", "y_var"} and saved["y_mean"].shape == (2, T, K + 1, Dy)
    assert saved["y_var"].shape == (2, T, K + 1, Dy) and len(saved["y_hat"]) == K + 1
    with open(tr.epoch_data_DIR + "trajectory_1.p", "rb") as fh:
        assert set(pickle.load(fh)) == {"Xs"}


def test_flag_off_changes_nothing(monkeypatch, tmp_path, capsys):
    tr, calls, (B, T, N, Dx, Dy, K) = _trainer(monkeypatch, tmp_path, False)
    rec = _Recorder(tr)
    tr.evaluate_and_save_metrics(0)
    tr._save_epoch_samples(1, tr.obs_test, tr.hidden_test, True)
    assert rec.fetches == [["log_ZSMC", "y_hat", "y"]] * 2 + ["Xs", "y_hat"]
    assert calls == []
    with open(tr.epoch_data_DIR + "metric_1.p", "rb") as fh:
        m = pickle.load(fh)
    assert set(m) == {"log_ZSMC_train", "log_ZSMC_test", "R_square_train", "R_square_test"}
    with open(tr.epoch_data_DIR + "y_hat_1.p", "rb") as fh:
        assert set(pickle.load(fh)) == {"y_hat"}
    assert "forecast" not in capsys.readouterr().out
