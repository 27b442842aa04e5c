"""Host side of exogenous inputs (FLAGS.Di): the flag, routing, refusals, the loader and the generator, the alignment of
n_step_prediction, and the fp64 reference of tests/exo_reference.py against the missing-observation reference and against itself
(anchors, the separation condition of the GPU cases, the fp32 reference's own error).  No GPU."""
import pickle

import numpy as np
import pytest
import torch

from tests import exo_reference as ER
from tests import helpers as Hh
from tests import missing_reference as MR

# the value tolerances of tests/test_gpu_exo.py (max-abs on logW)
LOGW_ATOL = 5e-4


def _objective(obj, **kw):
    from psvo_amd.model import SSM
    from psvo_amd.SMC.AESMC import AESMC
    from psvo_amd.SMC.IWAE import IWAE
    from psvo_amd.SMC.PSVO import PSVO
    from psvo_amd.SMC.PSVOwR import PSVOwR
    from psvo_amd.SMC.SVO import SVO
    FLAGS = Hh.make_flags(obj, **kw)
    model = SSM(FLAGS)
    return FLAGS, model, {"AESMC": AESMC, "IWAE": IWAE, "PSVO": PSVO, "PSVOwR": PSVOwR, "SVO": SVO}[obj](model, FLAGS)


def test_flag_parsing_and_default():
    from psvo_amd.flags import Flags, parse_flags
    assert Flags().Di == 0 and parse_flags([]).Di == 0
    F = parse_flags(["--noPSVO", "--AESMC", "--Di=2", "--generateTrainingData"])
    assert F.Di == 2 and isinstance(F.Di, int) and F.AESMC
    assert parse_flags(["--Di", "3"]).Di == 3
    assert "Di" in Flags().as_dict()


def test_routing_and_shapes():
    from psvo_amd import autograd, ops
    assert hasattr(autograd, "FilterWobsInputFunction")
    for name in ("filter_forward_wobs_input", "filter_backward_wobs_input", "mlp_wgrad_rowbias"):
        assert hasattr(ops, name), name
    for obj in ("AESMC", "SVO", "IWAE"):
        for Dy in (1, 2, 3, 32):
            FLAGS, model, smc = _objective(obj, Dy=Dy, Dx=3, Di=2)
            assert smc.Di == 2 and model.Di == 2 and smc.wide_obs is False and smc.missing_obs is False
            assert model.q1_tran.kernels[0].shape == (5, model.q1_tran.Dhs[0]) and model.q1_tran.Di == 2
            assert model.f_tran.kernels[0].shape[0] == 5 and model.g_tran.kernels[0].shape[0] == 3 and model.g_tran.Di == 0
            assert model.q0_tran.Di == 0 and (model.q2_tran is None or model.q2_tran.Di == 0)
        # Di = 0: nothing changes
        FLAGS, model, smc = _objective(obj, Dy=10, Dx=3)
        assert smc.Di == 0 and model.Di == 0 and smc.wide_obs is True and model.q1_tran.kernels[0].shape[0] == 3
    # every emission form at every width, missing observations and the smoothers beside it
    for kw in (dict(poisson_emission=True), dict(count_emission=True), dict(missing_obs=True),
               dict(FFBS=True, FFBSi=True, MAP_path=True)):
        for Dy in (1, 5):
            assert _objective("AESMC", Dy=Dy, Di=1, **kw)[2].Di == 1
    sep = _objective("SVO", Dy=2, Dx=3, Di=2, use_bootstrap=False)[1]
    assert sep.f_tran is not sep.q1_tran and sep.f_tran.Di == 2 and sep.f_tran.kernels[0].shape[0] == 5


def test_di_zero_builds_the_same_model():
    """with Di = 0 the model's parameters are those of a build without the flag: same shapes, same draws from the generator"""
    from psvo_amd.flags import Flags
    from psvo_amd.model import SSM
    F = Hh.make_flags("SVO", Dx=3, Dy=2, use_bootstrap=False)
    torch.manual_seed(4)
    a = SSM(F)
    F2 = Hh.make_flags("SVO", Dx=3, Dy=2, use_bootstrap=False)
    del F2.Di                                   # (flags as they were before the feature)
    torch.manual_seed(4)
    b = SSM(F2)
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert pa.keys() == pb.keys()
    for n in pa:
        assert torch.equal(pa[n], pb[n]), n
    assert "Di" in Flags().as_dict()


@pytest.mark.parametrize("obj,kw,word", [
    ("AESMC", dict(Di=-1), r"--Di = -1.*Di >= 0"),
    ("PSVO", dict(Di=1), r"--Di with --PSVO / --PSVOwR.*no input form"),
    ("PSVOwR", dict(Di=1), r"--Di with --PSVO / --PSVOwR"),
    ("AESMC", dict(Di=1, resample_ess=0.5), r"--Di with --resample_ess"),
    ("AESMC", dict(Di=1, particle_forecast=True), r"--Di with --particle_forecast"),
    ("AESMC", dict(Di=1, output_cov=True, diag_cov=True), r"--Di with output_cov"),
    ("AESMC", dict(Di=1, q1_layers="32,32", g_layers="32,32"), r"--Di with per-particle MLP layers.*one hidden layer"),
    ("SVO", dict(Di=1, Dy=10, Dx=3, g_layers="16,16"), r"--Di with per-particle MLP layers.*one hidden layer"),
    ("AESMC", dict(Di=1, Dy=33, Dx=3), r"--Di with Dy = 33.*1 <= Dy <= 32"),
], ids=["negative", "PSVO", "PSVOwR", "resample_ess", "particle_forecast", "output_cov", "two-layers", "two-layers-g", "Dy33"])
def test_refusals(obj, kw, word):
    with pytest.raises(ValueError, match=word):
        _objective(obj, **kw)


def test_check_inputs_names_every_limit():
    """the check runner.main makes on the flags alone"""
    from psvo_amd.SMC.SVO import check_inputs
    ok = dict(Dy=10, layers=["32", "32"])
    assert check_inputs(2, **ok) == 2 and check_inputs(1, Dy=1, layers=[[64]]) == 1 and check_inputs(4, Dy=32, layers=["16"]) == 4
    # off: nothing to refuse, whatever else is set
    assert check_inputs(0, backward_simulation=True, resample_ess=0.5, particle_forecast=True, output_cov=True, Dy=40,
                        layers=["32,32"]) == 0
    assert check_inputs(None) == 0
    for kw, word in ((dict(ok, backward_simulation=True), "--PSVO / --PSVOwR"),
                     (dict(ok, resample_ess=0.5), "--resample_ess"),
                     (dict(ok, particle_forecast=True), "--particle_forecast"),
                     (dict(ok, output_cov=True), "output_cov"),
                     (dict(ok, layers=["32", "32,32"]), r"per-particle MLP layers \[\[32, 32\]\].*one hidden layer"),
                     (dict(ok, Dy=33), r"Dy = 33.*1 <= Dy <= 32"),
                     (dict(ok, Dy=0), r"Dy = 0.*1 <= Dy <= 32")):
        with pytest.raises(ValueError, match=word):
            check_inputs(1, **kw)
    with pytest.raises(ValueError, match=r"--Di = -2"):
        check_inputs(-2, **ok)


def test_runner_refuses_before_it_touches_a_device(monkeypatch):
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags

    def unreachable(*a, **k):
        raise AssertionError("runner.main went on after a refusal")
    monkeypatch.setattr(runner, "_device", unreachable)
    monkeypatch.setattr(runner, "_dataset", unreachable)
    for argv, word in ((["--Di=1"], "--PSVO / --PSVOwR"),                                  # (PSVO is the default objective)
                       (["--noPSVO", "--PSVOwR", "--Di=1"], "--PSVO / --PSVOwR"),
                       (["--noPSVO", "--AESMC", "--Di=-1"], "Di >= 0"),
                       (["--noPSVO", "--AESMC", "--Di=1", "--resample_ess=0.5"], "--Di with --resample_ess"),
                       (["--noPSVO", "--AESMC", "--Di=1", "--particle_forecast"], "--Di with --particle_forecast"),
                       (["--noPSVO", "--AESMC", "--Di=1", "--output_cov", "--diag_cov"], "output_cov"),
                       (["--noPSVO", "--AESMC", "--Di=1", "--g_layers=32,32"], "one hidden layer"),
                       (["--noPSVO", "--AESMC", "--Di=1", "--Dy=33"], "1 <= Dy <= 32")):
        with pytest.raises(ValueError, match=word):
            runner.main(parse_flags(argv))


def test_get_log_ZSMC_checks_the_inputs():
    """missing or mis-shaped inputs are refused before anything is computed; so are inputs to a model without the channel"""
    _, _, smc = _objective("AESMC", Dy=2, Dx=3, Di=2)
    obs = torch.zeros(2, 6, 2)
    with pytest.raises(ValueError, match=r"--Di = 2.*pass inputs"):
        smc.get_log_ZSMC(obs, None)
    for bad in (torch.zeros(2, 6, 1), torch.zeros(2, 5, 2), torch.zeros(6, 2, 2), torch.zeros(2, 6)):
        with pytest.raises(ValueError, match=r"--Di = 2: inputs must be \(batch, time, Di\)"):
            smc.get_log_ZSMC(obs, None, inputs=bad)
    _, _, plain = _objective("AESMC", Dy=2, Dx=3)
    with pytest.raises(ValueError, match="without an input channel"):
        plain.get_log_ZSMC(obs, None, inputs=torch.zeros(2, 6, 2))


# ---- the transformation ---------------------------------------------------------------------------------------------------
def test_mean_takes_the_input_rows_and_none_means_zeros():
    _, model, smc = _objective("SVO", Dy=2, Dx=3, Di=2, use_bootstrap=False)
    Hh.perturb_(model)
    x, v = torch.randn(4, 7, 3), torch.randn(4, 7, 2)
    tr = model.f_tran
    W1, b1 = tr.kernels[0], tr.biases[0]
    want = torch.relu(torch.cat([x, v], -1) @ W1 + b1) @ tr.mu_kernel + tr.mu_bias
    assert torch.equal(model.f_dist.mean(x, inputs=v), want)
    assert torch.equal(model.f_dist.mean(x), model.f_dist.mean(x, inputs=torch.zeros_like(v)))
    assert torch.equal(smc.get_nextX(x), model.f_dist.mean(x))                       # quiver plots: zero input
    assert not torch.equal(model.f_dist.mean(x), want)
    with pytest.raises(ValueError, match="inputs .* beside states"):
        model.f_dist.mean(x, inputs=v[:, :6])
    with pytest.raises(ValueError, match="state columns expected"):
        model.f_dist.mean(torch.randn(4, 7, 5))
    with pytest.raises(ValueError, match=r"without input columns \(Di = 0\)"):
        model.g_tran.transform(x, v)


def test_n_step_prediction_alignment():
    """horizon k pushes the mean through f with inputs[:, k:T-1]: the state of origin t at horizon k meets v_{t+k}"""
    _, model, smc = _objective("SVO", Dy=2, Dx=3, Di=2, use_bootstrap=False)
    Hh.perturb_(model)
    B, T, N, K = 2, 7, 5, 3
    hidden, obs, v = torch.randn(B, T, N, 3), torch.randn(B, T, 2), torch.randn(B, T, 2)
    with torch.no_grad():
        y_hat, y = smc.n_step_prediction(K, hidden, obs, inputs=v)
        tr = model.f_tran
        f = lambda x, vv: torch.relu(torch.cat([x, vv], -1) @ tr.kernels[0] + tr.biases[0]) @ tr.mu_kernel + tr.mu_bias
        for t in range(T):
            x = hidden[:, t].mean(1)
            for k in range(K + 1):
                if t + k >= T:
                    break
                assert torch.allclose(y_hat[k][:, t], model.g_dist.mean(x), atol=1e-6), (t, k)
                assert torch.equal(y[k][:, t], obs[:, t + k])
                x = f(x, v[:, t + k])
        # the input matters, and one step out of line shows
        other, _ = smc.n_step_prediction(K, hidden, obs, inputs=torch.roll(v, 1, dims=1))
        assert float((other[1] - y_hat[1]).abs().max()) > 1e-3
    assert [a.shape[1] for a in y_hat] == [T - k for k in range(K + 1)]
    with pytest.raises(ValueError, match="pass inputs"):
        smc.n_step_prediction(K, hidden, obs)
    _, _, plain = _objective("SVO", Dy=2, Dx=3)
    with pytest.raises(ValueError, match="without an input channel"):
        plain.n_step_prediction(K, hidden, obs, inputs=v)


# ---- loader and generator -------------------------------------------------------------------------------------------------
def _datadict(tmp_path, **arrays):
    path = tmp_path / "data.p"
    with open(path, "wb") as fh:
        pickle.dump(arrays, fh)
    return str(path)


def test_loader_reads_the_inputs(tmp_path):
    from psvo_amd.utils.data_loader import load_data
    rng = np.random.RandomState(0)
    Y, Yv, Yt = rng.randn(6, 9, 2), rng.randn(3, 9, 2), rng.randn(4, 9, 2)
    V, Vv, Vt = rng.randn(6, 9, 1), rng.randn(3, 9, 1), rng.randn(4, 9, 1)
    base = dict(Ytrain=Y, Yvalid=Yv, Ytest=Yt)
    path = _datadict(tmp_path, Vtrain=V, Vvalid=Vv, Vtest=Vt, **base)
    plain = load_data(path, 3, False, False)
    assert len(plain) == 4 and len(load_data(path, 3, False, False, Di=0)) == 4      # Di = 0: the result as it was
    out = load_data(path, 3, False, False, Di=1)
    assert len(out) == 6
    for a, b in zip(out[:4], plain):
        assert np.array_equal(a, b)
    assert np.array_equal(out[2], Y) and np.array_equal(out[3], Yt)                  # (the larger held-out split: Ytest)
    assert np.array_equal(out[4], V) and np.array_equal(out[5], Vt)                  # ... and the inputs that go with it
    only_valid = _datadict(tmp_path, Ytrain=Y, Yvalid=Yv, Vtrain=V, Vvalid=Vv)
    assert np.array_equal(load_data(only_valid, 3, False, False, Di=1)[5], Vv)
    flat = _datadict(tmp_path, Ytrain=Y, Yvalid=Yv, Vtrain=V[:, :, 0], Vvalid=Vv[:, :, 0])     # (n, T) gets the feature axis
    assert load_data(flat, 3, False, False, Di=1)[4].shape == (6, 9, 1)
    for arrays, word in ((dict(base), "holds no exogenous inputs under 'Vtrain'"),
                         (dict(base, Vtrain=V), "holds no exogenous inputs under 'Vtest'"),
                         (dict(base, Vtrain=V, Vtest=Vt[:, :8]), r"Vtest must be \(n, T, Di\)"),
                         (dict(base, Vtrain=rng.randn(6, 9, 2), Vtest=Vt), r"Vtrain must be \(n, T, Di\) = \(6, 9, 1\)"),
                         (dict(base, Vtrain=np.where(np.arange(9)[None, :, None] == 4, np.nan, V), Vtest=Vt), "non-finite")):
        with pytest.raises(ValueError, match=word):
            load_data(_datadict(tmp_path, **arrays), 3, False, False, Di=1)


def test_generator_inputs_are_seeded_pulses():
    from psvo_amd.utils.data_generator import FHN_PARAMS, _fhn_step, generate_dataset
    np.random.seed(5)
    plain = generate_dataset(3, 2, 30, model="fhn", Dy=1)
    np.random.seed(5)
    again = generate_dataset(3, 2, 30, model="fhn", Dy=1, input_dim=0)
    assert len(plain) == 4 and all(np.array_equal(a, b) for a, b in zip(plain, again))      # off: the data as they were
    np.random.seed(5)
    d1 = generate_dataset(3, 2, 30, model="fhn", Dy=1, input_dim=1)
    np.random.seed(5)
    d2 = generate_dataset(3, 2, 30, model="fhn", Dy=1, input_dim=1)
    assert len(d1) == 6 and all(np.array_equal(a, b) for a, b in zip(d1, d2))               # reproducible under the seed
    Xtr, Xte, Ytr, Yte, Vtr, Vte = d1
    assert Vtr.shape == (3, 30, 1) and Vte.shape == (2, 30, 1) and np.isfinite(Vtr).all()
    for v in list(Vtr) + list(Vte):                  # piecewise constant: few levels, runs of at least 5 steps inside
        change = np.flatnonzero(np.diff(v[:, 0]) != 0)
        assert len(change) <= 30 // 5 and (len(change) < 2 or np.diff(change).min() >= 5)
    assert any(np.unique(v).size > 1 for v in Vtr) and not np.array_equal(Vtr[0], Vtr[1])
    # the current of the step t -> t + 1 is I + v_t
    for t in range(29):
        assert np.allclose(Xtr[0, t + 1], _fhn_step(Xtr[0, t], FHN_PARAMS, float(Vtr[0, t, 0])), atol=1e-12)
    for kw in (dict(model="lorenz", input_dim=1), dict(model="fhn", input_dim=2)):
        with pytest.raises(ValueError, match="generated exogenous inputs"):
            generate_dataset(2, 2, 10, Dy=1, **kw)


def test_runner_dataset_hands_the_inputs_on(tmp_path):
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    argv = ["--noPSVO", "--AESMC", "--generateTrainingData", "--Dy=1", "--Dx=2", "--time=12", "--n_train=3", "--n_test=2"]
    np.random.seed(2)
    assert len(runner._dataset(parse_flags(argv))) == 4
    np.random.seed(2)
    data = runner._dataset(parse_flags(argv + ["--Di=1"]))
    assert len(data) == 6 and data[4].shape == (3, 12, 1) and data[5].shape == (2, 12, 1)
    with pytest.raises(ValueError, match="generated exogenous inputs"):
        runner._dataset(parse_flags(argv + ["--Di=2"]))
    rng = np.random.RandomState(1)
    arrays = dict(Ytrain=rng.randn(4, 8, 1), Yvalid=rng.randn(3, 8, 1), Vtrain=rng.randn(4, 8, 2), Vvalid=rng.randn(3, 8, 2))
    with open(tmp_path / "d.p", "wb") as fh:
        pickle.dump(arrays, fh)
    F = parse_flags(["--noPSVO", "--AESMC", "--Di=2", "--Dy=1", "--datadir=%s/" % tmp_path, "--datadict=d.p"])
    data = runner._dataset(F)
    assert len(data) == 6 and np.array_equal(data[5], arrays["Vvalid"]) and (F.n_train, F.n_test, F.time) == (4, 3, 8)
    F0 = parse_flags(["--noPSVO", "--AESMC", "--Dy=1", "--datadir=%s/" % tmp_path, "--datadict=d.p"])
    assert len(runner._dataset(F0)) == 4                                             # Di = 0 leaves the datadict as it is


# ---- the reference ----------------------------------------------------------------------------------------------------------
def _sliced(P, Dx):
    """the model's parameters with the first layers of q1 / f cut to their state rows: what the missing reference can run"""
    first = lambda p: {**p, "layers": [(p["layers"][0][0][:Dx].clone(), p["layers"][0][1])]}
    return {**P, "q1": first(P["q1"]), **({"f": first(P["f"])} if "f" in P else {})}


@pytest.mark.parametrize("run", [ER.RUNS[0], ER.RUNS[2], ER.RUNS[3], ER.RUNS[6], ER.RUNS[7]], ids=ER.run_id)
@pytest.mark.parametrize("how", ["zero-rows", "zero-inputs"])
def test_anchor_on_the_missing_reference(run, how):
    """with W1[Dx:] = 0, and separately with v = 0, the restated loop equals missing_reference's oracle on the same model,
    observations and noise, exactly in fp64"""
    obj, Dx = run[0][0], run[0][5]
    FLAGS, model, obs, v, noise = ER.cpu_setup(run, 3)
    if how == "zero-rows":
        with torch.no_grad():
            for tr in {model.q1_tran, model.f_tran}:
                tr.kernels[0][Dx:].zero_()
    else:
        v = torch.zeros_like(v)
    P = model.export_reference_layout(torch.float64)
    z, log = ER.run(model, FLAGS, obj, obs, v, noise, P=P)
    o = MR.objective(_sliced(P, Dx), FLAGS, obj)
    with torch.no_grad():
        z0, log0 = o.get_log_ZSMC(obs, MR._cast(noise, torch.float64))
    assert torch.equal(z, z0) and torch.isfinite(z)
    for key in ("X_prevs", "X_ancestors", "log_Ws", "Xs"):
        assert torch.equal(log[key], log0[key]), key
    assert (log["idx_f"] is None) == (log0["idx_f"] is None) and (log["idx_f"] is None or torch.equal(log["idx_f"], log0["idx_f"]))


@pytest.mark.parametrize("run", ER.RUNS, ids=ER.run_id)
def test_concat_and_hoisted_forms_agree(run):
    """concat[x, v] W1 + b1 and x W1[:Dx] + (b1 + v W1[Dx:]) agree to fp64 rounding (teacher-forced: one particle system)"""
    obj = run[0][0]
    FLAGS, model, obs, v, noise = ER.cpu_setup(run, 3)
    z, log = ER.run(model, FLAGS, obj, obs, v, noise)
    teacher = {"idx_f": log["idx_f"]} if log["idx_f"] is not None else {}
    z2, log2 = ER.run(model, FLAGS, obj, obs, v, noise, teacher=teacher, form="concat")
    scale = float(log["log_Ws"].abs().max())
    assert float((log["log_Ws"] - log2["log_Ws"]).abs().max()) <= 1e-11 * max(scale, 1.0)
    assert float((log["X_prevs"] - log2["X_prevs"]).abs().max()) <= 1e-12 * max(float(log["X_prevs"].abs().max()), 1.0)
    assert abs(float(z) - float(z2)) <= 1e-12 * abs(float(z))


@pytest.mark.parametrize("run", ER.RUNS, ids=ER.run_id)
def test_separation_condition(run):
    """in the reference alone, on every GPU case and both model seeds: rolling v by one step, swapping the two sequences' inputs
    (B = 2) and zeroing v each move logW by at least 100 x the value tolerance (max-abs), so a kernel that reads the wrong row,
    the wrong sequence or no row cannot pass"""
    obj, B = run[0][0], run[0][1]
    for seed in (3, 5):
        FLAGS, model, obs, v, noise = ER.cpu_setup(run, seed)
        _, ref = ER.run(model, FLAGS, obj, obs, v, noise)
        teacher = {"idx_f": ref["idx_f"]} if ref["idx_f"] is not None else {}
        moves = {"roll": torch.roll(v, 1, dims=1), "zero": torch.zeros_like(v)}
        if B == 2:
            moves["swap"] = v.flip(0)
        for name, w in moves.items():
            _, other = ER.run(model, FLAGS, obj, obs, w, noise, teacher=teacher)
            moved = float((other["log_Ws"] - ref["log_Ws"]).abs().max())
            print("%s seed %d %s: logW moves by %.3e" % (ER.run_id(run), seed, name, moved))
            assert moved >= 100 * LOGW_ATOL, (name, seed, moved)


def test_the_fp32_reference_backs_the_tolerances():
    """tools/exo_reference_error.py on the GPU runs: the fp32 reference's own error against fp64 is below a third of every
    tolerance (values, ELBO, gradients)"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("exo_reference_error", os.path.join(root, "tools", "exo_reference_error.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rows = tool.table()
    assert len(rows) == len(ER.RUNS)
    for r in rows:
        assert r["bound_share"] < 1 / 3, r                 # |fp32 - fp64| / (atol + rtol |fp64|), worst element of X, logW, lse
        assert r["elbo_rel"] < 1e-4 / 3 and r["elbo_abs_min"] >= 1.0, r
        assert r["grad_rel"] < 2e-3 / 3, r
