"""Host side of missing observations (FLAGS.missing_obs, FLAGS.missing_rate): flags, routing, refusals, the count check, the
masked R-square, the knock-out of generated data, and the fp64 reference of tests/missing_reference.py against itself.  No GPU."""
import math

import numpy as np
import pytest
import torch

from oracle import psvo_oracle as O
from tests import helpers as Hh
from tests import missing_reference as MR


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
    assert Flags().missing_obs is False and Flags().missing_rate == 0.0
    assert parse_flags([]).missing_obs is False and parse_flags([]).missing_rate == 0.0
    F = parse_flags(["--noPSVO", "--AESMC", "--missing_obs", "--missing_rate=0.3", "--generateTrainingData"])
    assert F.missing_obs is True and F.missing_rate == 0.3 and F.AESMC and F.generateTrainingData
    assert parse_flags(["--missing_obs", "--nomissing_obs"]).missing_obs is False
    assert parse_flags(["--missing_rate", "0.25"]).missing_rate == 0.25
    assert {"missing_obs", "missing_rate"} <= set(Flags().as_dict())


def test_routing():
    from psvo_amd import autograd, ops
    assert hasattr(autograd, "FilterWobsMissingFunction")
    assert hasattr(ops, "filter_forward_wobs_missing") and hasattr(ops, "filter_backward_wobs_missing")
    for obj in ("AESMC", "SVO", "IWAE"):
        for Dy in (1, 2, 3, 10, 32):
            FLAGS, model, smc = _objective(obj, Dy=Dy, Dx=3, missing_obs=True)
            assert smc.missing_obs is True and model.missing_obs is True and smc.wide_obs is False
        assert _objective(obj, Dy=10, Dx=3)[2].missing_obs is False                 # without the flag nothing changes
        assert _objective(obj, Dy=10, Dx=3)[2].wide_obs is True
    # every emission form, the widths of the plain kernels included
    for kw in (dict(poisson_emission=True), dict(count_emission=True)):
        for Dy in (1, 2, 5):
            assert _objective("AESMC", Dy=Dy, missing_obs=True, **kw)[2].missing_obs is True
    smc = _objective("AESMC", Dy=2, missing_obs=True, FFBS=True, FFBSi=True)[2]     # the smoothers stay available behind it
    assert smc.FFBS and smc.FFBSi and smc.missing_obs


@pytest.mark.parametrize("obj,kw,word", [
    ("PSVO", dict(Dy=1), r"--missing_obs with --PSVO / --PSVOwR.*evaluate the emission too"),
    ("PSVOwR", dict(Dy=1), r"--missing_obs with --PSVO / --PSVOwR"),
    ("PSVO", dict(Dy=10, Dx=3, BSim_wide_obs=True), r"--missing_obs with --PSVO / --PSVOwR"),
    ("AESMC", dict(Dy=1, resample_ess=0.5), r"--missing_obs with --resample_ess"),
    ("SVO", dict(Dy=10, Dx=3, resample_ess=0.5, resample_ess_wide_obs=True), r"--missing_obs with --resample_ess"),
    ("AESMC", dict(Dy=3, particle_forecast=True), r"--missing_obs with --particle_forecast.*lpd.*whole observation rows"),
    ("AESMC", dict(Dy=1, output_cov=True, diag_cov=True), r"--missing_obs with output_cov"),
    ("AESMC", dict(Dy=1, q1_layers="32,32", g_layers="32,32"), r"--missing_obs with per-particle MLP layers.*one hidden layer"),
    ("SVO", dict(Dy=10, Dx=3, g_layers="16,16"), r"--missing_obs with per-particle MLP layers.*one hidden layer"),
    ("AESMC", dict(Dy=33, Dx=3), r"--missing_obs with Dy = 33.*1 <= Dy <= 32"),
    ("AESMC", dict(Dy=1, missing_rate=1.0), r"--missing_rate = 1\.0.*\[0, 1\)"),
    ("AESMC", dict(Dy=1, missing_rate=-0.1), r"--missing_rate = -0\.1.*\[0, 1\)"),
], ids=["PSVO", "PSVOwR", "PSVO-wide", "resample_ess", "resample_ess-wide", "particle_forecast", "output_cov", "two-layers",
        "two-layers-g", "Dy33", "rate-1", "rate-negative"])
def test_refusals(obj, kw, word):
    with pytest.raises(ValueError, match=word):
        _objective(obj, missing_obs=True, **kw)


def test_missing_rate_without_the_flag():
    with pytest.raises(ValueError, match=r"--missing_rate without --missing_obs"):
        _objective("AESMC", Dy=1, missing_rate=0.3)
    with pytest.raises(ValueError, match=r"--missing_rate = nan"):
        _objective("AESMC", Dy=1, missing_obs=True, missing_rate=float("nan"))


def test_check_missing_obs_names_every_limit():
    """the check runner.main makes on the flags alone"""
    from psvo_amd.SMC.SVO import check_missing_obs
    ok = dict(Dy=10, layers=["32", "32"])
    assert check_missing_obs(True, **ok) is True and check_missing_obs(True, missing_rate=0.3, **ok) is True
    assert check_missing_obs(True, Dy=1, layers=[[64], [64]]) is True and check_missing_obs(True, Dy=32, layers=["16"]) is True
    # the flag off: nothing to refuse, whatever else is set
    assert check_missing_obs(False, backward_simulation=True, resample_ess=0.5, output_cov=True, Dy=40, layers=["32,32"]) is False
    for kw, word in ((dict(ok, backward_simulation=True), "--PSVO / --PSVOwR"),
                     (dict(ok, resample_ess=0.5), "--resample_ess"),
                     (dict(ok, particle_forecast=True), "--particle_forecast"),
                     (dict(ok, output_cov=True), "output_cov"),
                     (dict(ok, layers=["32", "32,32"]), r"per-particle MLP layers \[\[32, 32\]\].*one hidden layer"),
                     (dict(ok, Dy=33), r"Dy = 33.*1 <= Dy <= 32"),
                     (dict(ok, Dy=0), r"Dy = 0.*1 <= Dy <= 32"),
                     (dict(ok, missing_rate=1.5), r"--missing_rate = 1\.5")):
        with pytest.raises(ValueError, match=word):
            check_missing_obs(True, **kw)
    with pytest.raises(ValueError, match="--missing_rate without --missing_obs"):
        check_missing_obs(False, missing_rate=0.1)


def test_runner_refuses_before_it_touches_a_device(monkeypatch):
    """runner.main checks the flags first: no device, no data set, no model is reached"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags

    def unreachable(*a, **k):
        raise AssertionError("runner.main went on after a refusal")
    monkeypatch.setattr(runner, "_device", unreachable)
    monkeypatch.setattr(runner, "_dataset", unreachable)
    for argv, word in ((["--missing_obs"], "--PSVO / --PSVOwR"),                                  # (PSVO is the default objective)
                       (["--noPSVO", "--PSVOwR", "--missing_obs"], "--PSVO / --PSVOwR"),
                       (["--noPSVO", "--AESMC", "--missing_obs", "--resample_ess=0.5"], "--missing_obs with --resample_ess"),
                       (["--noPSVO", "--AESMC", "--missing_obs", "--particle_forecast"], "--particle_forecast"),
                       (["--noPSVO", "--AESMC", "--missing_obs", "--output_cov", "--diag_cov"], "output_cov"),
                       (["--noPSVO", "--AESMC", "--missing_obs", "--g_layers=32,32"], "one hidden layer"),
                       (["--noPSVO", "--AESMC", "--missing_obs", "--Dy=33"], "1 <= Dy <= 32"),
                       (["--noPSVO", "--AESMC", "--missing_obs", "--missing_rate=1"], r"\[0, 1\)"),
                       (["--noPSVO", "--AESMC", "--missing_rate=0.3"], "--missing_rate without --missing_obs")):
        with pytest.raises(ValueError, match=word):
            runner.main(parse_flags(argv))


def test_check_counts():
    from psvo_amd.runner import check_counts
    nan, inf = float("nan"), float("inf")
    ok = np.array([[0.0, 3.0], [nan, 7.0]])
    check_counts(ok, missing_obs=True)
    check_counts(np.full((2, 3), nan), missing_obs=True)                  # nothing observed: nothing to refuse
    with pytest.raises(ValueError, match=r"non-finite values \(first at index \(1, 0\)\)"):
        check_counts(ok)                                                  # without the flag a NaN is refused as before
    for bad, word in ((np.array([[0.0, inf], [nan, 1.0]]), r"non-finite values \(first at index \(0, 1\)\)"),
                      (np.array([[0.0, -inf], [nan, 1.0]]), r"non-finite values \(first at index \(0, 1\)\)"),
                      (np.array([[nan, 2.0], [-1.0, 1.0]]), r"negative values \(minimum -1\.0\)"),
                      (np.array([[nan, 2.0], [1.0, 1.5]]), r"non-integer values \(first: 1\.5 at index \(1, 1\)\)")):
        with pytest.raises(ValueError, match=word):
            check_counts(bad, missing_obs=True)
    for bad, word in ((np.array([1.0, inf]), "non-finite"), (np.array([1.0, -2.0]), "negative"), (np.array([0.5]), "non-integer")):
        with pytest.raises(ValueError, match=word):
            check_counts(bad)
    check_counts(np.array([0.0, 5.0]))


def test_masked_r_square_by_hand():
    """a 3 x 4 x 2 array (sequences, steps, outputs) with NaN targets against sums written out entry by entry"""
    from psvo_amd.trainer import _r_square
    rng = np.random.RandomState(3)
    y = rng.randn(3, 4, 2)
    y_hat = y + 0.3 * rng.randn(3, 4, 2)
    full = _r_square(y_hat, y)
    assert _r_square(y_hat, y, True) == pytest.approx(full, rel=1e-12)         # nothing missing: the reference's number
    assert full == 1.0 - np.square(y_hat - y).sum() / np.square(y - y.mean(axis=0, keepdims=True)).sum()
    y[0, 1, 0] = y[2, 1, 0] = y[1, 3, 1] = np.nan
    y[:, 2, 1] = np.nan                                                         # a (step, output) nobody observed
    res = tot = 0.0
    for t in range(4):
        for e in range(2):
            seen = [i for i in range(3) if not math.isnan(y[i, t, e])]
            if not seen:
                continue
            mean = sum(y[i, t, e] for i in seen) / len(seen)
            res += sum((y_hat[i, t, e] - y[i, t, e]) ** 2 for i in seen)
            tot += sum((y[i, t, e] - mean) ** 2 for i in seen)
    got = _r_square(y_hat, y, True)
    assert math.isfinite(got) and got == pytest.approx(1.0 - res / tot, rel=1e-12)
    assert math.isnan(_r_square(y_hat, y))                                      # the flag off: the function is unchanged


def test_missing_rate_knock_out():
    from psvo_amd.utils.data_generator import knock_out
    base = np.arange(64 * 50 * 3, dtype=float).reshape(64, 50, 3)
    np.random.seed(11)
    a = knock_out(base, 0.3)
    np.random.seed(11)
    b = knock_out(base, 0.3)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], base[~np.isnan(a)])
    np.random.seed(12)
    assert not np.array_equal(np.isnan(knock_out(base, 0.3)), np.isnan(a))
    state = np.random.get_state()[1].copy()
    z = knock_out(base, 0.0)
    assert not np.isnan(z).any() and np.array_equal(z, base) and np.array_equal(np.random.get_state()[1], state)
    assert not np.isnan(base).any()                                             # a copy: the input keeps its entries
    n, p = base.size, 0.3
    observed = float(np.mean(~np.isnan(a)))
    assert abs(observed - (1 - p)) <= 4.0 * math.sqrt(p * (1 - p) / n), observed


def test_runner_dataset_knocks_out_after_generation():
    """_dataset under --generateTrainingData --missing_obs --missing_rate: same seed, same data and mask; the observed entries
    are the entries of the run without knock-out"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    argv = ["--noPSVO", "--AESMC", "--generateTrainingData", "--time=20", "--n_train=6", "--n_test=4"]
    got = []
    for extra in (["--missing_obs", "--missing_rate=0.3"], ["--missing_obs", "--missing_rate=0.3"], ["--missing_obs"], []):
        np.random.seed(5)
        got.append(runner._dataset(parse_flags(argv + extra)))
    for k in range(4):
        assert np.array_equal(got[0][k], got[1][k], equal_nan=True)
    for k in (2, 3):
        miss = np.isnan(got[0][k])
        assert 0.1 < miss.mean() < 0.5 and got[0][k].shape == got[2][k].shape
        assert np.array_equal(got[0][k][~miss], got[2][k][~miss])
        assert not np.isnan(got[2][k]).any() and np.array_equal(got[2][k], got[3][k])
    # count data: NaN passes the count check with the flag and is refused without it
    cnt = argv + ["--Dy=3", "--count_emission"]
    np.random.seed(5)
    data = runner._dataset(parse_flags(cnt + ["--missing_obs", "--missing_rate=0.3"]))
    assert np.isnan(data[2]).any() and (data[2][~np.isnan(data[2])] >= 0).all()


# ---- the reference against itself, fp64 --------------------------------------------------------------------------------------

def _reference_case(Dy=4, count=False, seed=2):
    B, T, N, Dx = 2, 5, 8, 2
    FLAGS = Hh.make_flags("AESMC", Dx=Dx, Dy=Dy, n_particles=N, count_emission=count)
    of = dict(Hh.oracle_flags(FLAGS, "AESMC"), layers=[16])
    P = O.make_params(of, seed=seed, bias_scale=0.3)
    g = torch.Generator().manual_seed(40 + seed)
    for name in P:          # distinct scales per output
        if isinstance(P[name], dict) and "sigma_raw" in P[name]:
            P[name]["sigma_raw"] = P[name]["sigma_raw"] + torch.randn(P[name]["sigma_raw"].shape, generator=g, dtype=torch.float64)
    obs = (torch.poisson(4.0 * torch.rand(B, T, Dy, generator=g, dtype=torch.float64), generator=g) if count
           else torch.randn(B, T, Dy, generator=g, dtype=torch.float64) * 1.5)
    noise = O.make_noise(of, B, T, seed=77 + seed)
    return FLAGS, P, obs, noise


def _clone(P):
    if torch.is_tensor(P):
        return P.detach().clone()
    if isinstance(P, dict):
        return {k: _clone(v) for k, v in P.items()}
    if isinstance(P, (list, tuple)):
        return type(P)(_clone(v) for v in P)
    return P


def _without_output(P, e):
    """the parameters of the model with observation output e removed: its column of g's output layer and scale, and its row of
    every first layer that reads the observations (q0 and q2 under AESMC's wiring)"""
    keep = [i for i in range(P["g"]["mu"][1].shape[0]) if i != e]
    Q = _clone(P)
    Q["g"]["mu"] = (Q["g"]["mu"][0][:, keep].clone(), Q["g"]["mu"][1][keep].clone())
    Q["g"]["sigma_raw"] = Q["g"]["sigma_raw"][keep].clone()
    for name in ("q0", "q2"):
        W, b = Q[name]["layers"][0]
        Q[name]["layers"][0] = (W[keep].clone(), b)
    return Q, keep


@pytest.mark.parametrize("count", [False, True], ids=["gaussian", "count"])
def test_reference_never_observed_output_is_the_model_without_it(count):
    Dy, e = 4, 1
    FLAGS, P, obs, noise = _reference_case(Dy, count)
    miss = torch.rand(obs.shape, generator=torch.Generator().manual_seed(9)) < 0.3
    miss[:, :, e] = True
    full = MR.knock_out(obs, miss)
    Pf = MR.require_grad(_clone(P))
    of = MR.objective(Pf, FLAGS, "AESMC")
    z_f, log_f = of.get_log_ZSMC(full, noise)
    z_f.backward()
    Q, keep = _without_output(P, e)
    Q = MR.require_grad(Q)
    FLAGS_r = Hh.make_flags("AESMC", Dx=FLAGS.Dx, Dy=Dy - 1, n_particles=FLAGS.n_particles, count_emission=count)
    orr = MR.objective(Q, FLAGS_r, "AESMC")
    z_r, log_r = orr.get_log_ZSMC(full[:, :, keep], {**noise, "idx_f": log_f["idx_f"]})
    z_r.backward()
    assert torch.equal(log_f["idx_f"], log_r["idx_f"])
    assert float((log_f["log_Ws"] - log_r["log_Ws"]).detach().abs().max()) <= 1e-10
    assert abs(float(z_f.detach()) - float(z_r.detach())) <= 1e-10
    # the removed output: exactly zero gradients
    assert torch.equal(Pf["g"]["mu"][0].grad[:, e], torch.zeros(16, dtype=torch.float64))
    assert float(Pf["g"]["mu"][1].grad[e]) == 0.0
    if not count:
        assert float(Pf["g"]["sigma_raw"].grad[e]) == 0.0
        assert float((Pf["g"]["sigma_raw"].grad[keep] - Q["g"]["sigma_raw"].grad).abs().max()) <= 1e-10
        assert float(Q["g"]["sigma_raw"].grad.abs().min()) > 0
    # every other parameter: the gradients of the smaller model
    assert float((Pf["g"]["mu"][0].grad[:, keep] - Q["g"]["mu"][0].grad).abs().max()) <= 1e-10
    assert float((Pf["g"]["mu"][1].grad[keep] - Q["g"]["mu"][1].grad).abs().max()) <= 1e-10
    assert float(Q["g"]["mu"][0].grad.abs().max()) > 0
    for name in ("q0", "q2"):
        assert float((Pf[name]["layers"][0][0].grad[keep] - Q[name]["layers"][0][0].grad).abs().max()) <= 1e-10
        assert float(Pf[name]["layers"][0][0].grad[e].abs().max()) == 0.0           # (its input is the imputed zero)
    checked = 0
    for name in ("q0", "q1", "q2", "g"):
        pairs = [(Pf[name]["layers"][0][1], Q[name]["layers"][0][1]), (Pf[name]["sigma_raw"], Q[name]["sigma_raw"])]
        if name != "g":
            pairs += [(Pf[name]["mu"][0], Q[name]["mu"][0]), (Pf[name]["mu"][1], Q[name]["mu"][1])]
        else:
            pairs = pairs[:1] + [(Pf[name]["layers"][0][0], Q[name]["layers"][0][0])]
        if name == "q1":
            pairs.append((Pf[name]["layers"][0][0], Q[name]["layers"][0][0]))
        for a, b in pairs:
            ga = torch.zeros_like(a) if a.grad is None else a.grad
            gb = torch.zeros_like(b) if b.grad is None else b.grad
            assert float((ga - gb).abs().max()) <= 1e-10, name
            checked += 1
    assert checked >= 12


@pytest.mark.parametrize("obj", ["AESMC", "SVO", "IWAE"])
def test_reference_all_observed_is_the_unmodified_oracle(obj):
    B, T, N, Dx, Dy = 2, 5, 8, 2, 3
    FLAGS = Hh.make_flags(obj, Dx=Dx, Dy=Dy, n_particles=N)
    of = dict(Hh.oracle_flags(FLAGS, obj), layers=[16], y_smoother_Dhs=[8], X0_smoother_Dhs=[8])
    P = O.make_params(of, seed=4, bias_scale=0.3)
    g = torch.Generator().manual_seed(44)
    obs = torch.randn(B, T, Dy, generator=g, dtype=torch.float64) * 1.5
    noise = O.make_noise(of, B, T, seed=81)
    with torch.no_grad():
        z0, log0 = O.OBJECTIVES[obj](P, Hh.oracle_flags(FLAGS, obj)).get_log_ZSMC(obs, noise)
        z1, log1 = MR.objective(P, FLAGS, obj).get_log_ZSMC(obs, noise)
    assert float((log0["log_Ws"] - log1["log_Ws"]).abs().max()) <= 1e-12
    assert float((log0["X_prevs"] - log1["X_prevs"]).abs().max()) <= 1e-12
    assert abs(float(z0) - float(z1)) <= 1e-12
    if log0["idx_f"] is not None:
        assert torch.equal(log0["idx_f"], log1["idx_f"])


def test_reference_nothing_observed_has_no_emission_term():
    """every entry NaN: the weights are the transition over the proposal, finite, and no gradient reaches the output layer"""
    FLAGS, P, obs, noise = _reference_case(3)
    Pf = MR.require_grad(_clone(P))
    z, log = MR.objective(Pf, FLAGS, "AESMC").get_log_ZSMC(torch.full_like(obs, float("nan")), noise)
    z.backward()
    assert torch.isfinite(z) and torch.isfinite(log["log_Ws"]).all()
    assert float(Pf["g"]["mu"][0].grad.abs().max()) == 0.0 and float(Pf["g"]["sigma_raw"].grad.abs().max()) == 0.0
    assert float(Pf["q1"]["mu"][0].grad.abs().max()) > 0 and torch.isfinite(Pf["q1"]["mu"][0].grad).all()


def test_mask_pattern():
    """the mask of the GPU tests is what tests/missing_reference.py says it is, on every shape they use"""
    for B, T, Dy in ((2, 5, 1), (2, 6, 2), (2, 5, 3), (2, 6, 10), (2, 5, 17), (1, 4, 32), (1, 60, 10)):
        for seed in (3, 5):
            miss, t_all, e_never = MR.mask(B, T, Dy, seed)
            again = MR.mask(B, T, Dy, seed)[0]
            assert torch.equal(miss, again) and miss.shape == (B, T, Dy)
            assert bool(miss[:, t_all].all()) and 1 <= t_all < T
            assert (e_never is None) == (Dy == 1)
            if e_never is not None:
                assert bool(miss[:, :, e_never].all())
            if B == 2:
                assert bool(miss[1, T - 2:].all()) and t_all < T - 2
            rest = [e for e in range(Dy) if e != e_never]
            assert not bool(miss[0, 0, rest].any())
