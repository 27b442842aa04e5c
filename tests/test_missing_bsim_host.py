"""Host side of PSVO on missing observations (FLAGS.missing_obs with FLAGS.BSim_missing_obs): the flag, routing, refusals, and the
fp64 reference of tests/missing_bsim_reference.py against the unmodified oracle.  No GPU."""
import pytest
import torch

from oracle import psvo_oracle as O
from tests import helpers as Hh
from tests import missing_bsim_reference as MB
from tests.test_missing_host import _clone, _objective

ON = dict(missing_obs=True, BSim_missing_obs=True)


def test_flag_parsing_and_default():
    from psvo_amd.flags import Flags, parse_flags
    assert Flags().BSim_missing_obs is False and parse_flags([]).BSim_missing_obs is False
    F = parse_flags(["--missing_obs", "--BSim_missing_obs"])
    assert F.PSVO and F.missing_obs is True and F.BSim_missing_obs is True
    assert parse_flags(["--BSim_missing_obs", "--noBSim_missing_obs"]).BSim_missing_obs is False
    assert "BSim_missing_obs" in Flags().as_dict()


def test_routing():
    from psvo_amd import autograd, ops
    for name in ("BsimWobsMissingFunction", "FilterWobsMissingBsimFunction"):
        assert hasattr(autograd, name), name
    for name in ("bsim_forward_wobs_missing", "bsim_backward_wobs_missing"):
        assert hasattr(ops, name), name
    # every width, the widths of the plain kernels included; --BSim_wide_obs is not needed
    for Dy in (1, 2, 3, 10, 32):
        FLAGS, model, smc = _objective("PSVO", Dy=Dy, Dx=3, **ON)
        assert smc.missing_obs is True and model.missing_obs is True and smc.wide_obs is True
        assert smc.uses_backward_simulation and smc.resample_ess == 0.0
    # every emission form, separate f, no q2, the forward-only encoder
    for kw in (dict(poisson_emission=True), dict(count_emission=True)):
        for Dy in (1, 2, 5):
            assert _objective("PSVO", Dy=Dy, **ON, **kw)[2].missing_obs is True
    for kw in (dict(use_bootstrap=False), dict(use_2_q=False), dict(BSim_use_single_RNN=True), dict(BSim_wide_obs=True, Dy=10, Dx=3)):
        smc = _objective("PSVO", **{"Dy": 2, **ON, **kw})[2]
        assert smc.missing_obs and smc.wide_obs
    # the forecast on gappy data stays available behind it
    smc = _objective("PSVO", Dy=3, particle_forecast=True, particle_forecast_missing_obs=True, **ON)[2]
    assert smc.forecast and smc.forecast_missing


def test_the_flag_has_no_effect_without_missing_obs():
    for obj, kw in (("PSVO", dict(Dy=1)), ("PSVO", dict(Dy=2)), ("PSVO", dict(Dy=10, Dx=3, BSim_wide_obs=True)),
                    ("AESMC", dict(Dy=1)), ("SVO", dict(Dy=10, Dx=3)), ("PSVOwR", dict(Dy=2))):
        a = _objective(obj, **kw)[2]
        b = _objective(obj, BSim_missing_obs=True, **kw)[2]
        assert a.missing_obs is b.missing_obs is False and a.wide_obs == b.wide_obs, (obj, kw)
    # ... and the wide refusal of PSVO stays, with or without it
    for kw in (dict(), dict(BSim_missing_obs=True)):
        with pytest.raises(ValueError, match=r"Dy = 3 with PSVO / PSVOwR.*Dy <= 2"):
            _objective("PSVO", Dy=3, **kw)
    # a filter objective with --missing_obs takes its own route whatever the flag says
    for kw in (dict(), dict(BSim_missing_obs=True)):
        smc = _objective("AESMC", Dy=3, missing_obs=True, **kw)[2]
        assert smc.missing_obs is True and smc.wide_obs is False


UNFLAGGED = ("--missing_obs with --PSVO / --PSVOwR: missing observations run on psvo_filter_forward_wobs_missing, the filter of "
             "SVO / AESMC / IWAE; the backward-simulation kernels evaluate the emission too and have no missing-observation form")


def test_the_unflagged_refusal_is_word_for_word():
    from psvo_amd.SMC.SVO import check_missing_obs
    for obj in ("PSVO", "PSVOwR"):
        with pytest.raises(ValueError) as e:
            _objective(obj, Dy=1, missing_obs=True)
        assert str(e.value) == UNFLAGGED
    with pytest.raises(ValueError) as e:
        check_missing_obs(True, backward_simulation=True, Dy=10, layers=["32", "32"])
    assert str(e.value) == UNFLAGGED


@pytest.mark.parametrize("obj,kw,word", [
    ("PSVOwR", dict(Dy=1), r"--BSim_missing_obs with --PSVOwR.*covers PSVO only"),
    ("PSVOwR", dict(Dy=10, Dx=3, BSim_wide_obs=True), r"--BSim_missing_obs with --PSVOwR.*covers PSVO only"),
    ("PSVO", dict(Dy=1, output_cov=True, diag_cov=True), r"--missing_obs with output_cov.*state-independent scales"),
    ("PSVO", dict(Dy=1, q1_layers="32,32", g_layers="32,32"), r"--missing_obs with per-particle MLP layers.*one hidden layer"),
    ("PSVO", dict(Dy=3, g_layers="16,16"), r"--missing_obs with per-particle MLP layers.*one hidden layer"),
    ("PSVO", dict(Dy=2, use_bootstrap=False, f_layers="32,32"), r"--missing_obs with per-particle MLP layers.*one hidden layer"),
    ("PSVO", dict(Dy=33, Dx=3), r"--missing_obs with Dy = 33.*1 <= Dy <= 32"),
    ("PSVO", dict(Dy=1, resample_ess=0.5), r"--resample_ess.*PSVO"),
    ("PSVO", dict(Dy=1, resample_ess=0.5, resample_ess_missing_obs=True), r"--resample_ess.*PSVO"),
    ("PSVO", dict(Dy=3, particle_forecast=True), r"--missing_obs with --particle_forecast.*lpd.*whole observation rows"),
    ("PSVO", dict(Dy=1, missing_rate=1.0), r"--missing_rate = 1\.0.*\[0, 1\)"),
], ids=["PSVOwR", "PSVOwR-wide", "output_cov", "two-layers", "two-layers-g", "two-layers-f", "Dy33", "resample_ess",
        "resample_ess-missing", "particle_forecast", "rate"])
def test_refusals(obj, kw, word):
    with pytest.raises(ValueError, match=word):
        _objective(obj, **ON, **kw)


def test_check_missing_obs_names_every_limit():
    """the check runner.main makes on the flags alone"""
    from psvo_amd.SMC.SVO import check_missing_obs
    ok = dict(Dy=10, layers=["32", "32"], backward_simulation=True, bsim_missing_obs=True)
    assert check_missing_obs(True, **ok) is True and check_missing_obs(True, missing_rate=0.3, **ok) is True
    assert check_missing_obs(True, **dict(ok, Dy=1)) is True and check_missing_obs(True, **dict(ok, Dy=32)) is True
    # the flag off: nothing to refuse, whatever else is set; a filter objective: the flag changes nothing
    assert check_missing_obs(False, cross_chain=True, resample_ess=0.5, **ok) is False
    assert check_missing_obs(True, Dy=10, layers=["32"], bsim_missing_obs=True) is True
    for kw, word in ((dict(ok, bsim_missing_obs=False), "--PSVO / --PSVOwR"),
                     (dict(ok, cross_chain=True), "PSVOwR"),
                     (dict(ok, resample_ess=0.5, resample_ess_missing_obs=True), r"--resample_ess under --PSVO"),
                     (dict(ok, particle_forecast=True), "--particle_forecast"),
                     (dict(ok, output_cov=True), "output_cov"),
                     (dict(ok, layers=["32", "32,32"]), r"per-particle MLP layers \[\[32, 32\]\].*one hidden layer"),
                     (dict(ok, Dy=33), r"Dy = 33.*1 <= Dy <= 32"),
                     (dict(ok, Dy=0), r"Dy = 0.*1 <= Dy <= 32")):
        with pytest.raises(ValueError, match=word):
            check_missing_obs(True, **kw)


def test_runner_refuses_before_it_touches_a_device(monkeypatch):
    """runner.main checks the flags first: no device, no data set, no model is reached -- and lets PSVO through with the flag"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags

    class Reached(Exception):
        pass

    def unreachable(*a, **k):
        raise AssertionError("runner.main went on after a refusal")

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(runner, "_device", unreachable)
    monkeypatch.setattr(runner, "_dataset", unreachable)
    on = ["--missing_obs", "--BSim_missing_obs"]
    for argv, word in ((["--missing_obs"], "--PSVO / --PSVOwR"),                                  # (PSVO is the default objective)
                       (["--noPSVO", "--PSVOwR"] + on, "--BSim_missing_obs with --PSVOwR"),
                       (on + ["--resample_ess=0.5"], "--resample_ess with --PSVO"),
                       (on + ["--output_cov", "--diag_cov"], "output_cov"),
                       (on + ["--g_layers=32,32"], "one hidden layer"),
                       (on + ["--Dy=33"], "1 <= Dy <= 32"),
                       (on + ["--particle_forecast"], "--particle_forecast"),
                       (on + ["--missing_rate=1"], r"\[0, 1\)")):
        with pytest.raises(ValueError, match=word):
            runner.main(parse_flags(argv))
    monkeypatch.setattr(runner, "_device", reached)
    for argv in (on, on + ["--Dy=1"], on + ["--Dy=10", "--Dx=3"], on + ["--count_emission", "--Dy=2"],
                 on + ["--particle_forecast", "--particle_forecast_missing_obs"], on + ["--missing_rate=0.3"]):
        with pytest.raises(Reached):
            runner.main(parse_flags(argv))


# ---- the reference against the unmodified oracle, fp64 -------------------------------------------------------------------------

def _psvo_case(extra=None, seed=4, Dy=3):
    B, T, N, Dx = 2, 5, 8, 2
    FLAGS = Hh.make_flags("PSVO", Dx=Dx, Dy=Dy, n_particles=N, n_particles_for_BSim_proposal=4, **(extra or {}))
    of = dict(Hh.oracle_flags(FLAGS, "PSVO"), layers=[16], y_smoother_Dhs=[8], X0_smoother_Dhs=[8])
    P = O.make_params(of, seed=seed, bias_scale=0.3)
    g = torch.Generator().manual_seed(40 + seed)
    obs = torch.randn(B, T, Dy, generator=g, dtype=torch.float64) * 1.5
    noise = O.make_noise(of, B, T, seed=81 + seed)
    return FLAGS, P, obs, noise


def _leaves(P, out=None, path=""):
    out = {} if out is None else out
    if torch.is_tensor(P):
        out[path] = P
    elif isinstance(P, dict):
        [_leaves(v, out, path + "/" + str(k)) for k, v in P.items()]
    elif isinstance(P, (list, tuple)):
        [_leaves(v, out, path + "/" + str(i)) for i, v in enumerate(P)]
    return out


@pytest.mark.parametrize("extra", [dict(), dict(use_bootstrap=False), dict(BSim_use_single_RNN=True), dict(poisson_emission=True)],
                         ids=["default", "separate-f", "single-RNN", "poisson"])
def test_reference_all_observed_is_the_unmodified_oracle(extra):
    """with every entry observed the reference reproduces the unmodified oracle's PSVO: every value bit for bit (the forward
    arithmetic is the oracle's, operation for operation), every gradient to fp64 rounding.  The gradients cannot be asked bit for
    bit: MissingEmission's selects are nodes of their own in the autograd graph, so a parameter's gradient is the same terms
    added in another order.  Bound: a gradient entry sums at most T N M B Dy = 5 * 8 * 4 * 2 * 3 = 960 terms, each rounded once
    per operation on a path of a few dozen operations; 960 * 50 * 2^-53 = 5.3e-12 of the tensor's largest entry would cover the
    worst case, random signs give its square root -- the test asks 1e-12 (measured on the four wirings: 0, 3.0e-16, 1.4e-16, 0)."""
    FLAGS, P, obs, noise = _psvo_case(extra)
    P0, P1 = MB.require_grad(_clone(P)), MB.require_grad(_clone(P))
    z0, log0 = O.OBJECTIVES["PSVO"](P0, Hh.oracle_flags(FLAGS, "PSVO")).get_log_ZSMC(obs, noise)
    z1, log1 = MB.objective(P1, FLAGS).get_log_ZSMC(obs, noise)
    z0.backward()
    z1.backward()
    assert torch.equal(z0.detach(), z1.detach())
    assert torch.equal(log0["idx_f"], log1["idx_f"]) and torch.equal(log0["idx_b"], log1["idx_b"])
    for key in ("log_Ws", "X_prevs", "bw_Xs", "f_log_probs", "g_log_probs", "bw_log_Omegas"):
        assert torch.equal(log0[key].detach(), log1[key].detach()), key
    l0, l1 = _leaves(P0), _leaves(P1)
    assert l0.keys() == l1.keys()
    seen, worst = 0, 0.0
    for k in l0:
        if l0[k].grad is None:
            assert l1[k].grad is None, k
            continue
        e, s = float((l0[k].grad - l1[k].grad).abs().max()), float(l0[k].grad.abs().max())
        worst = max(worst, e / max(s, 1e-300))
        assert e <= 1e-12 * s, (k, e, s)
        seen += 1
    print("worst gradient difference / largest entry: %.3e" % worst)
    assert seen > 20


def test_reference_zero_fills_every_proposal_side_reader():
    """what the backward simulation's proposal reads -- the encoder behind BSim_q2 and BSim_q_init -- sees the zero-filled
    observations: the value under the mask is finite, a never-observed output's column of g's output layer and its scale get
    exactly zero gradient, and the row of the encoder's input weights that reads it gets none either"""
    Dy = 4
    FLAGS, P, obs, noise = _psvo_case(Dy=Dy)
    miss, t_all, e_never = MB.mask(2, 5, Dy, 3)
    full = MB.knock_out(obs, miss)
    Pf = MB.require_grad(_clone(P))
    o = MB.objective(Pf, FLAGS)
    seen = []
    inner = o.BS_preprocess_obs
    o.BS_preprocess_obs = lambda y: (seen.append(y), inner(y))[1]
    z, log = o.get_log_ZSMC(full, noise)
    z.backward()
    assert len(seen) == 1 and bool(torch.isnan(seen[0]).any())          # (the NaN reaches the wrapper, which fills it)
    assert torch.isfinite(z) and all(torch.isfinite(log[k]).all() for k in ("bw_Xs", "g_log_probs", "bw_log_Omegas", "log_Ws"))
    assert bool((log["g_log_probs"][t_all] == 0.0).all())               # a step with nothing observed: log g = 0 exactly
    assert torch.equal(Pf["g"]["mu"][0].grad[:, e_never], torch.zeros(16, dtype=torch.float64))
    assert float(Pf["g"]["mu"][1].grad[e_never]) == 0.0 and float(Pf["g"]["sigma_raw"].grad[e_never]) == 0.0
    others = [e for e in range(Dy) if e != e_never]
    assert float(Pf["g"]["mu"][1].grad[others].abs().min()) > 0
    for name, p in _leaves(Pf).items():
        assert p.grad is None or torch.isfinite(p.grad).all(), name
    for name in ("BSim_q2", "BSim_q_init", "q1_inv"):
        assert float(Pf[name]["mu"][0].grad.abs().max()) > 0, name
