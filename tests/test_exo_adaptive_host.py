"""Host side of adaptive resampling under exogenous inputs (--Di with --resample_ess --resample_ess_inputs;
psvo_filter_forward_wobs_input_adaptive / psvo_filter_backward_wobs_input_adaptive): the flag and the refusals it lifts, the C ABI
as far as it can be checked without a GPU, and the reference of tests/exo_adaptive_reference.py against the two it composes.
No GPU."""
import ctypes

import pytest
import torch

from tests import adaptive_reference as AR
from tests import exo_adaptive_reference as XA
from tests import exo_reference as ER
from tests import helpers as Hh

REFUSAL = ("--Di with --resample_ess: exogenous inputs run on psvo_filter_forward_wobs_input, the filter of SVO / AESMC / IWAE, "
           "which resamples at every step (or never); the adaptive kernels have no input form")


def _objective(obj, **kw):
    from psvo_amd.model import SSM
    from psvo_amd.SMC.AESMC import AESMC
    from psvo_amd.SMC.IWAE import IWAE
    from psvo_amd.SMC.PSVO import PSVO
    from psvo_amd.SMC.SVO import SVO
    FLAGS = Hh.make_flags(obj, **kw)
    model = SSM(FLAGS)
    return FLAGS, model, {"AESMC": AESMC, "IWAE": IWAE, "PSVO": PSVO, "SVO": SVO}[obj](model, FLAGS)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", XA.RUNS[:3], ids=XA.run_id)
def test_the_two_ends_are_exo_reference(run):
    """every decision forced to `resample`: exo_reference.smc as it stands, to the last bit of fp64; every decision forced to
    `keep`: the same loop with resample_particles off (the draw is still made and returned)"""
    obj, B, T = run[0][0], run[0][1], run[0][2]
    FLAGS, model, obs, v, noise = ER.cpu_setup(run, 3)
    z0, ref0 = ER.run(model, FLAGS, obj, obs, v, noise)
    z1, ref1 = XA.run(model, FLAGS, obj, obs, v, noise, teacher={"rs_f": torch.ones(T, B, dtype=torch.int64)})
    assert torch.equal(z0, z1)
    for k in ("X_prevs", "X_ancestors", "log_Ws", "idx_f"):
        assert torch.equal(ref0[k], ref1[k]), k
    assert bool(ref1["rs_f"].all())
    o = ER.objective(model.export_reference_layout(torch.float64), FLAGS, obj)
    o.resample_particles = False
    with torch.no_grad():
        zk, refk = ER.smc(o, obs.double(), v.double(), noise)
    z2, ref2 = XA.run(model, FLAGS, obj, obs, v, noise, teacher={"rs_f": torch.zeros(T, B, dtype=torch.int64)})
    assert torch.equal(zk, z2) and torch.equal(refk["X_prevs"], ref2["X_prevs"]) and torch.equal(refk["log_Ws"], ref2["log_Ws"])
    assert not torch.equal(z0, z2)


@pytest.mark.parametrize("run", XA.RUNS, ids=XA.run_id)
def test_forced_pattern_is_mixed_and_matters(run):
    """the pattern of the forced-decision GPU tests holds a kept and a resampled step in every sequence, differs from what the
    rule decides, and changes the ELBO; the inputs matter under it"""
    obj, B, T = run[0][0], run[0][1], run[0][2]
    rs = XA.forced(T, B)
    assert rs.shape == (T, B) and rs.dtype == torch.int32
    for b in range(B):
        assert bool((rs[:, b] == 1).any()) and bool((rs[:, b] == 0).any()), b
    if T > 20:          # (the long case: one CPU pass of it is enough for the GPU tests to share)
        return
    FLAGS, model, obs, v, noise = ER.cpu_setup(run, 3)
    z_free, free = XA.run(model, FLAGS, obj, obs, v, noise)
    z_f, ref = XA.run(model, FLAGS, obj, obs, v, noise, teacher={"rs_f": rs.long()})
    assert torch.equal(ref["rs_f"], rs != 0) and not torch.equal(free["rs_f"], rs != 0)
    assert torch.equal(ref["ess"][0], free["ess"][0]) and not torch.equal(z_f, z_free)
    z_0, _ = XA.run(model, FLAGS, obj, obs, torch.zeros_like(v), noise, teacher={"rs_f": rs.long()})
    assert abs(float(z_0) - float(z_f)) > 1e-3 * abs(float(z_f))


def test_rule_is_adaptive_reference():
    run = XA.RUNS[0]
    obj, B, T, N = run[0][:4]
    FLAGS, model, obs, v, noise = ER.cpu_setup(run, 3)
    _, ref = XA.run(model, FLAGS, obj, obs, v, noise, ess_frac=0.5)
    for t in range(T):
        ess = AR.ess_of(ref["log_Ws"][t])
        assert torch.allclose(ess, ref["ess"][t]) and torch.equal(AR.decide(ess, 0.5, N), ref["rs_f"][t])
    assert float(ref["ess"].min()) >= 1.0 - 1e-9 and float(ref["ess"].max()) <= N + 1e-9


# ---- the flag and the refusals -----------------------------------------------------------------------------------------------------
def test_flag_parsing_and_default():
    from psvo_amd.flags import Flags, parse_flags
    assert Flags().resample_ess_inputs is False and parse_flags([]).resample_ess_inputs is False
    assert parse_flags(["--resample_ess_inputs"]).resample_ess_inputs is True
    assert "resample_ess_inputs" in Flags().as_dict()


def test_check_inputs_with_and_without_the_flag():
    from psvo_amd.SMC.SVO import check_inputs, check_resample_ess
    ok = dict(Dy=10, layers=["32", "32"])
    for kw in ({}, dict(resample_ess_inputs=False), dict(particle_forecast_inputs=True)):
        with pytest.raises(ValueError) as e:
            check_inputs(1, resample_ess=0.5, **ok, **kw)
        assert str(e.value) == REFUSAL                         # word for word
    assert check_inputs(1, resample_ess=0.5, resample_ess_inputs=True, **ok) == 1
    assert check_inputs(3, resample_ess_inputs=True, **ok) == 3 and check_inputs(0, resample_ess=0.5, resample_ess_inputs=True) == 0
    for kw, word in ((dict(backward_simulation=True), "--PSVO / --PSVOwR"), (dict(particle_forecast=True), "--Di with --particle_forecast"),
                     (dict(output_cov=True), "output_cov"), (dict(Dy=33), "1 <= Dy <= 32"), (dict(layers=["32,32"]), "one hidden layer")):
        with pytest.raises(ValueError, match=word):
            check_inputs(1, **{**ok, "resample_ess": 0.5, "resample_ess_inputs": True, **kw})
    # the threshold's own check: every width without --resample_ess_wide_obs, every other refusal as it was
    assert check_resample_ess(0.5, Dy=10, inputs=True) == 0.5 and check_resample_ess(0.0, Dy=10, inputs=True) == 0.0
    with pytest.raises(ValueError, match=r"--resample_ess with Dy = 10: without --resample_ess_wide_obs"):
        check_resample_ess(0.5, Dy=10)
    with pytest.raises(ValueError, match="--resample_ess with --IWAE"):
        check_resample_ess(0.5, never_resamples=True, inputs=True)
    with pytest.raises(ValueError, match="--resample_ess with --PSVO / --PSVOwR"):
        check_resample_ess(0.5, backward_simulation=True, inputs=True)
    with pytest.raises(ValueError, match="0 < tau <= 1"):
        check_resample_ess(1.5, inputs=True)


def test_objectives_route_the_flag():
    with pytest.raises(ValueError) as e:
        _objective("AESMC", Di=1, resample_ess=0.5)
    assert str(e.value) == REFUSAL
    for obj in ("AESMC", "SVO"):
        for kw in (dict(Dy=1), dict(Dy=10, Dx=3), dict(Dy=5, count_emission=True), dict(Dy=2, poisson_emission=True),
                   dict(Dy=3, use_bootstrap=False)):
            smc = _objective(obj, Di=2, resample_ess=0.25, resample_ess_inputs=True, **kw)[2]
            assert smc.Di == 2 and smc.resample_ess == 0.25 and smc.wide_obs is False
    with pytest.raises(ValueError, match="--resample_ess with --IWAE"):
        _objective("IWAE", Di=1, resample_ess=0.5, resample_ess_inputs=True)
    with pytest.raises(ValueError, match=r"--Di with --PSVO / --PSVOwR"):
        _objective("PSVO", Di=1, resample_ess=0.5, resample_ess_inputs=True)
    # no effect without inputs: the adaptive routes as they were
    with pytest.raises(ValueError, match="without --resample_ess_wide_obs"):
        _objective("AESMC", Dy=10, Dx=3, resample_ess=0.5, resample_ess_inputs=True)
    assert _objective("AESMC", resample_ess=0.5, resample_ess_inputs=True)[2].Di == 0
    # gappy data beside it: its own flag is still required
    with pytest.raises(ValueError, match="--missing_obs with --resample_ess"):
        _objective("AESMC", Di=1, missing_obs=True, resample_ess=0.5, resample_ess_inputs=True)
    smc = _objective("AESMC", Di=1, missing_obs=True, resample_ess=0.5, resample_ess_inputs=True, resample_ess_missing_obs=True)[2]
    assert smc.Di == 1 and smc.missing_obs and smc.resample_ess == 0.5


def test_runner_refuses_before_it_touches_a_device(monkeypatch):
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags

    def unreachable(*a, **k):
        raise AssertionError("runner.main went on after a refusal")
    monkeypatch.setattr(runner, "_device", unreachable)
    monkeypatch.setattr(runner, "_dataset", unreachable)
    with pytest.raises(ValueError) as e:
        runner.main(parse_flags(["--noPSVO", "--AESMC", "--Di=1", "--resample_ess=0.5"]))
    assert str(e.value) == REFUSAL
    for extra in ([], ["--Dy=10", "--Dx=3"]):
        with pytest.raises(AssertionError, match="went on"):
            runner.main(parse_flags(["--noPSVO", "--AESMC", "--Di=1", "--resample_ess=0.5", "--resample_ess_inputs"] + extra))
    with pytest.raises(ValueError, match="--resample_ess with --IWAE"):
        runner.main(parse_flags(["--noPSVO", "--IWAE", "--Di=1", "--resample_ess=0.5", "--resample_ess_inputs"]))
    with pytest.raises(ValueError, match="--PSVO / --PSVOwR"):
        runner.main(parse_flags(["--Di=1", "--resample_ess=0.5", "--resample_ess_inputs"]))


def test_routing_names():
    from psvo_amd import autograd, ops
    assert hasattr(autograd, "FilterWobsInputAdaptiveFunction")
    for name in ("filter_forward_wobs_input_adaptive", "filter_backward_wobs_input_adaptive"):
        assert hasattr(ops, name), name


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound(built_lib):
    from psvo_amd import _lib
    lib = ctypes.CDLL(built_lib)
    P = ctypes.c_void_p
    for name, twin, extra in (("psvo_filter_forward_wobs_input_adaptive", "psvo_filter_forward_wobs_adaptive", [P, P]),
                              ("psvo_filter_backward_wobs_input_adaptive", "psvo_filter_backward_wobs_adaptive", [P, P])):
        assert hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        base = _lib.SIGNATURES[twin][1]
        assert res is ctypes.c_int and args == base[:-1] + extra + base[-1:]          # the rows sit ahead of the stream
        assert getattr(_lib.load(), name).argtypes == args
    assert _lib.load().psvo_abi_version() == 6


@pytest.fixture
def host_only():
    if torch.cuda.is_available():
        pytest.skip("host-code test: never hands a host pointer to a library that can reach a device")


def _fwd(lib, _lib, desc_kw=None, **kw):
    """psvo_filter_forward_wobs_input_adaptive with every argument valid except what `desc_kw` / `kw` replace (calls that return
    before a launch only)"""
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p(ctypes.addressof(buf))
    d = _lib.psvo_desc()
    d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = 2, 4, 8, 1, 2, 1, 32
    d.resample, d.two_q, d.bootstrap, d.emission, d.layers = 1, 1, 0, 0, 1
    for k, v in (desc_kw or {}).items():
        setattr(d, k, v)
    mlps = [_lib.psvo_mlp() for _ in range(3)]
    for m in mlps:
        m.W1 = m.b1 = m.W2 = m.b2 = ctypes.addressof(buf)
    names = ("sig_q1", "sig_q2", "sig_f", "sig_g", "mu2", "m0", "sig0", "fm0", "fsig0", "obs", "eps", "u", "idx_in", "X", "Xanc",
             "Fm", "P1", "logW", "idx_out", "lse")
    a = {n: P for n in names}
    a.update(ess_frac=ctypes.c_float(0.5), rs_in=None, rs_out=P, ess_out=P, hb_q1=P, hb_f=P)
    a.update(kw)
    st = lib.psvo_filter_forward_wobs_input_adaptive(ctypes.byref(d), *[ctypes.byref(m) for m in mlps], *[a[n] for n in names],
                                                     a["ess_frac"], a["rs_in"], a["rs_out"], a["ess_out"], a["hb_q1"], a["hb_f"], None)
    assert all(x == 0.0 for x in buf), "a refused call wrote to its buffers"
    return st


def test_forward_refusals_come_before_any_launch(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    for kw in (dict(ess_frac=ctypes.c_float(0.0)), dict(ess_frac=ctypes.c_float(float("nan"))), dict(rs_out=None),
               dict(ess_out=None), dict(hb_q1=None), dict(hb_f=None), dict(obs=None), dict(lse=None), dict(u=None, idx_in=None)):
        assert _fwd(lib, _lib, **kw) == _lib.PSVO_ERR_INVALID, kw
    for kw in (dict(resample=0), dict(T=1), dict(B=0), dict(N=0)):
        assert _fwd(lib, _lib, desc_kw=kw) == _lib.PSVO_ERR_INVALID, kw
    # (under bootstrap hb_f is not required: the refusal then comes from the shape alone)
    assert _fwd(lib, _lib, desc_kw=dict(bootstrap=1, Dx=5), hb_f=None) == _lib.PSVO_ERR_UNSUPPORTED
    for kw in (dict(Dy=0), dict(Dy=33), dict(Dx=5), dict(H=48), dict(N=513), dict(layers=2), dict(emission=3)):
        assert _fwd(lib, _lib, desc_kw=kw) == _lib.PSVO_ERR_UNSUPPORTED, kw
