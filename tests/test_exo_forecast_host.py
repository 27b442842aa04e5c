"""Host side of the particle forecast under exogenous inputs (--Di with --particle_forecast --particle_forecast_inputs;
psvo_particle_forecast_input): the flag and the refusals it lifts, the C ABI as far as it can be checked without a GPU, and the
reference of tests/exo_forecast_reference.py against forecast_reference and against itself -- the inputs of the GPU cases matter.
No GPU."""
import ctypes

import pytest
import torch

from tests import exo_forecast_reference as XR
from tests import forecast_reference as R
from tests import helpers as Hh
from tests.test_gpu_forecast import K_TOL

REFUSAL = ("--Di with --particle_forecast: the forecast kernel (psvo_particle_forecast) propagates the cloud through an autonomous "
           "f; it has no input form")


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def test_zero_rows_are_the_missing_form_of_forecast_reference():
    """hb_f = 0: the moments of forecast_reference.forecast to the last bit of fp64 (b1 + 0 is b1), lpd equal where nothing is
    missing up to the grouping of the Gaussian constants"""
    for name in ("four-origins", "three-waves", "count-eight-waves"):
        c = XR.case(name)
        zero = XR.run(c, torch.float64, hb_f=torch.zeros_like(c["hb_f"]))
        plain = R.run(c, torch.float64)
        for k in ("ymean", "yvar", "xmean"):
            assert torch.equal(zero[k], plain[k]), (name, k)
        assert torch.allclose(zero["lpd"], plain["lpd"], rtol=1e-12, atol=1e-12), name


@pytest.mark.parametrize("name", list(XR.CASES))
def test_the_inputs_matter(name):
    """on every GPU case, zeroing hb_f and rolling it by one step each move ymean at some horizon k >= 1 by at least 100 times that
    case's tolerance bound: a kernel that ignored the rows, or met them one step early or late, cannot pass"""
    c = XR.case(name)
    bound = XR.bound(c, "ymean", K_TOL["ymean"])
    ref = c["ref64"]["ymean"]
    for what, hb in (("zeroed", torch.zeros_like(c["hb_f"])), ("rolled", torch.roll(c["hb_f"], 1, 0))):
        moved = (XR.run(c, torch.float64, hb_f=hb)["ymean"] - ref).abs()
        assert float(moved[0].max()) == 0.0                     # horizon 0 is the cloud itself
        print("exo-forecast-separation %s %s moved %.3e bound %.3e ratio %.1f"
              % (name, what, float(moved[1:].max()), bound, float(moved[1:].max()) / bound))
        assert float(moved[1:].max()) >= 100 * bound, (name, what)


def test_rows_past_tv_are_zero_input():
    """a Tv-row hb_f is the T + K rows with zeros behind it, and rows T .. Tv-1 are read: cutting them changes the forecast"""
    c = XR.case("count-eight-waves")
    T, B, Dx, Dy, H, N, K, _ = c["shape"]
    padded = torch.cat([c["hb_f"], torch.zeros(T + K - c["Tv"], B, H)])
    a, b = XR.run(c, torch.float64), XR.run(c, torch.float64, hb_f=padded)
    for k in XR.KEYS:
        assert torch.equal(a[k], b[k]), k
    cut = XR.run(c, torch.float64, hb_f=c["hb_f"][:T])
    assert not torch.equal(cut["ymean"], a["ymean"])
    # origin t meets row t + k: the last origin at horizon 1 has used row T - 1 only, which the cut keeps
    assert torch.equal(cut["ymean"][1], a["ymean"][1]) and not torch.equal(cut["ymean"][2, T - 1], a["ymean"][2, T - 1])


# ---- the flag and the refusals -----------------------------------------------------------------------------------------------------
def _objective(obj, **kw):
    from psvo_amd.model import SSM
    from psvo_amd.SMC.AESMC import AESMC
    from psvo_amd.SMC.IWAE import IWAE
    from psvo_amd.SMC.PSVO import PSVO
    from psvo_amd.SMC.SVO import SVO
    FLAGS = Hh.make_flags(obj, **kw)
    model = SSM(FLAGS)
    return FLAGS, model, {"AESMC": AESMC, "IWAE": IWAE, "PSVO": PSVO, "SVO": SVO}[obj](model, FLAGS)


def test_flag_parsing_and_default():
    from psvo_amd.flags import Flags, parse_flags
    assert Flags().particle_forecast_inputs is False and parse_flags([]).particle_forecast_inputs is False
    assert parse_flags(["--particle_forecast_inputs"]).particle_forecast_inputs is True
    assert "particle_forecast_inputs" in Flags().as_dict()


def test_check_inputs_with_and_without_the_flag():
    from psvo_amd.SMC.SVO import check_inputs
    ok = dict(Dy=10, layers=["32", "32"])
    with pytest.raises(ValueError) as e:
        check_inputs(1, particle_forecast=True, **ok)
    assert str(e.value) == REFUSAL                             # word for word
    with pytest.raises(ValueError) as e:
        check_inputs(1, particle_forecast=True, particle_forecast_inputs=False, **ok)
    assert str(e.value) == REFUSAL
    assert check_inputs(1, particle_forecast=True, particle_forecast_inputs=True, **ok) == 1
    # no effect without the forecast, and none at Di = 0
    assert check_inputs(2, particle_forecast_inputs=True, **ok) == 2
    assert check_inputs(0, particle_forecast=True, particle_forecast_inputs=True) == 0
    # the flag lifts this refusal alone
    for kw, word in ((dict(backward_simulation=True), "--PSVO / --PSVOwR"), (dict(resample_ess=0.5), "--Di with --resample_ess"),
                     (dict(output_cov=True), "output_cov"), (dict(Dy=33), "1 <= Dy <= 32"),
                     (dict(layers=["32,32"]), "one hidden layer")):
        with pytest.raises(ValueError, match=word):
            check_inputs(1, **{**ok, "particle_forecast": True, "particle_forecast_inputs": True, **kw})


def test_objectives_route_the_flag():
    with pytest.raises(ValueError) as e:
        _objective("AESMC", Di=1, particle_forecast=True)
    assert str(e.value) == REFUSAL
    for obj in ("AESMC", "SVO", "IWAE"):
        FLAGS, model, smc = _objective(obj, Di=2, Dx=3, Dy=4, particle_forecast=True, particle_forecast_inputs=True)
        assert smc.Di == 2 and smc.forecast is True and smc.forecast_missing is False
    # PSVO stays refused; without inputs the flag changes nothing
    with pytest.raises(ValueError, match=r"--Di with --PSVO / --PSVOwR"):
        _objective("PSVO", Di=1, particle_forecast=True, particle_forecast_inputs=True)
    FLAGS, model, smc = _objective("AESMC", particle_forecast=True, particle_forecast_inputs=True)
    assert smc.Di == 0 and smc.forecast is True
    # gappy data beside it: its own flag is still required
    with pytest.raises(ValueError, match="--missing_obs with --particle_forecast"):
        _objective("AESMC", Di=1, missing_obs=True, particle_forecast=True, particle_forecast_inputs=True)
    smc = _objective("AESMC", Di=1, missing_obs=True, particle_forecast=True, particle_forecast_inputs=True,
                     particle_forecast_missing_obs=True)[2]
    assert smc.forecast_missing is True and smc.Di == 1


def test_runner_refuses_before_it_touches_a_device(monkeypatch):
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags

    def unreachable(*a, **k):
        raise AssertionError("runner.main went on after a refusal")
    monkeypatch.setattr(runner, "_device", unreachable)
    monkeypatch.setattr(runner, "_dataset", unreachable)
    with pytest.raises(ValueError) as e:
        runner.main(parse_flags(["--noPSVO", "--AESMC", "--Di=1", "--particle_forecast"]))
    assert str(e.value) == REFUSAL
    # with the flag the checks pass and the run goes on to the device
    with pytest.raises(AssertionError, match="went on"):
        runner.main(parse_flags(["--noPSVO", "--AESMC", "--Di=1", "--particle_forecast", "--particle_forecast_inputs"]))
    with pytest.raises(ValueError, match="--PSVO / --PSVOwR"):
        runner.main(parse_flags(["--Di=1", "--particle_forecast", "--particle_forecast_inputs"]))


def test_particle_forecast_checks_its_inputs():
    """the argument checks of SVO.particle_forecast come ahead of anything that needs a device"""
    B, T, N, Dx, Di = 2, 5, 8, 2, 3
    hidden, obs = torch.zeros(B, T, N, Dx), torch.zeros(B, T, 1)
    smc = _objective("AESMC", Di=Di, Dx=Dx, particle_forecast=True, particle_forecast_inputs=True)[2]
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"--Di = 3: the model's transitions are driven by an input; pass inputs"):
            smc.particle_forecast(2, hidden, obs)
        for bad in ((B, T - 1, Di), (B, T, Di + 1), (B + 1, T, Di), (B, T)):
            with pytest.raises(ValueError, match=r"particle_forecast inputs must be \(batch, Tv, Di\)"):
                smc.particle_forecast(2, hidden, obs, inputs=torch.zeros(*bad))
        plain = _objective("AESMC", Dx=Dx, particle_forecast=True)[2]
        with pytest.raises(ValueError, match=r"inputs given to a model without an input channel \(--Di = 0\)"):
            plain.particle_forecast(2, hidden, obs, inputs=torch.zeros(B, T, Di))
    with pytest.raises(ValueError, match="no gradient"):
        smc.particle_forecast(2, hidden, obs, inputs=torch.zeros(B, T, Di))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
ARGS = ("desc", "K", "f", "g", "sig_f", "sig_g", "X", "logW", "obs", "eps", "ymean", "yvar", "xmean", "lpd", "hb_f", "Tv", "stream")


def test_symbol_is_exported_and_bound(built_lib):
    from psvo_amd import _lib
    assert hasattr(ctypes.CDLL(built_lib), "psvo_particle_forecast_input")
    res, args = _lib.SIGNATURES["psvo_particle_forecast_input"]
    assert res is ctypes.c_int and len(args) == len(ARGS)
    base = _lib.SIGNATURES["psvo_particle_forecast_missing"][1]
    assert args[:14] == base[:14] and args[14] is ctypes.c_void_p and args[15] is ctypes.c_int and args[16] is ctypes.c_void_p
    assert _lib.load().psvo_particle_forecast_input.argtypes == args
    assert _lib.load().psvo_abi_version() == 6        # (added within ABI 6: nothing existing changed)


def _call(lib, _lib, entry="psvo_particle_forecast_input", desc_kw=None, **kw):
    """the entry with every argument valid (one small host buffer behind every pointer) except what `desc_kw` / `kw` replace.
    Only for calls that return before a launch."""
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p(ctypes.addressof(buf))
    d = _lib.psvo_desc()
    d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = 2, 4, 8, 1, 2, 1, 32
    d.resample, d.two_q, d.bootstrap, d.emission, d.layers = 1, 1, 1, 0, 1
    for k, v in (desc_kw or {}).items():
        setattr(d, k, v)
    f, g = _lib.psvo_mlp(), _lib.psvo_mlp()
    for m in (f, g):
        m.W1 = m.b1 = m.W2 = m.b2 = ctypes.addressof(buf)
    a = dict(desc=ctypes.byref(d), K=3, f=ctypes.byref(f), g=ctypes.byref(g), sig_f=P, sig_g=P, X=P, logW=P, obs=P, eps=P,
             ymean=P, yvar=P, xmean=P, lpd=P, hb_f=P, Tv=4, stream=None)
    a.update(kw)
    names = ARGS if entry.endswith("_input") else tuple(n for n in ARGS if n not in ("hb_f", "Tv"))
    st = getattr(lib, entry)(*[a[k] for k in names])
    assert all(x == 0.0 for x in buf), "a refused call wrote to its buffers"
    return st


@pytest.fixture
def host_only():
    if torch.cuda.is_available():
        pytest.skip("host-code test: never hands a host pointer to a library that can reach a device")


def test_null_rows_and_short_tv_are_invalid(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    for kw in (dict(hb_f=None), dict(Tv=3), dict(Tv=0), dict(Tv=-1), dict(hb_f=None, Tv=9)):
        assert _call(lib, _lib, **kw) == _lib.PSVO_ERR_INVALID, kw
    # ... whatever the shape, as every invalid argument is
    assert _call(lib, _lib, desc_kw=dict(Dx=5), hb_f=None) == _lib.PSVO_ERR_INVALID
    assert _call(lib, _lib, desc_kw=dict(N=600), Tv=3) == _lib.PSVO_ERR_INVALID
    # the base form's own refusals
    for kw in (dict(desc=None), dict(f=None), dict(X=None), dict(obs=None), dict(sig_f=None), dict(K=-1),
               dict(ymean=None, yvar=None, xmean=None, lpd=None)):
        assert _call(lib, _lib, **kw) == _lib.PSVO_ERR_INVALID, kw
    with pytest.raises(ValueError):
        _lib.check(_call(lib, _lib, hb_f=None), "psvo_particle_forecast_input")


def test_unsupported_exactly_where_the_missing_form_says_so(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    edges = (dict(Dx=1), dict(Dx=5), dict(Dy=0), dict(Dy=33), dict(H=8), dict(H=48), dict(H=128), dict(N=513), dict(emission=3),
             dict(emission=-1), dict(layers=2), dict(layers=3), dict(T=1 << 20, B=1 << 12), dict(M=3, resample=7, Dx=7))
    for kw in edges:
        tv = dict(Tv=kw["T"]) if "T" in kw else {}
        assert _call(lib, _lib, entry="psvo_particle_forecast_missing", desc_kw=kw) == _lib.PSVO_ERR_UNSUPPORTED, kw
        assert _call(lib, _lib, desc_kw=kw, **tv) == _lib.PSVO_ERR_UNSUPPORTED, kw


def test_op_takes_the_rows():
    """ops.particle_forecast(..., hb_f=...) exists; its shape errors come ahead of the launch (checked on the GPU)"""
    import inspect
    from psvo_amd import ops
    from psvo_amd.SMC.SVO import SVO
    assert inspect.signature(ops.particle_forecast).parameters["hb_f"].default is None
    assert inspect.signature(SVO.particle_forecast).parameters["inputs"].default is None
