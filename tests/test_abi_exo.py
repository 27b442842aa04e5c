"""C ABI of exogenous inputs (include/psvo_hip.h: psvo_filter_forward_wobs_input / psvo_filter_backward_wobs_input,
psvo_mlp_wgrad_rowbias) as far as it can be checked without a GPU: the symbols are exported and bound with the missing-observation
pair's argument lists plus hb_q1 / hb_f, and every refusal of the contract comes back as a status before anything is launched."""
import ctypes

import pytest

from tests.test_abi_missing import BWD as MISSING_BWD
from tests.test_abi_missing import FWD as MISSING_FWD

FWD = MISSING_FWD[:-1] + ("hb_q1", "hb_f", "stream")
BWD = MISSING_BWD[:-1] + ("hb_q1", "hb_f", "stream")
FWD_NAME, BWD_NAME = "psvo_filter_forward_wobs_input", "psvo_filter_backward_wobs_input"


def test_symbols_are_exported_and_bound(built_lib):
    from psvo_amd import _lib
    so = ctypes.CDLL(built_lib)
    P = ctypes.c_void_p
    for name, base in ((FWD_NAME, "psvo_filter_forward_wobs_missing"), (BWD_NAME, "psvo_filter_backward_wobs_missing")):
        assert hasattr(so, name), name
        want = _lib.SIGNATURES[base]
        assert _lib.SIGNATURES[name] == (want[0], want[1][:-1] + [P, P] + want[1][-1:]), name     # ... then hb_q1, hb_f, stream
        assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name][1]
    for name in ("psvo_mlp_wgrad_rowbias", "psvo_mlp_wgrad_rowbias_blocks"):
        assert hasattr(so, name) and name in _lib.SIGNATURES, name
    plain = _lib.SIGNATURES["psvo_mlp_wgrad"][1]
    assert _lib.SIGNATURES["psvo_mlp_wgrad_rowbias"][1] == plain[:7] + [P] + plain[7:10] + [P] + plain[10:]      # + hb, + dhb
    assert _lib.load().psvo_abi_version() == 6        # (added within ABI 6: nothing existing changed)
    blocks = _lib.load().psvo_mlp_wgrad_rowbias_blocks
    assert blocks(1) == 1 and blocks(32) == 1 and blocks(33) == 2 and blocks(10 ** 9) == 1024


def test_the_header_declares_them():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "psvo_hip.h")).read()
    for name in (FWD_NAME, BWD_NAME):
        assert ("int %s(const psvo_desc* desc," % name) in text, name
    assert "int psvo_mlp_wgrad_rowbias(long long S, int L, int Din, int H, int Dout," in text
    assert "int psvo_mlp_wgrad_rowbias_blocks(long long S);" in text
    for words in ("x_{t+1} ~ f(. | x_t, v_t)", "ONE fp32 add", "hb[t,b,:] = v[b,t,:] W1[Dx:]"):
        assert words in text, words


@pytest.fixture
def host_only():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-code test: never hands a host pointer to a library that can reach a device")


def _call(lib, _lib, name, desc_kw=None, **kw):
    """tests/test_abi_missing._call for the input pair: every pointer set, Dx = 5 OUTSIDE the envelope, so that a call which
    passes every check ends in the shape dispatch's PSVO_ERR_UNSUPPORTED and nothing is ever launched"""
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    d = _lib.psvo_desc()
    d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = 2, 4, 8, 1, 5, 10, 32
    d.resample, d.two_q, d.bootstrap, d.emission, d.layers = 1, 1, 0, 0, 1
    for k, v in (desc_kw or {}).items():
        setattr(d, k, v)
    mlps = []
    for _ in range(3):
        m = _lib.psvo_mlp()
        m.W1 = m.b1 = m.W2 = m.b2 = P.value
        mlps.append(m)
    names = {FWD_NAME: FWD, BWD_NAME: BWD}[name]
    a = {k: P for k in names}
    a.update(desc=ctypes.byref(d), q1=ctypes.byref(mlps[0]), f=ctypes.byref(mlps[1]), g=ctypes.byref(mlps[2]), stream=None)
    a.update(kw)
    st = getattr(lib, name)(*[a[k] for k in names])
    assert all(x == 0.0 for x in buf), "a refused call wrote to its buffers"
    return st


@pytest.mark.parametrize("name", [FWD_NAME, BWD_NAME])
def test_a_complete_call_reaches_the_shape_dispatch(built_lib, host_only, name):
    from psvo_amd import _lib
    lib = _lib.load()
    assert _call(lib, _lib, name) == _lib.PSVO_ERR_UNSUPPORTED                           # (Dx = 5: see _call)
    for kw in (dict(emission=1), dict(emission=2), dict(bootstrap=1), dict(two_q=0), dict(resample=0), dict(Dy=1), dict(Dy=32),
               dict(T=2), dict(N=512), dict(Dx=2, H=48), dict(Dx=1), dict(Dx=2, H=8), dict(Dx=4, H=128)):
        assert _call(lib, _lib, name, desc_kw=kw) == _lib.PSVO_ERR_UNSUPPORTED, kw
    # hb_f is ignored under bootstrap, required otherwise; hb_q1 always
    assert _call(lib, _lib, name, desc_kw=dict(bootstrap=1), hb_f=None) == _lib.PSVO_ERR_UNSUPPORTED
    assert _call(lib, _lib, name, hb_f=None) == _lib.PSVO_ERR_INVALID
    for boot in (0, 1):
        assert _call(lib, _lib, name, desc_kw=dict(bootstrap=boot), hb_q1=None) == _lib.PSVO_ERR_INVALID
    if name == BWD_NAME:
        assert _call(lib, _lib, name, dlse=None) == _lib.PSVO_ERR_UNSUPPORTED            # dlse is optional (NULL = 0)


@pytest.mark.parametrize("name", [FWD_NAME, BWD_NAME])
def test_refusals(built_lib, host_only, name):
    from psvo_amd import _lib
    lib = _lib.load()
    # outside the envelope (inside Dx / H, so that the shape dispatch is not what answers)
    for kw in (dict(Dy=0), dict(Dy=33), dict(layers=2), dict(N=513), dict(emission=3), dict(Dy=-1), dict(emission=-1)):
        assert _call(lib, _lib, name, desc_kw=dict(Dx=2, **kw)) == _lib.PSVO_ERR_UNSUPPORTED, kw
    # a missing required pointer, a size that is none
    assert _call(lib, _lib, name, desc_kw=dict(Dx=2), obs=None) == _lib.PSVO_ERR_INVALID
    for T in (1, 0, -3):
        assert _call(lib, _lib, name, desc_kw=dict(Dx=2, T=T)) == _lib.PSVO_ERR_INVALID, T
    for kw in (dict(B=0), dict(N=0)):
        assert _call(lib, _lib, name, desc_kw=dict(Dx=2, **kw)) == _lib.PSVO_ERR_INVALID, kw
    more = (dict(desc=None), dict(X=None), dict(lse=None), dict(eps=None), dict(sig_g=None), dict(f=None), dict(mu2=None))
    more += (dict(u=None, idx_in=None),) if name == FWD_NAME else (dict(dG=None), dict(ws=None), dict(idx=None), dict(P1=None))
    for kw in more:
        assert _call(lib, _lib, name, **kw) == _lib.PSVO_ERR_INVALID, kw
    with pytest.raises(ValueError):
        _lib.check(_call(lib, _lib, name, obs=None), name)


def test_rowbias_refusals(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    m = _lib.psvo_mlp()
    m.W1 = m.b1 = m.W2 = m.b2 = P.value
    M = ctypes.byref(m)
    fn = lib.psvo_mlp_wgrad_rowbias
    # (S, L, Din, H, Dout, X, dOut, hb, w, partial, grad, dhb, accumulate, stream)
    for H in (8, 48, 128, 0):
        assert fn(8, 4, 2, H, 2, P, P, P, M, P, P, P, 0, None) == _lib.PSVO_ERR_UNSUPPORTED, H
    for Din, Dout in ((5, 2), (0, 2), (2, 5), (2, 0)):
        assert fn(8, 4, Din, 32, Dout, P, P, P, M, P, P, P, 0, None) == _lib.PSVO_ERR_UNSUPPORTED, (Din, Dout)
    for i in (5, 6, 7, 8, 9, 10, 11):      # X, dOut, hb, w, partial, grad, dhb
        args = [8, 4, 2, 32, 2, P, P, P, M, P, P, P, 0, None]
        args[i] = None
        assert fn(*args) == _lib.PSVO_ERR_INVALID, i
    for S, L in ((0, 4), (8, 0), (-1, 4)):
        assert fn(S, L, 2, 32, 2, P, P, P, M, P, P, P, 0, None) == _lib.PSVO_ERR_INVALID, (S, L)
    assert all(x == 0.0 for x in buf)
