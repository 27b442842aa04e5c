"""C ABI of adaptive resampling and the particle forecast on missing observations (include/psvo_hip.h:
psvo_filter_forward_wobs_missing_adaptive / psvo_filter_backward_wobs_missing_adaptive / psvo_particle_forecast_missing) as far as it
can be checked without a GPU: the symbols are exported and bound with the adaptive wide pair's and psvo_particle_forecast's
argument lists, and every refusal of the contract comes back as a status before anything is launched."""
import ctypes

import pytest

FWD = ("desc", "q1", "f", "g", "sig_q1", "sig_q2", "sig_f", "sig_g", "mu2", "m0", "sig0", "fm0", "fsig0", "obs", "eps", "u",
       "idx_in", "X", "Xanc", "Fm", "P1", "logW", "idx_out", "lse", "ess_frac", "rs_in", "rs_out", "ess_out", "stream")
BWD = ("desc", "q1", "f", "g", "sig_q1", "sig_q2", "sig_f", "sig_g", "mu2", "m0", "sig0", "fm0", "fsig0", "obs", "eps", "X", "Fm",
       "P1", "logW", "lse", "idx", "dlse", "dP", "dF", "dG", "dmu2", "dm0", "dfm0", "dsig_q1", "dsig_q2", "dsig_f", "dsig_g",
       "dsig0", "dfsig0", "ws", "rs", "stream")
FC = ("desc", "K", "f", "g", "sig_f", "sig_g", "X", "logW", "obs", "eps", "ymean", "yvar", "xmean", "lpd", "stream")
FWD_NAME, BWD_NAME = "psvo_filter_forward_wobs_missing_adaptive", "psvo_filter_backward_wobs_missing_adaptive"
FC_NAME = "psvo_particle_forecast_missing"
NAMES = {FWD_NAME: FWD, BWD_NAME: BWD, FC_NAME: FC}


def test_symbols_are_exported_and_bound(built_lib):
    from psvo_amd import _lib
    so = ctypes.CDLL(built_lib)
    D, M, P = ctypes.POINTER(_lib.psvo_desc), ctypes.POINTER(_lib.psvo_mlp), ctypes.c_void_p
    twins = {FWD_NAME: "psvo_filter_forward_wobs_adaptive", BWD_NAME: "psvo_filter_backward_wobs_adaptive",
             FC_NAME: "psvo_particle_forecast"}
    for name, twin in twins.items():
        want = _lib.SIGNATURES[twin]
        assert hasattr(so, name), name
        assert _lib.SIGNATURES[name] == want and len(want[1]) == len(NAMES[name]), name     # the twin's argument list
        assert getattr(_lib.load(), name).argtypes == want[1]
    assert _lib.load().psvo_abi_version() == 6        # (added within ABI 6: nothing existing changed)
    assert _lib.SIGNATURES[FWD_NAME][1] == [D, M, M, M] + [P] * 20 + [ctypes.c_float, P, P, P, P]
    assert _lib.SIGNATURES[BWD_NAME][1] == [D, M, M, M] + [P] * 33
    assert _lib.SIGNATURES[FC_NAME][1] == [D, ctypes.c_int, M, M] + [P] * 11


def test_the_header_declares_them():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "psvo_hip.h")).read()
    for name in (FWD_NAME, BWD_NAME):
        assert ("int %s(const psvo_desc* desc," % name) in text, name
    assert ("int %s(const psvo_desc* desc, int K," % FC_NAME) in text


@pytest.fixture
def host_only():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-code test: never hands a host pointer to a library that can reach a device")


def _call(lib, _lib, name, desc_kw=None, **kw):
    """the entry point with every pointer set (one small host buffer behind each), except what `desc_kw` / `kw` replace.  The
    descriptor's Dx = 5 lies OUTSIDE the envelope, so a call that passes every check ends in the shape dispatch's
    PSVO_ERR_UNSUPPORTED: nothing is ever launched."""
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
    names = NAMES[name]
    a = {k: P for k in names}
    a.update(desc=ctypes.byref(d), q1=ctypes.byref(mlps[0]), f=ctypes.byref(mlps[1]), g=ctypes.byref(mlps[2]), stream=None,
             ess_frac=ctypes.c_float(0.5), K=3)
    a.update(kw)
    st = getattr(lib, name)(*[a[k] for k in names])
    assert all(x == 0.0 for x in buf), "a refused call wrote to its buffers"
    return st


def test_a_complete_call_reaches_the_shape_dispatch(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    for name in (FWD_NAME, BWD_NAME):
        assert _call(lib, _lib, name) == _lib.PSVO_ERR_UNSUPPORTED, name                    # (Dx = 5: see _call)
        for kw in (dict(emission=1), dict(emission=2), dict(bootstrap=1), dict(two_q=0), dict(Dy=1), dict(Dy=2),
                   dict(Dy=3), dict(Dy=32), dict(T=2), dict(N=512)):
            assert _call(lib, _lib, name, desc_kw=kw) == _lib.PSVO_ERR_UNSUPPORTED, (name, kw)
    assert _call(lib, _lib, BWD_NAME, dlse=None) == _lib.PSVO_ERR_UNSUPPORTED               # dlse is optional (NULL = 0)
    assert _call(lib, _lib, FWD_NAME, rs_in=None) == _lib.PSVO_ERR_UNSUPPORTED              # free running
    assert _call(lib, _lib, FWD_NAME, ess_frac=ctypes.c_float(1.0)) == _lib.PSVO_ERR_UNSUPPORTED
    for kw in (dict(), dict(emission=1), dict(emission=2), dict(Dy=1), dict(Dy=32), dict(T=1), dict(N=512)):
        assert _call(lib, _lib, FC_NAME, desc_kw=kw) == _lib.PSVO_ERR_UNSUPPORTED, kw
    assert _call(lib, _lib, FC_NAME, K=0, eps=None, logW=None) == _lib.PSVO_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", [FWD_NAME, BWD_NAME])
def test_refusals(built_lib, host_only, name):
    from psvo_amd import _lib
    lib = _lib.load()
    # the adaptive contract, ahead of everything else (here: ahead of an envelope violation, which would answer UNSUPPORTED)
    bad = dict(Dx=2, Dy=33)
    assert _call(lib, _lib, name, desc_kw=dict(resample=0, **bad)) == _lib.PSVO_ERR_INVALID
    if name == FWD_NAME:
        for v in (0.0, -0.5, float("nan")):
            assert _call(lib, _lib, name, desc_kw=bad, ess_frac=ctypes.c_float(v)) == _lib.PSVO_ERR_INVALID, v
        for kw in (dict(rs_out=None), dict(ess_out=None)):
            assert _call(lib, _lib, name, desc_kw=bad, **kw) == _lib.PSVO_ERR_INVALID, kw
    else:
        assert _call(lib, _lib, name, desc_kw=bad, rs=None) == _lib.PSVO_ERR_INVALID
    assert _call(lib, _lib, name, desc=None) == _lib.PSVO_ERR_INVALID
    # outside the envelope (inside Dx / H, so that the shape dispatch is not what answers)
    for kw in (dict(Dy=0), dict(Dy=33), dict(layers=2), dict(N=513), dict(emission=3), dict(Dy=-1), dict(emission=-1)):
        assert _call(lib, _lib, name, desc_kw=dict(Dx=2, **kw)) == _lib.PSVO_ERR_UNSUPPORTED, kw
    # a missing required pointer, a size that is none
    assert _call(lib, _lib, name, obs=None) == _lib.PSVO_ERR_INVALID
    assert _call(lib, _lib, name, desc_kw=dict(Dx=2), obs=None) == _lib.PSVO_ERR_INVALID
    for T in (1, 0, -3):
        assert _call(lib, _lib, name, desc_kw=dict(Dx=2, T=T)) == _lib.PSVO_ERR_INVALID, T
    for kw in (dict(B=0), dict(N=0)):
        assert _call(lib, _lib, name, desc_kw=dict(Dx=2, **kw)) == _lib.PSVO_ERR_INVALID, kw
    more = (dict(X=None), dict(lse=None), dict(eps=None), dict(sig_g=None))
    more += (dict(u=None, idx_in=None),) if name == FWD_NAME else (dict(dG=None), dict(ws=None), dict(idx=None))
    for kw in more:
        assert _call(lib, _lib, name, **kw) == _lib.PSVO_ERR_INVALID, kw
    with pytest.raises(ValueError):
        _lib.check(_call(lib, _lib, name, obs=None), name)


def test_forecast_refusals(built_lib, host_only):
    """those of psvo_particle_forecast, status for status"""
    from psvo_amd import _lib
    lib = _lib.load()
    for kw in (dict(Dy=0), dict(Dy=33), dict(layers=2), dict(N=513), dict(emission=3)):
        assert _call(lib, _lib, FC_NAME, desc_kw=dict(Dx=2, **kw)) == _lib.PSVO_ERR_UNSUPPORTED, kw
    for kw in (dict(desc=None), dict(f=None), dict(g=None), dict(X=None), dict(obs=None), dict(sig_f=None), dict(sig_g=None),
               dict(K=-1), dict(ymean=None, yvar=None, xmean=None, lpd=None)):
        assert _call(lib, _lib, FC_NAME, **kw) == _lib.PSVO_ERR_INVALID, kw
    for kw in (dict(B=0), dict(T=0), dict(N=0)):
        assert _call(lib, _lib, FC_NAME, desc_kw=dict(Dx=2, **kw)) == _lib.PSVO_ERR_INVALID, kw
    assert _call(lib, _lib, FC_NAME, desc_kw=dict(emission=2), sig_g=None) == _lib.PSVO_ERR_UNSUPPORTED   # (count: no scale)


def test_the_existing_entry_points_are_as_they_were(built_lib, host_only):
    """the adaptive wide pair still refuses Dy < 3"""
    from psvo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    d = _lib.psvo_desc()
    d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = 2, 4, 8, 1, 2, 2, 32
    d.resample, d.two_q, d.bootstrap, d.emission, d.layers = 1, 1, 0, 0, 1
    m = _lib.psvo_mlp()
    m.W1 = m.b1 = m.W2 = m.b2 = P.value
    M, D = ctypes.byref(m), ctypes.byref(d)
    for Dy in (2, 1):
        d.Dy = Dy
        assert lib.psvo_filter_forward_wobs_adaptive(D, M, M, M, *[P] * 20, ctypes.c_float(0.5), P, P, P,
                                                     None) == _lib.PSVO_ERR_UNSUPPORTED
        assert lib.psvo_filter_backward_wobs_adaptive(D, M, M, M, *[P] * 31, P, None) == _lib.PSVO_ERR_UNSUPPORTED
    assert all(x == 0.0 for x in buf)
