"""C ABI of adaptive resampling on the wide-observation kernels (include/psvo_hip.h: psvo_filter_forward_wobs_adaptive /
psvo_filter_backward_wobs_adaptive) as far as it can be checked without a GPU: the symbols are exported and bound, and every
refusal of the contract comes back as a status before anything is launched."""
import ctypes

import pytest

FWD = ("desc", "q1", "f", "g", "sig_q1", "sig_q2", "sig_f", "sig_g", "mu2", "m0", "sig0", "fm0", "fsig0", "obs", "eps", "u",
       "idx_in", "X", "Xanc", "Fm", "P1", "logW", "idx_out", "lse", "ess_frac", "rs_in", "rs_out", "ess_out", "stream")
BWD = ("desc", "q1", "f", "g", "sig_q1", "sig_q2", "sig_f", "sig_g", "mu2", "m0", "sig0", "fm0", "fsig0", "obs", "eps", "X", "Fm",
       "P1", "logW", "lse", "idx", "dlse", "dP", "dF", "dG", "dmu2", "dm0", "dfm0", "dsig_q1", "dsig_q2", "dsig_f", "dsig_g",
       "dsig0", "dfsig0", "ws", "rs", "stream")
FWD_NAME, BWD_NAME = "psvo_filter_forward_wobs_adaptive", "psvo_filter_backward_wobs_adaptive"


def test_symbols_are_exported_and_bound(built_lib):
    from psvo_amd import _lib
    so = ctypes.CDLL(built_lib)
    D, M, P = ctypes.POINTER(_lib.psvo_desc), ctypes.POINTER(_lib.psvo_mlp), ctypes.c_void_p
    wide_f, wide_b = _lib.SIGNATURES["psvo_filter_forward_wobs"][1], _lib.SIGNATURES["psvo_filter_backward_wobs"][1]
    for name, names, want in ((FWD_NAME, FWD, wide_f[:-1] + [ctypes.c_float, P, P, P] + wide_f[-1:]),
                              (BWD_NAME, BWD, wide_b[:-1] + [P] + wide_b[-1:])):
        assert hasattr(so, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(names) and args == want, name       # the static arguments, then the new ones
        assert args[0] is D and args[1:4] == [M, M, M]
        assert getattr(_lib.load(), name).argtypes == args
    assert _lib.load().psvo_abi_version() == 6        # (added within ABI 6: nothing existing changed)
    # the existing entry points keep their signatures
    assert wide_f == [D, M, M, M] + [P] * 21 and wide_b == [D, M, M, M] + [P] * 32
    assert _lib.SIGNATURES["psvo_filter_forward_adaptive"][1] == [D, M, M, M] + [P] * 20 + [ctypes.c_float, P, P, P, P]


@pytest.fixture
def host_only():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-code test: never hands a host pointer to a library that can reach a device")


def _call(lib, _lib, name, desc_kw=None, **kw):
    """the entry point with every pointer set (one small host buffer behind each) and ess_frac = 0.5, except what `desc_kw` / `kw`
    replace.  The descriptor's Dx = 5 lies OUTSIDE the envelope, so a call that passes every check ends in the shape dispatch's
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
    names = {FWD_NAME: FWD, BWD_NAME: BWD}[name]
    a = {k: P for k in names}
    a.update(desc=ctypes.byref(d), q1=ctypes.byref(mlps[0]), f=ctypes.byref(mlps[1]), g=ctypes.byref(mlps[2]), stream=None,
             ess_frac=ctypes.c_float(0.5))
    a.update(kw)
    st = getattr(lib, name)(*[a[k] for k in names])
    assert all(x == 0.0 for x in buf), "a refused call wrote to its buffers"
    return st


def test_a_complete_call_reaches_the_shape_dispatch(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    for name in (FWD_NAME, BWD_NAME):
        assert _call(lib, _lib, name) == _lib.PSVO_ERR_UNSUPPORTED, name                    # (Dx = 5: see _call)
        for kw in (dict(emission=1), dict(emission=2), dict(bootstrap=1), dict(two_q=0), dict(Dy=3), dict(Dy=32)):
            assert _call(lib, _lib, name, desc_kw=kw) == _lib.PSVO_ERR_UNSUPPORTED, (name, kw)
    assert _call(lib, _lib, FWD_NAME, rs_in=None) == _lib.PSVO_ERR_UNSUPPORTED              # rs_in is optional
    assert _call(lib, _lib, FWD_NAME, ess_frac=ctypes.c_float(2.0)) == _lib.PSVO_ERR_UNSUPPORTED
    assert _call(lib, _lib, BWD_NAME, dlse=None) == _lib.PSVO_ERR_UNSUPPORTED               # dlse is optional (NULL = 0)


def test_forward_refusals(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    name = FWD_NAME
    for frac in (0.0, -0.5, float("nan"), -float("inf")):
        assert _call(lib, _lib, name, ess_frac=ctypes.c_float(frac)) == _lib.PSVO_ERR_INVALID, frac
    assert _call(lib, _lib, name, desc_kw=dict(resample=0)) == _lib.PSVO_ERR_INVALID
    for kw in (dict(rs_out=None), dict(ess_out=None), dict(desc=None), dict(X=None), dict(lse=None), dict(u=None, idx_in=None)):
        assert _call(lib, _lib, name, **kw) == _lib.PSVO_ERR_INVALID, kw
    # the adaptive contract is checked first: inside the envelope too, and whatever else is wrong with the call
    assert _call(lib, _lib, name, desc_kw=dict(Dx=2), rs_out=None) == _lib.PSVO_ERR_INVALID
    assert _call(lib, _lib, name, desc_kw=dict(Dx=2, layers=2), ess_out=None) == _lib.PSVO_ERR_INVALID
    assert _call(lib, _lib, name, desc_kw=dict(Dx=2, Dy=40), ess_frac=ctypes.c_float(0.0)) == _lib.PSVO_ERR_INVALID
    assert _call(lib, _lib, name, desc_kw=dict(Dx=2, emission=3, resample=0)) == _lib.PSVO_ERR_INVALID
    # the wide envelope's own limits (inside Dx / H, so that the shape dispatch is not what answers)
    for kw in (dict(Dy=2), dict(Dy=1), dict(Dy=33), dict(layers=2), dict(N=513), dict(emission=3), dict(emission=-1)):
        assert _call(lib, _lib, name, desc_kw=dict(Dx=2, **kw)) == _lib.PSVO_ERR_UNSUPPORTED, kw
    with pytest.raises(ValueError):
        _lib.check(_call(lib, _lib, name, rs_out=None), name)


def test_backward_refusals(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    name = BWD_NAME
    assert _call(lib, _lib, name, rs=None) == _lib.PSVO_ERR_INVALID
    assert _call(lib, _lib, name, desc_kw=dict(resample=0)) == _lib.PSVO_ERR_INVALID
    assert _call(lib, _lib, name, desc=None) == _lib.PSVO_ERR_INVALID
    # the adaptive contract first
    assert _call(lib, _lib, name, desc_kw=dict(Dx=2, Dy=40), rs=None) == _lib.PSVO_ERR_INVALID
    assert _call(lib, _lib, name, desc_kw=dict(Dx=2, layers=2, resample=0)) == _lib.PSVO_ERR_INVALID
    for kw in (dict(dP=None), dict(ws=None), dict(idx=None), dict(logW=None), dict(dG=None)):
        assert _call(lib, _lib, name, **kw) == _lib.PSVO_ERR_INVALID, kw
    for kw in (dict(Dy=2), dict(Dy=33), dict(layers=2), dict(N=513), dict(emission=3)):
        assert _call(lib, _lib, name, desc_kw=dict(Dx=2, **kw)) == _lib.PSVO_ERR_UNSUPPORTED, kw


def test_the_existing_entry_points_are_as_they_were(built_lib, host_only):
    """the same complete argument lists without the new arguments: the static wide pair ends in the shape dispatch, resample = 0
    is theirs to take; the plain adaptive pair still refuses the count emission and Dy > 2"""
    from psvo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    d = _lib.psvo_desc()
    d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = 2, 4, 8, 1, 5, 10, 32
    d.two_q, d.bootstrap, d.emission, d.layers = 1, 0, 0, 1
    m = _lib.psvo_mlp()
    m.W1 = m.b1 = m.W2 = m.b2 = P.value
    M, D = ctypes.byref(m), ctypes.byref(d)
    for resample in (0, 1):
        d.resample = resample
        assert lib.psvo_filter_forward_wobs(D, M, M, M, *[P] * 20, None) == _lib.PSVO_ERR_UNSUPPORTED
        assert lib.psvo_filter_backward_wobs(D, M, M, M, *[P] * 31, None) == _lib.PSVO_ERR_UNSUPPORTED
        assert lib.psvo_filter_backward_wobs_ext(D, M, M, M, *[P] * 18, 0, None, None, *[P] * 13, None) == _lib.PSVO_ERR_UNSUPPORTED
    d.Dx = 2
    d.Dy = 2
    assert lib.psvo_filter_forward_wobs(D, M, M, M, *[P] * 20, None) == _lib.PSVO_ERR_UNSUPPORTED
    assert lib.psvo_filter_backward_wobs(D, M, M, M, *[P] * 31, None) == _lib.PSVO_ERR_UNSUPPORTED
    # psvo_filter_forward_adaptive / psvo_filter_backward_adaptive: Dy > 2 and emission = 2 stay PSVO_ERR_UNSUPPORTED
    ad_f = lambda: lib.psvo_filter_forward_adaptive(D, M, M, M, *[P] * 20, ctypes.c_float(0.5), P, P, P, None)
    ad_b = lambda: lib.psvo_filter_backward_adaptive(D, M, M, M, *[P] * 18, 0, None, None, *[P] * 13, P, None)
    for Dy, emission in ((10, 0), (3, 0), (2, 2), (10, 2)):
        d.Dy, d.emission = Dy, emission
        assert ad_f() == _lib.PSVO_ERR_UNSUPPORTED, (Dy, emission)
        assert ad_b() == _lib.PSVO_ERR_UNSUPPORTED, (Dy, emission)
    d.Dy, d.emission, d.resample = 10, 0, 0
    assert ad_f() == _lib.PSVO_ERR_INVALID and ad_b() == _lib.PSVO_ERR_INVALID
    assert all(x == 0.0 for x in buf)
