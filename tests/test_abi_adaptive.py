"""C ABI of adaptive resampling (include/psvo_hip.h: psvo_filter_forward_adaptive / psvo_filter_backward_adaptive) as far as it can
be checked without a GPU: the symbols are exported and bound, and every refusal of the contract comes back as a status before
anything is launched."""
import ctypes

import pytest

FWD = ("desc", "q1", "f", "g", "sig_q1", "sig_q2", "sig_f", "sig_g", "mu2", "m0", "sig0", "fm0", "fsig0", "obs", "eps", "u",
       "idx_in", "X", "Xanc", "Fm", "P1", "logW", "idx_out", "lse", "ess_frac", "rs_in", "rs_out", "ess_out", "stream")
BWD = ("desc", "q1", "f", "g", "sig_q1", "sig_q2", "sig_f", "sig_g", "mu2", "m0", "sig0", "fm0", "fsig0", "obs", "eps", "X", "Fm",
       "P1", "logW", "lse", "idx", "dlse", "nparts", "dFm_ext", "dlogW_ext", "dP", "dF", "dG", "dmu2", "dm0", "dfm0", "dsig_q1",
       "dsig_q2", "dsig_f", "dsig_g", "dsig0", "dfsig0", "sacc", "rs", "stream")


def test_symbols_are_exported_and_bound(built_lib):
    from psvo_amd import _lib
    so = ctypes.CDLL(built_lib)
    D, M, P = ctypes.POINTER(_lib.psvo_desc), ctypes.POINTER(_lib.psvo_mlp), ctypes.c_void_p
    plain_f, plain_b = _lib.SIGNATURES["psvo_filter_forward"][1], _lib.SIGNATURES["psvo_filter_backward"][1]
    for name, names, want in (("psvo_filter_forward_adaptive", FWD, plain_f[:-1] + [ctypes.c_float, P, P, P] + plain_f[-1:]),
                              ("psvo_filter_backward_adaptive", BWD, plain_b[:-1] + [P] + plain_b[-1:])):
        assert hasattr(so, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(names) and args == want, name       # the static arguments, then the new ones
        assert args[0] is D and args[1:4] == [M, M, M]
        assert getattr(_lib.load(), name).argtypes == args
    assert _lib.load().psvo_abi_version() == 6        # (added within ABI 6: nothing existing changed)
    # the existing entry points keep their signatures
    assert plain_f == [D, M, M, M] + [P] * 21 and plain_b == [D, M, M, M] + [P] * 18 + [ctypes.c_int] + [P] * 16


@pytest.fixture
def host_only():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-code test: never hands a host pointer to a library that can reach a device")


def _call(lib, _lib, name, desc_kw=None, **kw):
    """the entry point with every pointer set (one small host buffer behind each), ess_frac = 0.5, nparts = 0 and no upstream
    gradient of Fm / logW, except what `desc_kw` / `kw` replace.  The descriptor's Dx = 5 lies OUTSIDE the envelope, so a call
    that passes every check ends in the shape dispatch's PSVO_ERR_UNSUPPORTED: nothing is ever launched."""
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    d = _lib.psvo_desc()
    d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = 2, 4, 8, 4, 5, 1, 32
    d.resample, d.two_q, d.bootstrap, d.emission, d.layers = 1, 1, 1, 0, 1
    for k, v in (desc_kw or {}).items():
        setattr(d, k, v)
    mlps = []
    for _ in range(3):
        m = _lib.psvo_mlp()
        m.W1 = m.b1 = m.W2 = m.b2 = P.value
        mlps.append(m)
    names = FWD if name.endswith("forward_adaptive") else BWD
    a = {k: P for k in names}
    a.update(desc=ctypes.byref(d), q1=ctypes.byref(mlps[0]), f=ctypes.byref(mlps[1]), g=ctypes.byref(mlps[2]), stream=None,
             ess_frac=ctypes.c_float(0.5), nparts=0, dFm_ext=None, dlogW_ext=None)
    a.update(kw)
    st = getattr(lib, name)(*[a[k] for k in names])
    assert all(x == 0.0 for x in buf), "a refused call wrote to its buffers"
    return st


def test_a_complete_call_reaches_the_shape_dispatch(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    for name in ("psvo_filter_forward_adaptive", "psvo_filter_backward_adaptive"):
        assert _call(lib, _lib, name) == _lib.PSVO_ERR_UNSUPPORTED, name                    # (Dx = 5: see _call)
        assert _call(lib, _lib, name, desc_kw=dict(Dx=2, N=513)) == _lib.PSVO_ERR_UNSUPPORTED, name
    assert _call(lib, _lib, "psvo_filter_forward_adaptive", rs_in=None) == _lib.PSVO_ERR_UNSUPPORTED      # rs_in is optional
    assert _call(lib, _lib, "psvo_filter_forward_adaptive", ess_frac=ctypes.c_float(2.0)) == _lib.PSVO_ERR_UNSUPPORTED


def test_forward_refusals(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    name = "psvo_filter_forward_adaptive"
    for frac in (0.0, -0.5, float("nan"), -float("inf")):
        assert _call(lib, _lib, name, ess_frac=ctypes.c_float(frac)) == _lib.PSVO_ERR_INVALID, frac
    assert _call(lib, _lib, name, desc_kw=dict(resample=0)) == _lib.PSVO_ERR_INVALID
    for kw in (dict(rs_out=None), dict(ess_out=None), dict(desc=None), dict(X=None), dict(lse=None), dict(u=None, idx_in=None)):
        assert _call(lib, _lib, name, **kw) == _lib.PSVO_ERR_INVALID, kw
    # the adaptive contract is checked first: inside the envelope too, and whatever else is wrong with the call
    assert _call(lib, _lib, name, desc_kw=dict(Dx=2), rs_out=None) == _lib.PSVO_ERR_INVALID
    assert _call(lib, _lib, name, desc_kw=dict(Dx=2, layers=3), ess_out=None) == _lib.PSVO_ERR_INVALID
    for kw in (dict(layers=3), dict(emission=2), dict(emission=-1)):
        assert _call(lib, _lib, name, desc_kw=kw) == _lib.PSVO_ERR_UNSUPPORTED, kw
    with pytest.raises(ValueError):
        _lib.check(_call(lib, _lib, name, rs_out=None), name)


def test_backward_refusals(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    name = "psvo_filter_backward_adaptive"
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p(ctypes.addressof(buf))
    assert _call(lib, _lib, name, rs=None) == _lib.PSVO_ERR_INVALID
    assert _call(lib, _lib, name, desc_kw=dict(resample=0)) == _lib.PSVO_ERR_INVALID
    assert _call(lib, _lib, name, desc=None) == _lib.PSVO_ERR_INVALID
    # a backward simulation behind an adaptive filter is not built: upstream gradients of Fm / logW, partial or whole
    for kw in (dict(nparts=2), dict(dFm_ext=P, nparts=1), dict(dlogW_ext=P, nparts=1), dict(dFm_ext=P, dlogW_ext=P, nparts=4)):
        assert _call(lib, _lib, name, **kw) == _lib.PSVO_ERR_UNSUPPORTED, kw
        assert _call(lib, _lib, name, desc_kw=dict(Dx=2), **kw) == _lib.PSVO_ERR_UNSUPPORTED, kw
    assert _call(lib, _lib, name, desc_kw=dict(Dx=2), rs=None, dFm_ext=P, nparts=1) == _lib.PSVO_ERR_INVALID
    for kw in (dict(dP=None), dict(sacc=None), dict(idx=None), dict(logW=None)):
        assert _call(lib, _lib, name, **kw) == _lib.PSVO_ERR_INVALID, kw
    assert _call(lib, _lib, name, desc_kw=dict(layers=3)) == _lib.PSVO_ERR_UNSUPPORTED


def test_the_static_entry_points_are_as_they_were(built_lib, host_only):
    """the same complete argument lists without the adaptive arguments: the shape dispatch; resample = 0 is theirs to take"""
    from psvo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    d = _lib.psvo_desc()
    d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = 2, 4, 8, 4, 5, 1, 32
    d.two_q, d.bootstrap, d.emission, d.layers = 1, 1, 0, 1
    m = _lib.psvo_mlp()
    m.W1 = m.b1 = m.W2 = m.b2 = P.value
    M = ctypes.byref(m)
    for resample in (0, 1):
        d.resample = resample
        assert lib.psvo_filter_forward(ctypes.byref(d), M, M, M, *[P] * 20, None) == _lib.PSVO_ERR_UNSUPPORTED
        assert lib.psvo_filter_backward(ctypes.byref(d), M, M, M, *[P] * 18, 0, None, None, *[P] * 13, None) == _lib.PSVO_ERR_UNSUPPORTED
