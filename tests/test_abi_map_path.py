"""C ABI of the MAP trajectory (include/psvo_hip.h: psvo_map_path) as far as it can be checked without a GPU: the symbol is
exported and bound within ABI 6, and every refusal comes back as a status before anything is launched."""
import ctypes

import pytest

ARGS = ("desc", "g", "sig_f", "sig_g", "fm0", "fsig0", "obs", "X", "Fm", "delta", "lmax", "bp", "path", "Xmap", "stream")


def test_symbol_is_exported_and_bound(built_lib):
    from psvo_amd import _lib
    assert hasattr(ctypes.CDLL(built_lib), "psvo_map_path")
    res, args = _lib.SIGNATURES["psvo_map_path"]
    assert res is ctypes.c_int and len(args) == len(ARGS)
    assert args[0] is ctypes.POINTER(_lib.psvo_desc) and args[1] is ctypes.POINTER(_lib.psvo_mlp)
    assert all(a is ctypes.c_void_p for a in args[2:])
    assert _lib.load().psvo_map_path.argtypes == args
    assert _lib.load().psvo_abi_version() == 6        # (added within ABI 6: nothing existing changed)


def _call(lib, _lib, desc_kw=None, mlp_kw=None, **kw):
    """psvo_map_path with every argument valid (one small host buffer behind every pointer, all inputs and outputs) except what
    `desc_kw` / `mlp_kw` / `kw` replace.  Only for calls that return before a launch."""
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p(ctypes.addressof(buf))
    d = _lib.psvo_desc()
    d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = 2, 4, 8, 1, 2, 1, 32
    d.resample, d.two_q, d.bootstrap, d.emission, d.layers = 1, 1, 1, 0, 1
    for k, v in (desc_kw or {}).items():
        setattr(d, k, v)
    g = _lib.psvo_mlp()
    g.W1 = g.b1 = g.W2 = g.b2 = ctypes.addressof(buf)
    for k, v in (mlp_kw or {}).items():
        setattr(g, k, v)
    a = dict(desc=ctypes.byref(d), g=ctypes.byref(g), sig_f=P, sig_g=P, fm0=P, fsig0=P, obs=P, X=P, Fm=P, delta=P, lmax=P, bp=P,
             path=P, Xmap=P, stream=None)
    a.update(kw)
    st = lib.psvo_map_path(*[a[k] for k in ARGS])
    assert all(x == 0.0 for x in buf), "a refused call wrote to its buffers"
    return st


@pytest.fixture
def host_only():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-code test: never hands a host pointer to a library that can reach a device")


def test_invalid_arguments_are_refused_before_any_launch(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    for name in ("desc", "g", "sig_f", "fm0", "fsig0", "obs", "X", "Fm", "delta", "lmax", "bp"):      # required pointers
        assert _call(lib, _lib, **{name: None}) == _lib.PSVO_ERR_INVALID, name
    assert _call(lib, _lib, sig_g=None) == _lib.PSVO_ERR_INVALID                   # Gaussian emission without a scale
    assert _call(lib, _lib, desc_kw=dict(emission=1), sig_g=None) == _lib.PSVO_ERR_INVALID
    for name in ("W1", "b1", "W2", "b2"):
        assert _call(lib, _lib, mlp_kw={name: None}) == _lib.PSVO_ERR_INVALID, name
    for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(T=-3), dict(N=0), dict(N=-8)):
        assert _call(lib, _lib, desc_kw=kw) == _lib.PSVO_ERR_INVALID, kw
    with pytest.raises(ValueError):
        _lib.check(_call(lib, _lib, X=None), "psvo_map_path")


def test_shapes_outside_the_envelope_are_unsupported(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    edges = (dict(Dx=1), dict(Dx=5), dict(Dx=0), dict(Dy=0), dict(Dy=33), dict(Dy=-1), dict(H=8), dict(H=48), dict(H=128),
             dict(N=513), dict(N=600), dict(N=1024), dict(emission=3), dict(emission=-1), dict(layers=2), dict(layers=3),
             dict(layers=-1), dict(N=513, Dx=5), dict(T=1 << 20, B=1 << 12))
    for kw in edges:
        assert _call(lib, _lib, desc_kw=kw) == _lib.PSVO_ERR_UNSUPPORTED, kw
        assert _call(lib, _lib, desc_kw=kw, path=None, Xmap=None) == _lib.PSVO_ERR_UNSUPPORTED, kw
    # the count emission has no scale: sig_g = NULL passes the argument checks there (and the shape is then refused)
    assert _call(lib, _lib, desc_kw=dict(emission=2, Dx=5), sig_g=None) == _lib.PSVO_ERR_UNSUPPORTED
    assert _call(lib, _lib, desc_kw=dict(emission=1, Dx=5), sig_g=None) == _lib.PSVO_ERR_INVALID
    # an invalid argument is reported as such whatever the shape
    assert _call(lib, _lib, desc_kw=dict(Dx=5), X=None) == _lib.PSVO_ERR_INVALID
    assert _call(lib, _lib, desc_kw=dict(N=600), bp=None) == _lib.PSVO_ERR_INVALID
    # M, resample, two_q and bootstrap are not looked at
    assert _call(lib, _lib, desc_kw=dict(M=3, resample=7, two_q=5, bootstrap=9, Dx=7)) == _lib.PSVO_ERR_UNSUPPORTED
