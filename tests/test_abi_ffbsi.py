"""C ABI of the backward sampler (include/psvo_hip.h: psvo_ffbs_sample) as far as it can be checked without a GPU: the symbol
is exported and bound within ABI 6, and every refusal comes back as a status before anything is launched."""
import ctypes

import pytest

ARGS = ("desc", "X", "Fm", "Fs", "sig_f", "logW", "u", "idx_in", "Xs", "idx_out", "logq", "distinct", "stream")


def test_symbol_is_exported_and_bound(built_lib):
    from psvo_amd import _lib
    assert hasattr(ctypes.CDLL(built_lib), "psvo_ffbs_sample")
    res, args = _lib.SIGNATURES["psvo_ffbs_sample"]
    assert res is ctypes.c_int and len(args) == len(ARGS)
    assert args[0] is ctypes.POINTER(_lib.psvo_desc) and all(a is ctypes.c_void_p for a in args[1:])
    assert _lib.load().psvo_ffbs_sample.argtypes == args
    assert _lib.load().psvo_abi_version() == 6        # (added within ABI 6: nothing existing changed)


def _call(lib, _lib, desc_kw=None, **kw):
    """psvo_ffbs_sample with every argument valid (one small host buffer behind every pointer, constant scale, uniforms, all
    outputs) except what `desc_kw` / `kw` replace.  Only for calls that return before a launch."""
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p(ctypes.addressof(buf))
    d = _lib.psvo_desc()
    d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = 2, 4, 8, 4, 2, 1, 32
    d.resample, d.two_q, d.bootstrap, d.emission, d.layers = 1, 1, 1, 0, 1
    for k, v in (desc_kw or {}).items():
        setattr(d, k, v)
    a = dict(desc=ctypes.byref(d), X=P, Fm=P, Fs=None, sig_f=P, logW=P, u=P, idx_in=None, Xs=P, idx_out=P, logq=P, distinct=P,
             stream=None)
    a.update(kw)
    st = lib.psvo_ffbs_sample(*[a[k] for k in ARGS])
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
    keep = (ctypes.c_float * 64)()
    P = ctypes.c_void_p(ctypes.addressof(keep))
    bad = [dict(desc=None), dict(X=None), dict(Fm=None), dict(logW=None),                          # required pointers
           dict(Fs=P), dict(sig_f=None),                                                           # both scales / neither
           dict(u=None),                                                                           # nothing to draw with
           dict(Xs=None, idx_out=None, logq=None, distinct=None)]                                  # no output at all
    for kw in bad:
        assert _call(lib, _lib, **kw) == _lib.PSVO_ERR_INVALID, kw
    for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(T=-3), dict(N=0), dict(N=-8)):
        assert _call(lib, _lib, desc_kw=kw) == _lib.PSVO_ERR_INVALID, kw
    with pytest.raises(ValueError):
        _lib.check(_call(lib, _lib, X=None), "psvo_ffbs_sample")
    assert all(x == 0.0 for x in keep)


def test_shapes_outside_the_envelope_are_unsupported(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    for kw in (dict(Dx=1), dict(Dx=5), dict(Dx=0), dict(Dx=8), dict(N=513), dict(N=1024), dict(N=513, Dx=5)):
        assert _call(lib, _lib, desc_kw=kw) == _lib.PSVO_ERR_UNSUPPORTED, kw
    # nothing but B, T, N and Dx is dispatched on: values no other entry point takes are not looked at (Dx is still refused)
    assert _call(lib, _lib, desc_kw=dict(Dx=7, H=48, Dy=9, M=3, layers=5)) == _lib.PSVO_ERR_UNSUPPORTED
    # an invalid argument is reported as such whatever the shape
    assert _call(lib, _lib, desc_kw=dict(Dx=5), X=None) == _lib.PSVO_ERR_INVALID
    assert _call(lib, _lib, desc_kw=dict(N=600), u=None) == _lib.PSVO_ERR_INVALID
