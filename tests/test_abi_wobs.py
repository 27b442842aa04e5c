"""C ABI of the wide-observation entry points (include/psvo_hip.h: psvo_filter_forward_wobs, psvo_filter_wobs_ws_floats,
psvo_filter_backward_wobs, psvo_mlp_wgrad_wobs_blocks, psvo_mlp_wgrad_wobs) as far as it can be checked without a GPU: the
symbols are exported and bound, and every refusal comes back as a status before anything is launched."""
import ctypes

import pytest

NAMES = ("psvo_filter_forward_wobs", "psvo_filter_wobs_ws_floats", "psvo_filter_backward_wobs", "psvo_mlp_wgrad_wobs_blocks",
         "psvo_mlp_wgrad_wobs")
FILTERS = ("psvo_filter_forward_wobs", "psvo_filter_backward_wobs")
DX, DY, HH = (2, 3, 4), tuple(range(3, 33)), (16, 32, 64)       # the envelope (N <= 512, one hidden layer)


def test_symbols_are_exported_and_bound(built_lib):
    from psvo_amd import _lib
    dll = ctypes.CDLL(built_lib)
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(dll, name), name
        res, args = _lib.SIGNATURES[name]
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    D, M, P = ctypes.POINTER(_lib.psvo_desc), ctypes.POINTER(_lib.psvo_mlp), ctypes.c_void_p
    assert _lib.SIGNATURES["psvo_filter_forward_wobs"] == _lib.SIGNATURES["psvo_filter_forward"]       # the same contract
    assert _lib.SIGNATURES["psvo_filter_backward_wobs"] == (ctypes.c_int, [D, M, M, M] + [P] * 32)
    assert _lib.SIGNATURES["psvo_mlp_wgrad_wobs"] == _lib.SIGNATURES["psvo_mlp_wgrad"]
    assert _lib.SIGNATURES["psvo_mlp_wgrad_wobs_blocks"] == _lib.SIGNATURES["psvo_mlp_wgrad_blocks"]
    assert lib.psvo_abi_version() == 6        # (added within ABI 6: nothing existing changed)


def test_workspace_and_block_queries(built_lib):
    from psvo_amd import _lib
    lib = _lib.load()
    # per-sequence sums (two sets of 5 Dx, then Dy) | the (T, B, Dx, N) rows of d mu2
    assert lib.psvo_filter_wobs_ws_floats(2, 4, 8, 3, 10) == 2 * (10 * 3 + 10) + 4 * 2 * 3 * 8
    assert lib.psvo_filter_wobs_ws_floats(1, 1, 1, 2, 3) == 23 + 2
    assert lib.psvo_mlp_wgrad_wobs_blocks(1) == 1 and lib.psvo_mlp_wgrad_wobs_blocks(259) == 2
    assert lib.psvo_mlp_wgrad_wobs_blocks(10 ** 9) == 512


@pytest.fixture
def host_only():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-code test: never hands a host pointer to a library that can reach a device")


def _desc(_lib, **kw):
    d = _lib.psvo_desc()
    d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = 2, 4, 8, 1, 3, 10, 32
    d.resample, d.two_q, d.bootstrap, d.emission, d.layers = 1, 1, 0, 0, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(lib, _lib, name, buf, desc=None, drop=(), desc_null=False):
    """`name` with one small host buffer behind every pointer (and every MLP field) except the argument positions in `drop`
    (NULL).  Only for calls that return before a launch; the buffer must come back untouched."""
    addr = (ctypes.addressof(buf) + 15) & ~15
    types = _lib.SIGNATURES[name][1]
    d = desc if desc is not None else _desc(_lib)
    keep, args = [], [None if desc_null else ctypes.byref(d)]
    for i, ty in enumerate(types[1:], 1):
        if i in drop or i == len(types) - 1:           # (the stream is NULL)
            args.append(None)
        elif ty is ctypes.POINTER(_lib.psvo_mlp):
            m = _lib.psvo_mlp()
            for f, _ in m._fields_:
                setattr(m, f, addr)
            keep.append(m)
            args.append(ctypes.byref(m))
        else:
            args.append(ctypes.c_void_p(addr))
    st = getattr(lib, name)(*args)
    assert all(x == 0.0 for x in buf), "a refused call wrote to its buffers"
    return st


def test_invalid_arguments_are_refused_before_any_launch(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    # psvo_filter_forward_wobs: desc | q1 f g | sig_q1 sig_q2 sig_f sig_g | mu2 | m0 sig0 fm0 fsig0 | obs eps u idx_in | X Xanc Fm
    # P1 logW idx_out lse | stream.  Required whatever the wiring: everything but f, sig_q2, sig_f, mu2, u, idx_in, P1.
    fwd_required = [1, 3, 4, 7, 9, 10, 11, 12, 13, 14, 17, 18, 19, 21, 22, 23]
    for i in fwd_required:
        assert _call(lib, _lib, "psvo_filter_forward_wobs", buf, drop=(i,)) == _lib.PSVO_ERR_INVALID, i
    assert _call(lib, _lib, "psvo_filter_forward_wobs", buf, drop=(2,)) == _lib.PSVO_ERR_INVALID        # f without bootstrap
    assert _call(lib, _lib, "psvo_filter_forward_wobs", buf, drop=(8,)) == _lib.PSVO_ERR_INVALID        # mu2 under two_q
    assert _call(lib, _lib, "psvo_filter_forward_wobs", buf, drop=(15, 16)) == _lib.PSVO_ERR_INVALID    # nothing to draw with
    # psvo_filter_backward_wobs: ... obs eps | X Fm P1 logW lse idx | dlse | dP dF dG dmu2 dm0 dfm0 | six scale gradients | ws
    bwd_required = [1, 3, 4, 7, 9, 10, 11, 12, 13, 14, 15, 16, 18, 19, 22, 24, 26, 27, 28, 29, 30, 31, 32, 33, 34]
    for i in bwd_required:
        assert _call(lib, _lib, "psvo_filter_backward_wobs", buf, drop=(i,)) == _lib.PSVO_ERR_INVALID, i
    for i in (2, 17, 23, 20, 25):       # f / P1 / dF without bootstrap, idx under resampling, dmu2 under two_q
        assert _call(lib, _lib, "psvo_filter_backward_wobs", buf, drop=(i,)) == _lib.PSVO_ERR_INVALID, i
    for name in FILTERS:
        assert _call(lib, _lib, name, buf, desc_null=True) == _lib.PSVO_ERR_INVALID
        for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(T=-3), dict(N=0), dict(N=-8)):
            assert _call(lib, _lib, name, buf, desc=_desc(_lib, **kw)) == _lib.PSVO_ERR_INVALID, (name, kw)
        # an invalid argument is reported as such whatever the shape
        assert _call(lib, _lib, name, buf, desc=_desc(_lib, Dy=2), drop=(1,)) == _lib.PSVO_ERR_INVALID
    P = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    m = _lib.psvo_mlp()
    for f, _ in m._fields_:
        setattr(m, f, P.value)
    ok = dict(S=7, L=37, Din=3, H=32, Dout=10, X=P, dOut=P, w=ctypes.byref(m), partial=P, grad=P, accumulate=0, stream=None)
    order = ("S", "L", "Din", "H", "Dout", "X", "dOut", "w", "partial", "grad", "accumulate", "stream")
    for bad in (dict(X=None), dict(dOut=None), dict(w=None), dict(partial=None), dict(grad=None), dict(S=0), dict(L=0), dict(L=-4)):
        a = dict(ok, **bad)
        assert lib.psvo_mlp_wgrad_wobs(*[a[k] for k in order]) == _lib.PSVO_ERR_INVALID, bad
    assert all(x == 0.0 for x in buf)
    with pytest.raises(ValueError):
        _lib.check(_call(lib, _lib, "psvo_filter_forward_wobs", buf, drop=(1,)), "psvo_filter_forward_wobs")


def test_shapes_outside_the_envelope_are_unsupported(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    cases = [dict(Dy=v) for v in (0, 2, 33)] + [dict(Dx=v) for v in (1, 5)] + [dict(H=v) for v in (8, 48, 128)]
    cases += [dict(layers=2), dict(N=513), dict(Dy=1), dict(Dy=-3), dict(Dy=2, Dx=5), dict(H=128, layers=2)]
    for name in FILTERS:
        for kw in cases:
            d = _desc(_lib, **kw)
            inside = d.Dx in DX and d.Dy in DY and d.H in HH and d.layers in (0, 1) and 0 < d.N <= 512
            assert not inside, (name, kw)
            assert _call(lib, _lib, name, buf, desc=d) == _lib.PSVO_ERR_UNSUPPORTED, (name, kw)
    P = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    m = _lib.psvo_mlp()
    for f, _ in m._fields_:
        setattr(m, f, P.value)
    for Din, H, Dout in ((3, 32, 2), (3, 32, 0), (3, 32, 33), (0, 32, 10), (5, 32, 10), (3, 8, 10), (3, 48, 10), (3, 128, 10)):
        assert not (1 <= Din <= 4 and H in HH and 3 <= Dout <= 32)
        st = lib.psvo_mlp_wgrad_wobs(7, 37, Din, H, Dout, P, P, ctypes.byref(m), P, P, 0, None)
        assert st == _lib.PSVO_ERR_UNSUPPORTED, (Din, H, Dout)
    assert all(x == 0.0 for x in buf)
