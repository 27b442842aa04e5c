"""C ABI of the wide-observation backward simulation (include/psvo_hip.h: psvo_bsim_forward_wobs, psvo_bsim_backward_wobs,
psvo_bsim_wobs_blocks, psvo_bsim_wobs_ws_floats, psvo_filter_backward_wobs_ext) as far as it can be checked without a GPU: the
symbols are exported and bound, the queries follow their documented formulas, and every refusal comes back as a status before
anything is launched."""
import ctypes

import pytest

NAMES = ("psvo_bsim_forward_wobs", "psvo_bsim_backward_wobs", "psvo_bsim_wobs_blocks", "psvo_bsim_wobs_ws_floats",
         "psvo_filter_backward_wobs_ext")
BSIM = ("psvo_bsim_forward_wobs", "psvo_bsim_backward_wobs")
DX, DY, HH, MM = (2, 3, 4), tuple(range(3, 33)), (16, 32, 64), (4, 8, 16, 32)       # the envelope (N <= 512, one hidden layer)


def test_symbols_are_exported_and_bound(built_lib):
    from psvo_amd import _lib
    dll = ctypes.CDLL(built_lib)
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(dll, name), name
        res, args = _lib.SIGNATURES[name]
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    D, M, P, I = ctypes.POINTER(_lib.psvo_desc), ctypes.POINTER(_lib.psvo_mlp), ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["psvo_bsim_forward_wobs"] == _lib.SIGNATURES["psvo_bsim_forward"]            # the same contract
    plain = _lib.SIGNATURES["psvo_filter_backward_wobs"][1]
    # ... obs eps | X Fm P1 logW lse idx | dlse: 22 arguments, then nparts, dFm_ext, dlogW_ext
    assert _lib.SIGNATURES["psvo_filter_backward_wobs_ext"] == (ctypes.c_int, plain[:22] + [I, P, P] + plain[22:])
    assert _lib.SIGNATURES["psvo_bsim_backward_wobs"] == (ctypes.c_int, [D, P, P, P, M, M, M] + [P] * 35)
    assert lib.psvo_abi_version() == 6        # (added within ABI 6: nothing existing changed)


def _geometry(N, M):
    nt = min(256, 64 * ((N * M + 63) // 64))
    cpb = nt // M
    return (N + cpb - 1) // cpb


def test_workspace_and_block_queries(built_lib):
    from psvo_amd import _lib
    lib = _lib.load()
    for N, M, want in ((16, 4, 1), (40, 8, 2), (32, 16, 2), (24, 32, 3), (130, 4, 3), (512, 4, 8), (512, 32, 64), (1, 4, 1)):
        assert _geometry(N, M) == want
        assert lib.psvo_bsim_wobs_blocks(N, M) == want, (N, M)
    for B, T, N, M, Dx, Dy in ((2, 6, 40, 8, 3, 10), (1, 4, 512, 4, 4, 32), (3, 2, 1, 32, 2, 3)):
        nblk = _geometry(N, M)
        want = T * B * nblk * (Dx + 1) * N + B * nblk * (7 * Dx + Dy)       # d Fm / d logW partials | scale sums
        assert lib.psvo_bsim_wobs_ws_floats(B, T, N, M, Dx, Dy) == want
    assert lib.psvo_bsim_wobs_blocks(0, 4) == 0 and lib.psvo_bsim_wobs_ws_floats(0, 4, 8, 4, 2, 3) == 0


@pytest.fixture
def host_only():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host-code test: never hands a host pointer to a library that can reach a device")


def _desc(_lib, **kw):
    d = _lib.psvo_desc()
    d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = 2, 4, 8, 4, 3, 10, 32
    d.resample, d.two_q, d.bootstrap, d.emission, d.layers = 1, 1, 0, 0, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(lib, _lib, name, buf, desc=None, drop=(), desc_null=False, ints=None):
    """`name` with one small host buffer behind every pointer (and every MLP field) except the argument positions in `drop`
    (NULL); integer arguments take `ints[position]` (default 1).  Only for calls that return before a launch; the buffer must
    come back untouched."""
    addr = (ctypes.addressof(buf) + 15) & ~15
    types = _lib.SIGNATURES[name][1]
    d = desc if desc is not None else _desc(_lib)
    keep, args = [], [None if desc_null else ctypes.byref(d)]
    for i, ty in enumerate(types[1:], 1):
        if ty is ctypes.c_int:
            args.append((ints or {}).get(i, 1))
        elif i in drop or i == len(types) - 1:           # (the stream is NULL)
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
    # psvo_bsim_forward_wobs: desc | X Fm logW lse | f g q1_inv | sig_f sig_g sig_q1inv sig_bq2 | bmu2 minit sig_init | imean isig
    # | obs eps_b u_b sel_in | bwX flp glp Omega sel_out score | lam2_all om_all mu1_all | stream.  Required: everything but X,
    # one of u_b / sel_in, and the three saves.
    for i in [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 21, 22, 23, 24, 25, 26]:
        assert _call(lib, _lib, "psvo_bsim_forward_wobs", buf, drop=(i,)) == _lib.PSVO_ERR_INVALID, i
    assert _call(lib, _lib, "psvo_bsim_forward_wobs", buf, drop=(19, 20)) == _lib.PSVO_ERR_INVALID       # nothing to draw with
    # psvo_bsim_backward_wobs: every pointer argument is required (positions 1 .. 40, the workspace included)
    n = len(_lib.SIGNATURES["psvo_bsim_backward_wobs"][1])
    for i in range(1, n - 1):
        assert _call(lib, _lib, "psvo_bsim_backward_wobs", buf, drop=(i,)) == _lib.PSVO_ERR_INVALID, i
    for name in BSIM:
        assert _call(lib, _lib, name, buf, desc_null=True) == _lib.PSVO_ERR_INVALID
        for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(T=-3), dict(N=0), dict(N=-8)):
            assert _call(lib, _lib, name, buf, desc=_desc(_lib, **kw)) == _lib.PSVO_ERR_INVALID, (name, kw)
        # T = 1: no step has a successor (the rule of psvo_bsim_forward, stated in the header)
        assert _call(lib, _lib, name, buf, desc=_desc(_lib, T=1)) == _lib.PSVO_ERR_INVALID, name
        # an invalid argument is reported as such whatever the shape
        assert _call(lib, _lib, name, buf, desc=_desc(_lib, Dy=2), drop=(2,)) == _lib.PSVO_ERR_INVALID
        assert _call(lib, _lib, name, buf, desc=_desc(_lib, Dy=2, N=0)) == _lib.PSVO_ERR_INVALID
    # psvo_filter_backward_wobs_ext: what psvo_filter_backward_wobs requires, and nparts >= 1 with an external gradient
    ext = "psvo_filter_backward_wobs_ext"
    fdesc = lambda **kw: _desc(_lib, M=1, **kw)
    for i in [1, 3, 4, 7, 9, 10, 11, 12, 13, 14, 15, 16, 18, 19, 25, 27, 29, 30, 31, 32, 33, 34, 35, 36, 37]:
        assert _call(lib, _lib, ext, buf, desc=fdesc(), drop=(i,)) == _lib.PSVO_ERR_INVALID, i
    for nparts in (0, -2):
        assert _call(lib, _lib, ext, buf, desc=fdesc(), ints={22: nparts}) == _lib.PSVO_ERR_INVALID
        assert _call(lib, _lib, ext, buf, desc=fdesc(), ints={22: nparts}, drop=(23,)) == _lib.PSVO_ERR_INVALID
    assert _call(lib, _lib, ext, buf, desc=fdesc(Dy=2), drop=(1,)) == _lib.PSVO_ERR_INVALID
    with pytest.raises(ValueError):
        _lib.check(_call(lib, _lib, "psvo_bsim_forward_wobs", buf, drop=(2,)), "psvo_bsim_forward_wobs")


def test_shapes_outside_the_envelope_are_unsupported(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    cases = [dict(Dy=v) for v in (0, 1, 2, 33, -3)] + [dict(Dx=v) for v in (1, 5)] + [dict(H=v) for v in (8, 48, 128)]
    cases += [dict(M=v) for v in (1, 2, 3, 12, 64)] + [dict(layers=2), dict(layers=-1), dict(N=513), dict(Dy=2, Dx=5)]
    for name in BSIM:
        for kw in cases:
            d = _desc(_lib, **kw)
            inside = d.Dx in DX and d.Dy in DY and d.H in HH and d.M in MM and d.layers in (0, 1) and 0 < d.N <= 512
            assert not inside, (name, kw)
            assert _call(lib, _lib, name, buf, desc=d) == _lib.PSVO_ERR_UNSUPPORTED, (name, kw)
    for kw in (dict(Dy=2), dict(Dy=33), dict(Dx=5), dict(H=48), dict(layers=2), dict(N=513)):
        assert _call(lib, _lib, "psvo_filter_backward_wobs_ext", buf, desc=_desc(_lib, M=1, **kw)) == _lib.PSVO_ERR_UNSUPPORTED, kw
    # the Dy <= 2 entry points are unchanged: Dy = 3 is outside what they are instantiated for
    for name in ("psvo_bsim_forward", "psvo_bsim_backward"):
        assert _call(lib, _lib, name, buf, desc=_desc(_lib, Dy=3)) == _lib.PSVO_ERR_UNSUPPORTED, name
