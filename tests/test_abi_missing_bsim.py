"""C ABI of PSVO on missing observations (include/psvo_hip.h: psvo_bsim_forward_wobs_missing, psvo_bsim_backward_wobs_missing,
psvo_filter_backward_wobs_missing_ext) as far as it can be checked without a GPU: the symbols are exported and bound with the
static pair's argument lists, and every refusal comes back with the static pair's status, in the static pair's order, before
anything is launched."""
import ctypes

import pytest

from tests.test_abi_wobs_bsim import _call, _desc, host_only      # noqa: F401  (the fixture)

FWD, BWD, EXT = "psvo_bsim_forward_wobs_missing", "psvo_bsim_backward_wobs_missing", "psvo_filter_backward_wobs_missing_ext"
STATIC = {FWD: "psvo_bsim_forward_wobs", BWD: "psvo_bsim_backward_wobs", EXT: "psvo_filter_backward_wobs_ext"}
DX, DY, HH, MM = (2, 3, 4), tuple(range(1, 33)), (16, 32, 64), (4, 8, 16, 32)       # the envelope (N <= 512, one hidden layer)


def test_symbols_are_exported_and_bound(built_lib):
    from psvo_amd import _lib
    dll = ctypes.CDLL(built_lib)
    lib = _lib.load()
    for name, static in STATIC.items():
        assert hasattr(dll, name), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[static], name           # the static entry point's argument list
        res, args = _lib.SIGNATURES[name]
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    assert lib.psvo_abi_version() == 6        # (added within ABI 6: nothing existing changed)
    # the dlse-only entry point keeps its signature
    assert _lib.SIGNATURES["psvo_filter_backward_wobs_missing"] == _lib.SIGNATURES["psvo_filter_backward_wobs"]


def test_the_header_declares_them():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "psvo_hip.h")).read()
    for name in STATIC:
        assert ("int %s(const psvo_desc* desc," % name) in text, name


def test_a_complete_call_inside_the_envelope_is_not_made_here(built_lib, host_only):
    """every check below ends in a refusal; the shapes the static pair refuses and this pair accepts are told apart by the
    FIRST refusal behind them: Dy = 1 and Dy = 2 with N = 513 are refused for N, not for Dy (and Dy = 1 with a NULL pointer for
    the pointer)"""
    from psvo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    for name in (FWD, BWD):
        for Dy in (1, 2, 3, 32):
            assert _call(lib, _lib, name, buf, desc=_desc(_lib, Dy=Dy, N=513)) == _lib.PSVO_ERR_UNSUPPORTED
            assert _call(lib, _lib, name, buf, desc=_desc(_lib, Dy=Dy), drop=(2,)) == _lib.PSVO_ERR_INVALID
            assert _call(lib, _lib, name, buf, desc=_desc(_lib, Dy=Dy, T=1)) == _lib.PSVO_ERR_INVALID


def test_invalid_arguments_are_refused_before_any_launch(built_lib, host_only):
    """the static pair's codes in the static pair's order: every call is made on both and the statuses are compared"""
    from psvo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    both = lambda name, **kw: (_call(lib, _lib, name, buf, **kw), _call(lib, _lib, STATIC[name], buf, **kw))
    # forward: required is everything but X, one of u_b / sel_in, and the three saves
    for i in [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 21, 22, 23, 24, 25, 26]:
        assert both(FWD, drop=(i,)) == (_lib.PSVO_ERR_INVALID,) * 2, i
    assert both(FWD, drop=(19, 20)) == (_lib.PSVO_ERR_INVALID,) * 2               # nothing to draw with
    n = len(_lib.SIGNATURES[BWD][1])
    for i in range(1, n - 1):                                                      # reverse: every pointer, the workspace included
        assert both(BWD, drop=(i,)) == (_lib.PSVO_ERR_INVALID,) * 2, i
    for name in (FWD, BWD):
        assert both(name, desc_null=True) == (_lib.PSVO_ERR_INVALID,) * 2
        for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(T=-3), dict(T=1), dict(N=0), dict(N=-8)):
            assert both(name, desc=_desc(_lib, **kw)) == (_lib.PSVO_ERR_INVALID,) * 2, (name, kw)
        # the order: a bad emission answers first, then a missing pointer, then a size that is none, then the envelope
        assert both(name, desc=_desc(_lib, emission=3), drop=(2,)) == (_lib.PSVO_ERR_UNSUPPORTED,) * 2
        assert both(name, desc=_desc(_lib, emission=-1, N=0)) == (_lib.PSVO_ERR_UNSUPPORTED,) * 2
        assert both(name, desc=_desc(_lib, Dy=33), drop=(2,)) == (_lib.PSVO_ERR_INVALID,) * 2
        assert both(name, desc=_desc(_lib, Dy=0, N=0)) == (_lib.PSVO_ERR_INVALID,) * 2
        assert both(name, desc=_desc(_lib, layers=2, T=1)) == (_lib.PSVO_ERR_INVALID,) * 2
        assert both(name, desc=_desc(_lib, M=3, B=0)) == (_lib.PSVO_ERR_INVALID,) * 2
    # psvo_filter_backward_wobs_missing_ext: what psvo_filter_backward_wobs_ext requires, and nparts >= 1 with an external gradient
    fdesc = lambda **kw: _desc(_lib, M=1, **kw)
    for i in [1, 3, 4, 7, 9, 10, 11, 12, 13, 14, 15, 16, 18, 19, 25, 27, 29, 30, 31, 32, 33, 34, 35, 36, 37]:
        assert both(EXT, desc=fdesc(), drop=(i,)) == (_lib.PSVO_ERR_INVALID,) * 2, i
    for nparts in (0, -2):
        assert both(EXT, desc=fdesc(), ints={22: nparts}) == (_lib.PSVO_ERR_INVALID,) * 2
        assert both(EXT, desc=fdesc(), ints={22: nparts}, drop=(23,)) == (_lib.PSVO_ERR_INVALID,) * 2
    assert _call(lib, _lib, EXT, buf, desc=fdesc(T=1)) == _lib.PSVO_ERR_INVALID     # (the missing pair's T >= 2)
    assert _call(lib, _lib, EXT, buf, desc=fdesc(Dy=1), drop=(1,)) == _lib.PSVO_ERR_INVALID
    with pytest.raises(ValueError):
        _lib.check(_call(lib, _lib, FWD, buf, drop=(2,)), FWD)


def test_shapes_outside_the_envelope_are_unsupported(built_lib, host_only):
    from psvo_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    cases = [dict(Dy=v) for v in (0, 33, -3)] + [dict(Dx=v) for v in (1, 5)] + [dict(H=v) for v in (8, 48, 128)]
    cases += [dict(M=v) for v in (1, 2, 3, 12, 64)] + [dict(layers=2), dict(layers=-1), dict(N=513), dict(Dy=2, Dx=5)]
    cases += [dict(emission=3), dict(emission=-1), dict(Dy=1, M=3), dict(Dy=1, layers=2)]
    for name in (FWD, BWD):
        for kw in cases:
            d = _desc(_lib, **kw)
            inside = (d.Dx in DX and d.Dy in DY and d.H in HH and d.M in MM and d.layers in (0, 1) and 0 < d.N <= 512
                      and d.emission in (0, 1, 2))
            assert not inside, (name, kw)
            assert _call(lib, _lib, name, buf, desc=d) == _lib.PSVO_ERR_UNSUPPORTED, (name, kw)
            # the static pair gives the same code for the same shape
            assert _call(lib, _lib, STATIC[name], buf, desc=d) == _lib.PSVO_ERR_UNSUPPORTED, (name, kw)
    for kw in (dict(Dy=0), dict(Dy=33), dict(Dx=5), dict(H=48), dict(layers=2), dict(N=513), dict(emission=3)):
        assert _call(lib, _lib, EXT, buf, desc=_desc(_lib, M=1, **kw)) == _lib.PSVO_ERR_UNSUPPORTED, kw
    # the existing entry points are as they were: the static pair still refuses Dy < 3
    for name in STATIC.values():
        for Dy in (1, 2):
            assert _call(lib, _lib, name, buf, desc=_desc(_lib, M=1 if name.startswith("psvo_filter") else 4, Dy=Dy)) \
                == _lib.PSVO_ERR_UNSUPPORTED, (name, Dy)
