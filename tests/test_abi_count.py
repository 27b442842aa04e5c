"""psvo_desc.emission at the C ABI, NULL pointers, no device: the wide-observation entry points take the count emission
(emission = 2) and refuse anything above it; every other entry point that reads the field takes {0, 1} only -- it used to run
the unit-normal kernels for any non-zero value.  The check sits ahead of the pointer checks (tests/test_abi.py pins that order
for psvo_desc.layers)."""
import ctypes

import pytest

WIDE = ("psvo_filter_forward_wobs", "psvo_filter_backward_wobs", "psvo_filter_backward_wobs_ext", "psvo_bsim_forward_wobs",
        "psvo_bsim_backward_wobs")
PLAIN = ("psvo_filter_forward", "psvo_filter_backward", "psvo_bsim_forward", "psvo_bsim_backward", "psvo_bsimwr_forward",
         "psvo_bsimwr_backward", "psvo_filter_forward_cov", "psvo_filter_backward_cov", "psvo_bsim_forward_cov",
         "psvo_bsim_backward_cov", "psvo_bsim_backward_cov_ws", "psvo_bsimwr_forward_cov", "psvo_bsimwr_backward_cov",
         "psvo_bsimwr_backward_cov_ws")


def _call(lib, _lib, name, d):
    null = lambda ty: 0 if ty in (ctypes.c_int, ctypes.c_longlong) else 0.0 if ty in (ctypes.c_float, ctypes.c_double) else None
    return getattr(lib, name)(ctypes.byref(d), *[null(ty) for ty in _lib.SIGNATURES[name][1][1:]])


def _desc(_lib, Dy, emission):
    d = _lib.psvo_desc()
    d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = 2, 4, 8, 4, 2, Dy, 32
    d.resample, d.two_q, d.bootstrap, d.emission, d.layers = 1, 1, 1, emission, 1
    return d


@pytest.mark.parametrize("name", WIDE)
def test_wide_entry_points_take_the_count_emission(built_lib, name):
    from psvo_amd import _lib
    lib = _lib.load()
    for emission in (0, 1, 2):          # accepted; the pointers are missing
        assert _call(lib, _lib, name, _desc(_lib, 10, emission)) == _lib.PSVO_ERR_INVALID, emission
    for emission in (3, -1, 1 << 20):
        assert _call(lib, _lib, name, _desc(_lib, 10, emission)) == _lib.PSVO_ERR_UNSUPPORTED, emission


@pytest.mark.parametrize("name", PLAIN)
def test_other_entry_points_refuse_it(built_lib, name):
    from psvo_amd import _lib
    lib = _lib.load()
    for emission in (0, 1):
        assert _call(lib, _lib, name, _desc(_lib, 1, emission)) == _lib.PSVO_ERR_INVALID, emission
    for emission in (2, 3, -1):
        assert _call(lib, _lib, name, _desc(_lib, 1, emission)) == _lib.PSVO_ERR_UNSUPPORTED, emission


def test_abi_version_is_unchanged(built_lib):
    from psvo_amd import _lib
    assert _lib.load().psvo_abi_version() == 6
