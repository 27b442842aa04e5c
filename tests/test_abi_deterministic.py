"""PSVO_TUNE_DETERMINISTIC (include/psvo_hip.h): the switch round-trips, refuses other values, defaults to 0, is set by the
PSVO_DETERMINISTIC environment variable, and the cov backward simulations refuse the mode without their workspace.  No GPU
needed."""
import ctypes
import os
import subprocess
import sys

from tests import helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_key_value_matches_the_header(built_lib):
    from psvo_amd import _lib
    txt = open(os.path.join(ROOT, "include", "psvo_hip.h")).read()
    assert "#define PSVO_TUNE_DETERMINISTIC 8" in txt
    assert _lib.PSVO_TUNE_DETERMINISTIC == 8


def test_round_trip_and_refusals(built_lib):
    from psvo_amd import _lib
    lib = _lib.load()
    key = _lib.PSVO_TUNE_DETERMINISTIC
    before = lib.psvo_get_tuning(key)          # (0 unless PSVO_DETERMINISTIC is set: the default is the child-process test's)
    assert before in (0, 1)
    with Hh.tuning(key, 1):
        assert lib.psvo_get_tuning(key) == 1
        for bad in (-1, 2):
            assert lib.psvo_set_tuning(key, bad) == _lib.PSVO_ERR_INVALID
            assert lib.psvo_get_tuning(key) == 1
        assert lib.psvo_set_tuning(key, 0) == _lib.PSVO_OK
        assert lib.psvo_get_tuning(key) == 0
        assert lib.psvo_set_tuning(key, 1) == _lib.PSVO_OK
    assert lib.psvo_get_tuning(key) == before


def _child(env_value):
    env = dict(os.environ)
    env.pop("PSVO_DETERMINISTIC", None)
    if env_value is not None:
        env["PSVO_DETERMINISTIC"] = env_value
    code = "from psvo_amd import _lib; print(_lib.load().psvo_get_tuning(_lib.PSVO_TUNE_DETERMINISTIC))"
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


def test_environment_variable_sets_the_key(built_lib):
    r = _child("1")
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[-1] == "1"
    r = _child(None)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[-1] == "0"
    r = _child("2")
    assert r.returncode != 0 and "PSVO_DETERMINISTIC=2" in r.stderr


def test_cov_backward_simulation_needs_its_workspace_in_the_mode(built_lib):
    """psvo_bsim_backward_cov(_ws) / psvo_bsimwr_backward_cov(_ws) under the mode: INVALID without det_ws (checked before any
    other pointer, so null pointers are enough); with the mode off null pointers are INVALID as before"""
    from psvo_amd import _lib
    lib = _lib.load()
    d = _lib.psvo_desc()
    d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = 2, 4, 8, 4, 2, 1, 32
    m = _lib.psvo_mlp()
    mlps = (ctypes.byref(m), ctypes.byref(m), ctypes.byref(m))
    calls = [lambda: lib.psvo_bsim_backward_cov(ctypes.byref(d), *[None] * 4, *mlps, *[None] * 39),
             lambda: lib.psvo_bsimwr_backward_cov(ctypes.byref(d), *[None] * 4, *mlps, *[None] * 43),
             lambda: lib.psvo_bsim_backward_cov_ws(ctypes.byref(d), *[None] * 4, *mlps, *[None] * 40),
             lambda: lib.psvo_bsimwr_backward_cov_ws(ctypes.byref(d), *[None] * 4, *mlps, *[None] * 44)]
    for mode in (0, 1):
        with Hh.tuning(_lib.PSVO_TUNE_DETERMINISTIC, mode):
            for call in calls:
                assert call() == _lib.PSVO_ERR_INVALID


def test_cov_workspace_size(built_lib):
    """psvo_bsim_cov_det_ws_floats = per-workgroup slices (B nblk (2Dx+1) N + B nblk 4Dx), per-wave d sigma_con sums
    (B nblk waves (2Dx+Dy)) and one d bwX per chain (B Dx N); workgroups of 256 / M chains"""
    from psvo_amd import _lib
    lib = _lib.load()
    B, N, M, Dx, Dy = 4, 128, 16, 2, 1
    nblk, nwv = N // 16, 4
    assert lib.psvo_bsim_cov_det_ws_floats(B, N, M, Dx, Dy) == (B * nblk * (2 * Dx + 1) * N + B * nblk * 4 * Dx
                                                                + B * nblk * nwv * (2 * Dx + Dy) + B * Dx * N)
    assert lib.psvo_bsim_cov_det_ws_floats(2, 8, 4, 2, 1) == 2 * 1 * 5 * 8 + 2 * 8 + 2 * 1 * 5 + 2 * 2 * 8    # (one wave)
    assert lib.psvo_bsim_cov_det_ws_floats(0, 8, 4, 2, 1) == 0
