"""The C-ABI library builds, loads without a GPU, and exports every symbol include/psvo_hip.h
declares; argument validation returns status codes before anything touches a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    txt = open(os.path.join(ROOT, "include", "psvo_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(psvo_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_are_exported_and_bound(built_lib):
    from psvo_amd import _lib
    lib = ctypes.CDLL(built_lib)
    names = _declared_symbols()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), "libpsvo_hip.so does not export %s" % n
        assert n in _lib.SIGNATURES, "psvo_amd/_lib.py does not bind %s" % n
    for n in _lib.SIGNATURES:
        assert n in names, "%s is bound but not declared in include/psvo_hip.h" % n


def _declared_parameters():
    """{function: [parameter declarations]} of include/psvo_hip.h, comments stripped as in _declared_symbols()"""
    txt = open(os.path.join(ROOT, "include", "psvo_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(psvo_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        params = " ".join(params.split())
        out[name] = [] if params in ("", "void") else [q.strip() for q in params.split(",")]
    return out


def test_bound_signatures_match_the_header():
    """the hand-counted ctypes argument lists of psvo_amd/_lib.py: as many parameters as include/psvo_hip.h declares for the
    function, each of the matching ctypes type (a miscount would be silent stack garbage at the call)"""
    from psvo_amd import _lib
    declared = _declared_parameters()
    assert sorted(declared) == _declared_symbols()
    assert sorted(declared) == sorted(_lib.SIGNATURES)

    def ctype_of(decl):
        ty = re.sub(r"\bconst\b", " ", decl)
        ty = " ".join(re.sub(r"[A-Za-z_][A-Za-z0-9_]*$", "", ty.strip()).split()).replace(" *", "*")    # (drop the name)
        if ty == "psvo_desc*":
            return ctypes.POINTER(_lib.psvo_desc)
        if ty == "psvo_mlp*":
            return ctypes.POINTER(_lib.psvo_mlp)
        if ty.endswith("*"):
            return ctypes.c_void_p
        return {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float}[ty]
    for name, params in declared.items():
        bound = _lib.SIGNATURES[name][1]
        assert len(bound) == len(params), "%s: the header declares %d parameters, _lib.py binds %d" % (name, len(params), len(bound))
        for i, (decl, ty) in enumerate(zip(params, bound)):
            assert ty is ctype_of(decl), "%s: parameter %d (`%s`) is bound as %s" % (name, i, decl, ty.__name__)


def test_version_and_status_strings(built_lib):
    from psvo_amd import _lib
    lib = _lib.load()
    assert lib.psvo_abi_version() == 6      # (4: psvo_desc.layers, psvo_mlp.Wh / bh, psvo_mlp2_wgrad; 5: dlse of psvo_bsim_backward_fold; 6: *_cov)
    assert lib.psvo_status_string(0) == b"ok"
    assert b"unsupported" in lib.psvo_status_string(_lib.PSVO_ERR_UNSUPPORTED)
    assert lib.psvo_filter_acc_size(2, 1) == 21 and lib.psvo_bsim_acc_size(3, 2) == 23
    import ctypes
    from psvo_amd import ops
    blocks = lambda B, T, N, M, H, Dx, Dy=1: lib.psvo_bsim_blocks(ctypes.byref(ops.make_desc(B, T, N, M, Dx, Dy, H)))
    assert lib.psvo_get_tuning(_lib.PSVO_TUNE_BSIM_BWD) == -1
    assert lib.psvo_set_tuning(_lib.PSVO_TUNE_BSIM_BWD, 0) == 0           # v1 geometry: lane = (chain, half, m)
    assert blocks(32, 200, 128, 16, 32, 2) == 16 and blocks(32, 200, 128, 16, 32, 3) == 8 and blocks(2, 6, 8, 4, 16, 2) == 1
    assert lib.psvo_set_tuning(_lib.PSVO_TUNE_BSIM_BWD, 1) == 0           # v2: 8 chains per 256-thread workgroup at M = 16
    assert blocks(32, 200, 128, 16, 32, 2) == 16 and blocks(32, 200, 128, 16, 32, 3) == 16 and blocks(2, 6, 8, 4, 16, 2) == 1
    assert blocks(64, 1000, 512, 16, 32, 4) == 32                         # (4 GiB per array: v1 geometry)
    assert lib.psvo_set_tuning(_lib.PSVO_TUNE_BSIM_BWD, 7) == _lib.PSVO_ERR_INVALID
    assert lib.psvo_set_tuning(_lib.PSVO_TUNE_BSIM_BWD, -1) == 0
    assert lib.psvo_mlp_wgrad_blocks(10) == 1 and lib.psvo_mlp_wgrad_blocks(10 ** 9) == 1024


def test_invalid_arguments_are_rejected_without_a_device(built_lib):
    from psvo_amd import _lib
    lib = _lib.load()
    d = _lib.psvo_desc()
    d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = 2, 4, 8, 4, 2, 1, 32
    nul = [None] * 20
    st = lib.psvo_filter_forward(ctypes.byref(d), None, None, None, *nul, None)
    assert st == _lib.PSVO_ERR_INVALID
    st = lib.psvo_elbo_filter(ctypes.byref(d), None, None, None)
    assert st == _lib.PSVO_ERR_INVALID
    # psvo_desc.layers outside {0, 1, 2} (three or more hidden layers; garbage from a shorter, older struct): refused by every
    # entry point that dispatches on it, before anything else is looked at -- never the one-layer kernels by default
    for bad in (3, -1, 1 << 20):
        d.layers = bad
        assert lib.psvo_filter_forward(ctypes.byref(d), None, None, None, *nul, None) == _lib.PSVO_ERR_UNSUPPORTED
        assert lib.psvo_bsim_blocks(ctypes.byref(d)) == _lib.PSVO_ERR_UNSUPPORTED
        for name in ("psvo_filter_backward", "psvo_bsim_forward", "psvo_bsim_backward", "psvo_bsimwr_forward",
                     "psvo_bsimwr_backward", "psvo_filter_forward_cov", "psvo_filter_backward_cov", "psvo_bsim_forward_cov",
                     "psvo_bsim_backward_cov", "psvo_bsimwr_forward_cov", "psvo_bsimwr_backward_cov"):
            fn = getattr(lib, name)
            null = lambda ty: 0 if ty in (ctypes.c_int, ctypes.c_longlong) else 0.0 if ty in (ctypes.c_float, ctypes.c_double) else None
            args = [ctypes.byref(d)] + [null(ty) for ty in _lib.SIGNATURES[name][1][1:]]
            assert fn(*args) == _lib.PSVO_ERR_UNSUPPORTED, name
    # the state-dependent-scale filter (output_cov and diag_cov): one hidden layer
    nul_cov = lambda name: [None] * (len(_lib.SIGNATURES[name][1]) - 1)
    for layers, emission, want in ((2, 0, _lib.PSVO_ERR_UNSUPPORTED), (1, 1, _lib.PSVO_ERR_INVALID),
                                   (1, 0, _lib.PSVO_ERR_INVALID)):
        d.layers, d.emission = layers, emission
        for name in ("psvo_filter_forward_cov", "psvo_filter_backward_cov", "psvo_bsim_forward_cov", "psvo_bsim_backward_cov",
                     "psvo_bsimwr_forward_cov", "psvo_bsimwr_backward_cov"):
            assert getattr(lib, name)(ctypes.byref(d), *nul_cov(name)) == want, (name, layers, emission)
    d.layers, d.emission = 1, 0
    # sums | two row sets | pad to 16 bytes | affine-scan records (4 Dx^2 + 4 Dx + 1 floats, rounded up to 4) | per-step partials
    assert lib.psvo_filter_cov_ws_floats(2, 4, 8, 2, 1) == 2 * 5 + 2 * 4 * 2 * 2 * 8 + 4 + 4 * 2 * 28 * 8 + 4 * 2 * 5
    with pytest.raises(ValueError):
        _lib.check(_lib.PSVO_ERR_UNSUPPORTED, "x")
    with pytest.raises(_lib.PsvoHipError):
        _lib.check(_lib.PSVO_ERR_HIP, "x")


def test_shapes_outside_the_envelope_are_unsupported(built_lib):
    """Every entry point that reaches a shape dispatch (psvo_amd/csrc/common.h: pick_dx / pick_dy / pick_h / pick_m), called with
    every pointer set and a descriptor that is valid except for its shape, returns PSVO_ERR_UNSUPPORTED from the dispatcher's
    default arm: nothing ahead of the dispatch touches a device.  A shape INSIDE the lists would launch with host pointers, so
    each shape is asserted to be outside before the call, and the test does not run where a device is present."""
    import itertools
    import torch
    from psvo_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("host-code test: never hands a host pointer to a library that can reach a device")
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    addr = (ctypes.addressof(buf) + 15) & ~15        # one small 16-byte-aligned host buffer behind every pointer
    assert addr + 64 <= ctypes.addressof(buf) + ctypes.sizeof(buf)
    DX, DY, HH, MM = (2, 3, 4), (1, 2), (16, 32, 64), (4, 8, 16, 32)
    plain = ["psvo_filter_forward", "psvo_filter_backward", "psvo_bsim_forward", "psvo_bsim_backward", "psvo_bsimwr_forward",
             "psvo_bsimwr_backward"]
    cov = ["psvo_filter_forward_cov", "psvo_filter_backward_cov", "psvo_bsim_forward_cov", "psvo_bsim_backward_cov",
           "psvo_bsim_backward_cov_ws", "psvo_bsimwr_forward_cov", "psvo_bsimwr_backward_cov", "psvo_bsimwr_backward_cov_ws"]
    fold = ["psvo_bsim_backward_fold"]       # (dispatches on Dx and Dy only)

    def call(name, d):
        types = _lib.SIGNATURES[name][1]
        keep, args = [], [ctypes.byref(d)]
        for i, ty in enumerate(types[1:], 1):
            if ty is ctypes.POINTER(_lib.psvo_mlp):
                m = _lib.psvo_mlp()
                for f, _ in m._fields_:
                    setattr(m, f, addr)
                keep.append(m)
                args.append(ctypes.byref(m))
            elif i == len(types) - 1:
                args.append(None)      # stream
            elif ty is ctypes.c_void_p:
                args.append(ctypes.c_void_p(addr))
            else:
                args.append(1)         # nparts
        return getattr(lib, name)(*args)

    vals = dict(Dx=(1, 5), Dy=(0, 3), H=(8, 48, 128), M=(2, 12, 64))
    calls = 0
    for name in plain + cov + fold:
        has_m, has_h = "filter" not in name and name not in fold, name not in fold
        keys = [k for k in vals if (k != "M" or has_m) and (k != "H" or has_h)]
        for layers in ((1,) if name in cov else (1, 2)):       # (cov: layers = 2 is refused earlier, with the same status)
            cases = [{k: v} for k in keys for v in vals[k]]
            cases += [{k1: vals[k1][0], k2: vals[k2][-1]} for k1, k2 in itertools.combinations(keys, 2)]
            if layers == 2 and has_h:
                cases.append({"H": 16})
            for c in cases:
                d = _lib.psvo_desc()
                d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = 2, 4, 8, 4, 2, 1, 32
                d.resample, d.two_q, d.bootstrap, d.emission, d.layers = 1, 1, 0, 0, layers
                for k, v in c.items():
                    setattr(d, k, v)
                inside = (d.Dx in DX and d.Dy in DY and (not has_h or (d.H in HH and not (layers == 2 and d.H == 16)))
                          and (not has_m or d.M in MM))
                assert not inside, (name, layers, c)
                assert call(name, d) == _lib.PSVO_ERR_UNSUPPORTED, (name, layers, c)
                calls += 1
    assert calls == 300


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from psvo_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.PsvoHipError):
        _lib.load()


@pytest.mark.timeout(900)
def test_no_register_copies_ahead_of_an_exec_restore(built_lib):
    """ISA check of EVERY kernel of the library (tools/exec_restore_check.py): no VGPR <-> AGPR move or scratch access sits
    between the skip target of a divergent region and the `s_or_b64 exec` that ends it -- neither behind the `then` arm
    (`s_and_saveexec_b64` + `s_cbranch_execz`) nor behind the `else` arm of a diamond (`s_xor_b64 exec, exec, sX` +
    `s_cbranch_execz`; hipcc builds such diamonds out of `acc += cond ? v : 0`).  hipcc 7.2 places the copies of a live-range
    split there under register pressure; they then run under the arm's partial EXEC mask, the lanes outside it keep a stale
    copy and read it back later under the full mask -- three two-hidden-layer kernels lost parts of scale gradients that way in
    round 2 (the third, bsim_bwd_kernel<4,2,64,4,16,1>, through the `else` arm, found in round 3).
    Since round 3 every unit is built with the default allocator and no kernel is exempt.
    Parity tests sample the instantiated (Dx, Dy, H, M, threads) combinations; this covers all of them."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("exec_restore_check", os.path.join(ROOT, "tools", "exec_restore_check.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    n, rows = chk.scan([built_lib], verbose=False)
    assert n > 1000, "expected the whole kernel set, scanned %d" % n
    class_a = [(k, a) for _, k, a, _ in rows if a]
    assert not class_a, "register copies ahead of an EXEC restore in: %s" % class_a[:10]
    from psvo_amd import build
    assert build.L2_FLAGS == []          # (default allocator everywhere: nothing is exempt from the check above)


# every psvo_set_tuning key (include/psvo_hip.h): default, accepted values, refused values
TUNING = [
    ("PSVO_TUNE_BSIM_BWD", -1, [-1, 0, 1, 2, 3, 4], [-2, 5, 100]),
    ("PSVO_TUNE_ROWS_BWD", 0, [0, 16, 64], [-1, 1, 8, 32, 128]),
    ("PSVO_TUNE_L2_SPLIT", 0, [0, 1], [-1, 2]),
    ("PSVO_TUNE_SKEW", 0, [0, 1, 50, 100, 1000], [-1, 1001]),
    ("PSVO_TUNE_WGRAD2", 0, [0, 2, 3], [-1, 1, 4]),
    ("PSVO_TUNE_FILTER_BWD", 1, [0, 1, 2], [-1, 3]),
]


@pytest.mark.parametrize("name,default,good,bad", TUNING, ids=[t[0] for t in TUNING])
def test_tuning_round_trip_and_refusals(built_lib, name, default, good, bad):
    """set / get round trip of every accepted value; a refused value returns PSVO_ERR_INVALID and leaves the setting as it
    was; tests.helpers.tuning restores the previous value even when its block raises"""
    from psvo_amd import _lib
    from tests import helpers as Hh
    lib = _lib.load()
    key = getattr(_lib, name)
    assert lib.psvo_get_tuning(key) == default
    try:
        for v in good:
            assert lib.psvo_set_tuning(key, v) == _lib.PSVO_OK, v
            assert lib.psvo_get_tuning(key) == v
            for w in bad:
                assert lib.psvo_set_tuning(key, w) == _lib.PSVO_ERR_INVALID, w
                assert lib.psvo_get_tuning(key) == v
    finally:
        assert lib.psvo_set_tuning(key, default) == _lib.PSVO_OK
    with pytest.raises(RuntimeError):
        with Hh.tuning(key, good[-1]):
            assert lib.psvo_get_tuning(key) == good[-1]
            raise RuntimeError("inside")
    assert lib.psvo_get_tuning(key) == default
    with pytest.raises(AssertionError):
        with Hh.tuning(key, bad[0]):
            pass
    assert lib.psvo_get_tuning(key) == default


def test_tuning_unknown_keys_are_refused(built_lib):
    from psvo_amd import _lib
    lib = _lib.load()
    for key in (0, 7, -1, 1 << 20):
        assert lib.psvo_set_tuning(key, 0) == _lib.PSVO_ERR_INVALID, key
        assert lib.psvo_get_tuning(key) == _lib.PSVO_ERR_INVALID, key
