"""ctypes binding of libpsvo_hip.so (the C ABI declared in include/psvo_hip.h).

The product path has NO fallback: if the shared library is missing or a call returns a
non-zero status this module raises.  Nothing here imports `oracle/`.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PSVO_HIP_LIB") or os.path.join(_HERE, "csrc", "libpsvo_hip.so")

PSVO_OK = 0
PSVO_ERR_INVALID = -1
PSVO_ERR_UNSUPPORTED = -2
PSVO_ERR_HIP = -3
PSVO_TUNE_BSIM_BWD = 1      # psvo_set_tuning keys (include/psvo_hip.h)
PSVO_TUNE_ROWS_BWD = 2
PSVO_TUNE_L2_SPLIT = 3
PSVO_TUNE_SKEW = 4
PSVO_TUNE_WGRAD2 = 5
PSVO_TUNE_FILTER_BWD = 6
PSVO_TUNE_DETERMINISTIC = 8


class PsvoHipError(RuntimeError):
    """A libpsvo_hip entry point returned a non-zero status."""


class psvo_desc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("B", "T", "N", "M", "Dx", "Dy", "H", "resample", "two_q", "bootstrap", "emission", "layers")]


class psvo_mlp(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("W1", "b1", "W2", "b2", "Wh", "bh")]


_P = ctypes.c_void_p
_DESC = ctypes.POINTER(psvo_desc)
_MLP = ctypes.POINTER(psvo_mlp)

# name -> (restype, argtypes); must list every symbol include/psvo_hip.h declares
SIGNATURES = {
    "psvo_abi_version": (ctypes.c_int, []),
    "psvo_status_string": (ctypes.c_char_p, [ctypes.c_int]),
    "psvo_last_hip_error": (ctypes.c_char_p, []),
    "psvo_filter_forward": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 20 + [_P]),
    "psvo_filter_acc_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "psvo_filter_ws_floats": (ctypes.c_longlong, [ctypes.c_int] * 5),
    "psvo_filter_backward": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 18 + [ctypes.c_int] + [_P] * 16),
    "psvo_filter_forward_adaptive": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 20 + [ctypes.c_float, _P, _P, _P] + [_P]),
    "psvo_filter_backward_adaptive": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 18 + [ctypes.c_int] + [_P] * 15
                                      + [_P, _P]),
    "psvo_filter_forward_wobs": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 20 + [_P]),
    "psvo_filter_wobs_ws_floats": (ctypes.c_longlong, [ctypes.c_int] * 5),
    "psvo_filter_backward_wobs": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 31 + [_P]),
    "psvo_filter_backward_wobs_ext": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 18 + [ctypes.c_int, _P, _P] + [_P] * 13
                                      + [_P]),
    "psvo_filter_forward_wobs_adaptive": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 20 + [ctypes.c_float, _P, _P, _P]
                                          + [_P]),
    "psvo_filter_backward_wobs_adaptive": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 31 + [_P, _P]),
    "psvo_filter_forward_wobs_missing": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 20 + [_P]),
    "psvo_filter_backward_wobs_missing": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 31 + [_P]),
    "psvo_filter_forward_wobs_missing_adaptive": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 20
                                                  + [ctypes.c_float, _P, _P, _P] + [_P]),
    "psvo_filter_backward_wobs_missing_adaptive": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 31 + [_P, _P]),
    "psvo_filter_forward_wobs_input": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 20 + [_P, _P] + [_P]),
    "psvo_filter_backward_wobs_input": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 31 + [_P, _P] + [_P]),
    "psvo_filter_forward_wobs_input_adaptive": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 20
                                                + [ctypes.c_float, _P, _P, _P] + [_P, _P] + [_P]),
    "psvo_filter_backward_wobs_input_adaptive": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 31 + [_P] + [_P, _P] + [_P]),
    "psvo_mlp_wgrad_rowbias_blocks": (ctypes.c_int, [ctypes.c_longlong]),
    "psvo_mlp_wgrad_rowbias": (ctypes.c_int, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              _P, _P, _P, _MLP, _P, _P, _P, ctypes.c_int, _P]),
    "psvo_bsim_forward_wobs": (ctypes.c_int, [_DESC] + [_P] * 4 + [_MLP, _MLP, _MLP] + [_P] * 22 + [_P]),
    "psvo_bsim_wobs_blocks": (ctypes.c_int, [ctypes.c_int] * 2),
    "psvo_bsim_wobs_ws_floats": (ctypes.c_longlong, [ctypes.c_int] * 6),
    "psvo_bsim_backward_wobs": (ctypes.c_int, [_DESC] + [_P] * 3 + [_MLP, _MLP, _MLP] + [_P] * 34 + [_P]),
    "psvo_bsim_forward_wobs_missing": (ctypes.c_int, [_DESC] + [_P] * 4 + [_MLP, _MLP, _MLP] + [_P] * 22 + [_P]),
    "psvo_bsim_backward_wobs_missing": (ctypes.c_int, [_DESC] + [_P] * 3 + [_MLP, _MLP, _MLP] + [_P] * 34 + [_P]),
    "psvo_filter_backward_wobs_missing_ext": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 18 + [ctypes.c_int, _P, _P]
                                              + [_P] * 13 + [_P]),
    "psvo_mlp_wgrad_wobs_blocks": (ctypes.c_int, [ctypes.c_longlong]),
    "psvo_mlp_wgrad_wobs": (ctypes.c_int, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           _P, _P, _MLP, _P, _P, ctypes.c_int, _P]),
    "psvo_filter_forward_cov": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 22 + [_P]),
    "psvo_filter_cov_ws_floats": (ctypes.c_longlong, [ctypes.c_int] * 5),
    "psvo_ffbs_smooth": (ctypes.c_int, [_DESC] + [_P] * 12 + [_P]),
    "psvo_ffbs_sample": (ctypes.c_int, [_DESC] + [_P] * 11 + [_P]),
    "psvo_particle_forecast": (ctypes.c_int, [_DESC, ctypes.c_int, _MLP, _MLP] + [_P] * 10 + [_P]),
    "psvo_particle_forecast_missing": (ctypes.c_int, [_DESC, ctypes.c_int, _MLP, _MLP] + [_P] * 10 + [_P]),
    "psvo_particle_forecast_input": (ctypes.c_int, [_DESC, ctypes.c_int, _MLP, _MLP] + [_P] * 10 + [_P, ctypes.c_int] + [_P]),
    "psvo_map_path": (ctypes.c_int, [_DESC, _MLP] + [_P] * 12 + [_P]),
    "psvo_filter_backward_cov": (ctypes.c_int, [_DESC, _MLP, _MLP, _MLP] + [_P] * 39 + [_P]),
    "psvo_bsim_forward_cov": (ctypes.c_int, [_DESC] + [_P] * 4 + [_MLP, _MLP, _MLP] + [_P] * 23 + [_P]),
    "psvo_bsim_backward_cov": (ctypes.c_int, [_DESC] + [_P] * 4 + [_MLP, _MLP, _MLP] + [_P] * 38 + [_P]),
    "psvo_bsimwr_forward_cov": (ctypes.c_int, [_DESC] + [_P] * 4 + [_MLP, _MLP, _MLP] + [_P] * 26 + [_P]),
    "psvo_bsimwr_backward_cov": (ctypes.c_int, [_DESC] + [_P] * 4 + [_MLP, _MLP, _MLP] + [_P] * 42 + [_P]),
    "psvo_bsim_cov_det_ws_floats": (ctypes.c_longlong, [ctypes.c_int] * 5),
    "psvo_bsim_backward_cov_ws": (ctypes.c_int, [_DESC] + [_P] * 4 + [_MLP, _MLP, _MLP] + [_P] * 39 + [_P]),
    "psvo_bsimwr_backward_cov_ws": (ctypes.c_int, [_DESC] + [_P] * 4 + [_MLP, _MLP, _MLP] + [_P] * 43 + [_P]),
    "psvo_mlp_wgrad_blocks": (ctypes.c_int, [ctypes.c_longlong]),
    "psvo_mlp_wgrad": (ctypes.c_int, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      _P, _P, _MLP, _P, _P, ctypes.c_int, _P]),
    "psvo_mlp2_wgrad_blocks": (ctypes.c_int, [ctypes.c_longlong]),
    "psvo_mlp2_wgrad": (ctypes.c_int, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       _P, _P, _MLP, _P, _P, ctypes.c_int, _P]),
    "psvo_bsim_forward": (ctypes.c_int, [_DESC] + [_P] * 4 + [_MLP, _MLP, _MLP] + [_P] * 22 + [_P]),
    "psvo_bsim_blocks": (ctypes.c_int, [_DESC]),
    "psvo_set_tuning": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "psvo_get_tuning": (ctypes.c_int, [ctypes.c_int]),
    "psvo_bsim_acc_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "psvo_bsim_backward": (ctypes.c_int, [_DESC] + [_P] * 3 + [_MLP, _MLP, _MLP] + [_P] * 28),
    "psvo_bsim_backward_fold": (ctypes.c_int, [_DESC] + [_P] * 15),
    "psvo_bsimwr_blocks": (ctypes.c_int, [ctypes.c_int] * 3),
    "psvo_bsimwr_ws_floats": (ctypes.c_longlong, [ctypes.c_int] * 3),
    "psvo_bsimwr_forward": (ctypes.c_int, [_DESC] + [_P] * 3 + [_MLP, _MLP, _MLP] + [_P] * 25 + [_P]),
    "psvo_bsimwr_bwd_ws_floats": (ctypes.c_longlong, [ctypes.c_int] * 4),
    "psvo_bsimwr_backward": (ctypes.c_int, [_DESC] + [_P] * 3 + [_MLP, _MLP, _MLP] + [_P] * 39),
    "psvo_rows_mlp_blocks": (ctypes.c_int, [ctypes.c_longlong]),
    "psvo_rows_mlp_forward": (ctypes.c_int, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _MLP, _P, _P]),
    "psvo_rows_mlp_backward": (ctypes.c_int, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _MLP,
                                              _P, _P, _P, ctypes.c_int, _P]),
    "psvo_dense_wgrad_slices": (ctypes.c_int, [ctypes.c_longlong]),
    "psvo_dense_forward": (ctypes.c_int, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, _P, _P, _P, ctypes.c_int, _P, _P]),
    "psvo_dense_backward": (ctypes.c_int, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P, ctypes.c_int,
                                           _P, _P, _P, ctypes.c_int, _P]),
    "psvo_bilstm_forward": (ctypes.c_int, [ctypes.c_int] * 4 + [_P] * 8 + [_P]),
    "psvo_bilstm_backward": (ctypes.c_int, [ctypes.c_int] * 4 + [_P] * 10 + [_P]),
    "psvo_bilstm_wgrad_fold": (ctypes.c_int, [ctypes.c_int] * 3 + [_P] * 4 + [ctypes.c_int, _P]),
    "psvo_adam_step": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_longlong, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                      ctypes.c_float, ctypes.c_longlong, ctypes.c_float, _P]),
    "psvo_grad_norm_blocks": (ctypes.c_int, [ctypes.c_longlong]),
    "psvo_grad_sumsq": (ctypes.c_int, [_P, ctypes.c_longlong, _P, _P]),
    "psvo_adam_step_guarded": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_longlong, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                              ctypes.c_float, ctypes.c_longlong, ctypes.c_float, ctypes.c_float, ctypes.c_int,
                                              _P, _P, _P]),
    "psvo_reduce_rows": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, _P, ctypes.c_int, _P]),
    "psvo_sigma_forward": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, _P]),
    "psvo_sigma_backward": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int, ctypes.c_int, _P]),
    "psvo_debug_stamp": (ctypes.c_int, [_P, _P]),
    "psvo_selftest_lanes": (ctypes.c_int, [_P, _P, _P]),
    "psvo_selftest_lanes2": (ctypes.c_int, [_P, _P, _P]),
    "psvo_elbo_filter": (ctypes.c_int, [_DESC, _P, _P, _P]),
    "psvo_elbo_bsim": (ctypes.c_int, [_DESC, _P, _P, _P]),
    "psvo_elbo_bsim_mean": (ctypes.c_int, [_DESC, _P, _P, _P]),
    "psvo_elbo_bsim_mean_backward": (ctypes.c_int, [_DESC, _P, _P, _P, _P]),
}

# environment variable -> the psvo_set_tuning key load() sets from it
ENV_TUNING = (
    ("PSVO_BSIM_BWD_VARIANT", PSVO_TUNE_BSIM_BWD),      # A/B measurements (tools/, bench.py --bsim-bwd-variant)
    ("PSVO_SKEW", PSVO_TUNE_SKEW),                      # A/B: phase offset of co-resident workgroups, per cent (0 = off)
    ("PSVO_FILTER_BWD_SCAN", PSVO_TUNE_FILTER_BWD),     # A/B: 0 = the persistent reverse filter kernel instead of the affine scan
    ("PSVO_WGRAD2", PSVO_TUNE_WGRAD2),                  # A/B: two-layer weight gradients on the bf16 matrix instructions (2 / 3 pieces)
    ("PSVO_L2_SPLIT", PSVO_TUNE_L2_SPLIT),              # A/B: two-layer backward-simulation kernels with the half-split chains
    ("PSVO_DETERMINISTIC", PSVO_TUNE_DETERMINISTIC),    # 1: fixed-order sums on the reverse paths (bit-reproducible gradients)
)

_lib = None


def load():
    """Load the library once; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PsvoHipError(
                "libpsvo_hip.so not found at %s -- build it with `python -m psvo_amd.build` "
                "(there is no CPU or PyTorch fallback for the PSVO hot path)" % LIB_PATH)
        # torch owns the device memory and the streams handed to the library, so both must share
        # ONE HIP runtime: import torch first so that its libamdhip64 is the one the loader binds.
        import torch  # noqa: F401
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        for var, key in ENV_TUNING:
            v = os.environ.get(var)
            if v is not None and lib.psvo_set_tuning(key, int(v)) != PSVO_OK:
                raise PsvoHipError("%s=%s is not a valid psvo_set_tuning value" % (var, v))
        _lib = lib
    return _lib


def check(status, what):
    if status != PSVO_OK:
        msg = load().psvo_status_string(status).decode()
        if status == PSVO_ERR_HIP:
            msg += ": " + load().psvo_last_hip_error().decode()
        exc = ValueError if status in (PSVO_ERR_INVALID, PSVO_ERR_UNSUPPORTED) else PsvoHipError
        raise exc("%s failed: %s (status %d)" % (what, msg, status))
