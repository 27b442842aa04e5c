"""The order and the stream of the native launches the host layer issues, arm by arm, against tests/golden/launch_order.json.

A change of the Python host layer (psvo_amd/autograd.py, ops.py, SMC/*.py) can leave every value as it was and still move a
launch to another place or another stream: the captured training step then has another topology (see ops.sum_chain_rows,
autograd.PRELAUNCH / DEFER_BSIM_WGRAD and the `split` cross-wait in FilterFunction.backward for what that has cost).  Every arm
runs one evaluation (training arms: and one reverse pass) under a timing hook that only writes down (entry point, phase,
stream role) of every marked launch, and the whole list must equal the recorded one.

The fixture is recorded by this module, `python -m tests.test_gpu_launch_order --record [path]`, on the commit BEFORE a
host-layer change and is not regenerated from the changed tree: if this test fails, the change is wrong, not the fixture.
"""
import contextlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_order.json")

_SVO = ("SVO", 2, 6, 16, 1, 2, 1, 16, True, True)
_SVO_WIDE = ("SVO", 2, 6, 16, 1, 2, 3, 16, True, True)
_PSVO = ("PSVO", 2, 6, 8, 4, 2, 1, 16, True, True)
_PSVOWR = ("PSVOwR", 2, 6, 8, 4, 2, 1, 16, True, True)
_COV = dict(output_cov=True, diag_cov=True)

# arm -> (case (obj, B, T, N, M, Dx, Dy, H, bootstrap, two_q), extra flags, mode)
#   "autograd": get_log_ZSMC(...)[0].backward(), gradients returned through autograd
#   "trainer" : the trainer's local step -- optim.FlatParams (weight gradients accumulated in place by the kernels: gbufs, the
#               second side stream, the deferred weight gradients) and autograd.deferred_join()
#   "eval"    : under torch.no_grad(), followed by smc.particle_forecast(3, log["Xs"], obs)
ARMS = {
    "svo": (_SVO, {}, "autograd"),
    "svo+mlp_f": (("SVO", 2, 6, 12, 1, 3, 1, 32, False, False), {}, "autograd"),
    "aesmc+two_layers": (("AESMC", 2, 6, 16, 1, 2, 1, 32, True, True), dict(q1_layers="32,32", g_layers="32,32"), "autograd"),
    "iwae": (("IWAE", 2, 5, 12, 1, 2, 1, 16, True, False), {}, "autograd"),
    "psvo": (_PSVO, {}, "autograd"),
    "psvowr": (_PSVOWR, {}, "autograd"),
    "psvo+padded": (_PSVO, dict(q1_layers="24"), "autograd"),
    "psvo+trainer": (_PSVO, {}, "trainer"),
    "psvowr+trainer": (_PSVOWR, {}, "trainer"),
    "psvo+padded+trainer": (_PSVO, dict(q1_layers="24"), "trainer"),
    "svo+wide": (_SVO_WIDE, {}, "autograd"),
    "psvo+wide": (("PSVO", 2, 6, 8, 4, 2, 3, 16, True, True), dict(BSim_wide_obs=True), "autograd"),
    "svo+adaptive": (_SVO, dict(resample_ess=0.5), "autograd"),
    "svo+wide+adaptive": (_SVO_WIDE, dict(resample_ess=0.5, resample_ess_wide_obs=True), "autograd"),
    "svo+cov": (_SVO, _COV, "autograd"),
    "psvo+cov": (_PSVO, _COV, "autograd"),
    "psvowr+cov": (_PSVOWR, _COV, "autograd"),
    "svo+eval": (_SVO, dict(FFBS=True, FFBSi=True), "eval"),
}


@contextlib.contextmanager
def _default_wiring():
    """the module switches of psvo_amd.autograd at their defaults, whatever the environment or an earlier test left"""
    from psvo_amd import autograd
    want = dict(OVERLAP=True, DEFER_JOIN=False, PRELAUNCH=True, DEFER_BSIM_WGRAD=True, SPLIT_FILTER_WGRAD=False,
                SPLIT_CROSS_WAIT=False)
    prev = {k: getattr(autograd, k) for k in want}
    for k, v in want.items():
        setattr(autograd, k, v)
    try:
        yield
    finally:
        for k, v in prev.items():
            setattr(autograd, k, v)


def record(arm):
    """[[entry point, phase, stream role], ...] of one run of `arm`"""
    from psvo_amd import autograd, ops
    from psvo_amd.optim import FlatParams
    from tests import helpers as Hh
    from tests.test_gpu_parity import _setup
    case, extra, mode = ARMS[arm]
    FLAGS, model, smc, obs, noise = _setup(*case, seed=4, **extra)
    nz = Hh.noise_to_hip(noise, "cuda")
    obs_c = obs.float().cuda()
    flat = FlatParams(model) if mode == "trainer" else None
    side = {autograd.side_stream(obs_c.device).cuda_stream: "side", autograd.side_stream(obs_c.device, 1).cuda_stream: "side2"}
    seen = []

    def hook(name, phase, stream):
        if stream.cuda_stream == torch.cuda.current_stream().cuda_stream:
            role = "main"
        else:
            role = side.get(stream.cuda_stream, "unknown stream %#x" % stream.cuda_stream)
        seen.append([name, int(phase), role])
    prev = ops._HOOK
    ops.set_timing_hook(hook)
    try:
        with _default_wiring():
            if mode == "eval":
                with torch.no_grad():
                    _, log = smc.get_log_ZSMC(obs_c, None, noise=nz)
                    smc.particle_forecast(3, log["Xs"], obs_c)
            elif mode == "trainer":
                flat.zero_grad()
                z, _ = smc.get_log_ZSMC(obs_c, None, noise=nz)
                with autograd.deferred_join():
                    z.backward()
            else:
                smc.get_log_ZSMC(obs_c, None, noise=nz)[0].backward()
    finally:
        ops.set_timing_hook(prev)
    torch.cuda.synchronize()
    return seen


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_fixture_covers_every_arm(recorded):
    assert sorted(recorded) == sorted(ARMS)


@pytest.mark.parametrize("arm", sorted(ARMS))
def test_launch_order(built_lib, recorded, arm):
    got = record(arm)
    roles = {r for _, _, r in got}
    assert roles <= {"main", "side", "side2"}, roles
    want = recorded[arm]
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, "launch %d of %d / %d: got %s, recorded %s" % (first, len(got), len(want), got[first:first + 3],
                                                                      want[first:first + 3])


if __name__ == "__main__":
    # --record [path]: write the fixture from THIS tree (every arm twice: what only a process's first run launches must not
    # get into it)
    if len(sys.argv) < 2 or sys.argv[1] != "--record":
        sys.exit("usage: python -m tests.test_gpu_launch_order --record [path]")
    out = {}
    for name in sorted(ARMS):
        first, out[name] = record(name), record(name)
        assert first == out[name], "%s: two runs of one tree disagree" % name
        assert {r for _, _, r in out[name]} <= {"main", "side", "side2"}, name
        print("%-22s %3d marks  %s" % (name, len(out[name]), sorted({r for _, _, r in out[name]})), flush=True)
    path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    with open(path, "w") as fh:
        fh.write("{\n%s\n}\n" % ",\n".join('"%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in out.items()))
