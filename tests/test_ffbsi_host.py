"""The backward sampler (--FFBSi) as far as it can be checked without a GPU: the reference restatement the GPU tests compare
against (tests/ffbsi_reference.py) run in fp32 against itself in fp64 on the GPU tests' inputs, and the flag is parsed, defaults
to off and is refused for the objectives that already return trajectories."""
import pytest
import torch

from tests import ffbsi_reference as R

EDGE_TOL = 5e-6            # (tests/test_gpu_large.py: a flipped draw needs u within this of a CDF edge)
CASES = R.cases()


@pytest.mark.parametrize("shape,masked", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_restatement_fp32_against_fp64(shape, masked):
    """forced indices: the fp32 log-probabilities are within 1e-4 of fp64 (the GPU test's yardstick err_32; at most 7.4e-5 on
    these inputs).  Free-running: every fp32 draw is the draw fp64 arithmetic makes given the chain's own successors, and no
    particle of weight zero is drawn."""
    T, B, Dx, N = shape[:4]
    c = R.case(shape, masked)
    f64, f32, free = c["forced64"], c["forced32"], c["free32"]
    assert torch.equal(f64["idx"], c["idx_in"].long()) and torch.equal(f32["idx"], f64["idx"])
    assert torch.equal(f32["Xs"], R.gather(c["X"], c["idx_in"])) and torch.equal(f32["distinct"], f64["distinct"])
    err_32, biggest = R.forced_error(f32["logq"], f64["logq"])
    print("ffbsi-reference %s err_32 %.3e max|logq_64| %.1f" % ("-".join(map(str, shape)), err_32, biggest))
    assert err_32 <= 1e-4
    assert masked or torch.isfinite(f64["logq"]).all()
    assert float(f64["logq"].max()) <= 1e-12                              # a log-probability
    d = R.draw_distances(c["X"], c["Fm"], c["S"], c["logW"], c["u"], free["idx"])
    assert float(d.max()) == 0.0
    assert torch.isfinite(torch.gather(c["logW"], 2, free["idx"])).all()
    assert int(free["idx"].min()) >= 0 and int(free["idx"].max()) < N
    assert int(free["distinct"].min()) >= 1 and int(free["distinct"].max()) <= N
    if masked:
        assert float(c["u"].max()) <= 0.9989 + 1e-4 and int(free["distinct"].max()) <= N - (N + 2) // 3
    # the probabilities of a step sum to one: teacher-force every index in turn at the last step (T - 1: no successor)
    if N <= 12:
        lw = c["logW"].double()
        tot = torch.zeros(B, N, dtype=torch.float64)
        for k in range(N):
            forced = c["idx_in"].clone()
            forced[T - 1] = k
            q = R.sample(c["X"].double(), c["Fm"].double(), c["S"].double(), lw, idx_in=forced)["logq"][T - 1]
            tot += q.exp()
        assert float((tot - 1).abs().max()) <= 1e-12


def test_distinct_counts_different_values():
    idx = torch.tensor([[[0, 0, 0, 0], [3, 1, 3, 2]], [[2, 2, 1, 1], [0, 1, 2, 3]]])
    assert R.distinct(idx).tolist() == [[1, 3], [2, 4]]


def test_flag():
    from psvo_amd.flags import Flags, parse_flags
    assert Flags().FFBSi is False
    assert parse_flags([]).FFBSi is False
    assert parse_flags(["--FFBSi"]).FFBSi is True and parse_flags(["--FFBSi"]).FFBS is False
    assert parse_flags(["--FFBS"]).FFBSi is False
    assert parse_flags(["--FFBSi", "--noFFBSi"]).FFBSi is False
    assert parse_flags(["--FFBSi=true"]).FFBSi is True
    assert Flags(FFBSi=True).as_dict()["FFBSi"] is True


@pytest.mark.parametrize("argv", [["--PSVO", "--FFBSi"], ["--PSVOwR", "--FFBSi"], ["--noPSVO", "--PSVOwR", "--FFBSi"]])
def test_runner_refuses_ffbsi_for_the_smoothing_objectives(argv, monkeypatch):
    """ValueError ahead of everything else: no device is looked for, nothing is built"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags

    def no_device():
        raise AssertionError("the device was touched before --FFBSi was refused")
    monkeypatch.setattr(runner, "_device", no_device)
    with pytest.raises(ValueError, match="FFBSi"):
        runner.main(parse_flags(argv))


def test_objectives_carry_the_flag():
    """the objective reads FLAGS.FFBSi once; a FLAGS object without the attribute (older callers) means off"""
    from psvo_amd.SMC.SVO import SVO
    from tests import helpers as Hh

    class _Model:
        q0_dist = q1_dist = q2_dist = f_dist = g_dist = None
    assert SVO(_Model(), Hh.make_flags("SVO", FFBSi=True)).FFBSi is True
    assert SVO(_Model(), Hh.make_flags("SVO")).FFBSi is False
    F = Hh.make_flags("SVO")
    del F.FFBSi
    assert SVO(_Model(), F).FFBSi is False

