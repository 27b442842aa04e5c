"""The marginal particle smoother (--FFBS) as far as it can be checked without a GPU: the reference restatement the GPU tests
compare against (tests/ffbs_reference.py) agrees with an independent dense computation in the probability domain, and the
flag is parsed, defaults to off and is refused for the objectives that already smooth."""
import math

import pytest
import torch

from tests import ffbs_reference as R


def _system(T, B, Dx, N, sig, cov, seed):
    """particles scattered around a random walk, transition means near them, scales `sig` (per particle when `cov`)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    X = torch.cumsum(0.3 * rn(T, B, Dx, 1), 0) + 2 * sig * rn(T, B, Dx, N)
    Fm = X + 0.1 * torch.tanh(X) + 0.05 * rn(T, B, Dx, N)
    S = torch.full((T, B, Dx, N), sig, dtype=torch.float64)
    if cov:
        S = S * (0.5 + torch.rand(T, B, Dx, N, generator=g, dtype=torch.float64))
    logW = -3.0 + 1.5 * rn(T, B, N)
    return X, Fm, S, logW


def test_restatement_matches_dense_probability_domain():
    """w_{t|T} = Bk^T w_{t+1|T} with Bk[j,k] = w_t[k] f(j|k) / sum_l w_t[l] f(j|l), explicit matrices, no logarithm anywhere"""
    T, B, Dx, N = 4, 2, 2, 5
    X, Fm, S, logW = _system(T, B, Dx, N, 0.7, True, seed=11)
    got = R.smooth(X, Fm, S, logW).exp()
    w = torch.exp(logW)
    w = w / w.sum(-1, keepdim=True)
    for b in range(B):
        sm = w[T - 1, b].clone()
        assert torch.allclose(got[T - 1, b], sm, rtol=0, atol=1e-12)
        for t in range(T - 2, -1, -1):
            f = torch.ones(N, N, dtype=torch.float64)                  # f[j, k] = N(X[t+1][j]; Fm[t][k], S[t][k])
            for j in range(N):
                for k in range(N):
                    for d in range(Dx):
                        z = (X[t + 1, b, d, j] - Fm[t, b, d, k]) / S[t, b, d, k]
                        f[j, k] *= torch.exp(-0.5 * z * z) / (S[t, b, d, k] * math.sqrt(2 * math.pi))
            Bk = w[t, b].unsqueeze(0) * f
            Bk = Bk / Bk.sum(1, keepdim=True)
            sm = Bk.t() @ sm
            assert torch.allclose(got[t, b], sm, rtol=0, atol=1e-12), (b, t)


@pytest.mark.parametrize("shape", [(1, 1, 2, 8, 1.0, False), (2, 2, 2, 12, 1.0, False), (6, 2, 3, 100, 1.0, False),
                                   (7, 2, 2, 130, 0.3, True), (40, 2, 2, 64, 0.05, False)],
                         ids=lambda s: "-".join(map(str, s)))
def test_restatement_sums_to_one_and_ends_at_the_filter_weights(shape):
    T, B, Dx, N, sig, cov = shape
    X, Fm, S, logW = _system(T, B, Dx, N, sig, cov, seed=3)
    lw = R.smooth(X, Fm, S, logW)
    assert torch.isfinite(lw).all()
    assert float((lw.exp().sum(-1) - 1).abs().max()) <= 1e-12
    assert torch.equal(lw[T - 1], logW[T - 1] - torch.logsumexp(logW[T - 1], -1, keepdim=True))
    xm, ess = R.moments(lw, X)
    assert xm.shape == (T, B, Dx) and ess.shape == (T, B)
    assert float(ess.min()) >= 1 - 1e-9 and float(ess.max()) <= N + 1e-9


def test_reference_draw_is_the_inverse_cdf_draw():
    from oracle import psvo_oracle as O
    T, B, Dx, N = 5, 2, 2, 12
    lw = R.smooth(*_system(T, B, Dx, N, 1.0, False, seed=5))
    u = torch.rand(T, B, N, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    idx = R.draw(lw, u)
    d = O.draw_distance(lw.reshape(T * B, N).t(), u.reshape(T * B, N).t(), idx.reshape(T * B, N).t())
    assert float(d.max()) == 0.0


def test_flag():
    from psvo_amd.flags import Flags, parse_flags
    assert Flags().FFBS is False
    assert parse_flags([]).FFBS is False
    assert parse_flags(["--FFBS"]).FFBS is True
    assert parse_flags(["--FFBS", "--noFFBS"]).FFBS is False
    assert parse_flags(["--FFBS=true"]).FFBS is True
    assert Flags(FFBS=True).as_dict()["FFBS"] is True


@pytest.mark.parametrize("argv", [["--PSVO", "--FFBS"], ["--PSVOwR", "--FFBS"], ["--noPSVO", "--PSVOwR", "--FFBS"]])
def test_runner_refuses_ffbs_for_the_smoothing_objectives(argv, monkeypatch):
    """ValueError ahead of everything else: no device is looked for, nothing is built"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags

    def no_device():
        raise AssertionError("the device was touched before --FFBS was refused")
    monkeypatch.setattr(runner, "_device", no_device)
    with pytest.raises(ValueError, match="FFBS"):
        runner.main(parse_flags(argv))


def test_objectives_carry_the_flag():
    """the objective reads FLAGS.FFBS once; a FLAGS object without the attribute (older callers) means off"""
    from psvo_amd.SMC.SVO import SVO
    from tests import helpers as Hh

    class _Model:
        q0_dist = q1_dist = q2_dist = f_dist = g_dist = None
    assert SVO(_Model(), Hh.make_flags("SVO", FFBS=True)).FFBS is True
    assert SVO(_Model(), Hh.make_flags("SVO")).FFBS is False
    F = Hh.make_flags("SVO")
    del F.FFBS
    assert SVO(_Model(), F).FFBS is False
