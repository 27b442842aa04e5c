"""Host side of the count emission (FLAGS.count_emission): flag, routing, refusals, the loader's check of the data, the
generator's count emitter and the torch log-density.  No GPU."""
import math

import numpy as np
import pytest
import torch

from tests import helpers as Hh


def _objective(obj, **kw):
    from psvo_amd.model import SSM
    from psvo_amd.SMC.AESMC import AESMC
    from psvo_amd.SMC.PSVO import PSVO
    from psvo_amd.SMC.PSVOwR import PSVOwR
    from psvo_amd.SMC.SVO import SVO
    FLAGS = Hh.make_flags(obj, **kw)
    model = SSM(FLAGS)
    return FLAGS, model, {"AESMC": AESMC, "PSVO": PSVO, "PSVOwR": PSVOwR, "SVO": SVO}[obj](model, FLAGS)


def test_flag_parsing():
    from psvo_amd.flags import Flags, parse_flags
    assert Flags().count_emission is False
    F = parse_flags(["--count_emission", "--Dy=10"])
    assert F.count_emission is True and F.poisson_emission is False and F.Dy == 10
    assert parse_flags(["--count_emission=false"]).count_emission is False
    assert parse_flags(["--count_emission", "--nocount_emission"]).count_emission is False
    assert "count_emission" in Flags().as_dict()


def test_routing_makes_emission_2():
    from psvo_amd.distribution.poisson import count_poisson
    for obj, kw in (("AESMC", {}), ("PSVO", dict(BSim_wide_obs=True))):
        FLAGS, model, smc = _objective(obj, count_emission=True, Dx=3, Dy=10, n_particles=8, **kw)
        assert smc.wide_obs and isinstance(model.g_dist, count_poisson)
        assert not any("g_dist.sigma" in n for n, _ in model.named_parameters())
        assert "sigma_raw" not in model.export_reference_layout()["g"]
        smc.batch_size, smc.time = 2, 5
        assert smc._make_desc(4, 32).emission == 2
    for kw, want in ((dict(poisson_emission=True), 1), ({}, 0)):
        FLAGS, model, smc = _objective("AESMC", Dx=3, Dy=10, **kw)
        smc.batch_size, smc.time = 2, 5
        assert smc._make_desc(1, 32).emission == want


@pytest.mark.parametrize("obj,kw,word", [
    ("AESMC", dict(count_emission=True, poisson_emission=True, Dy=10), r"--count_emission with --poisson_emission"),
    ("AESMC", dict(count_emission=True, Dy=2), r"Dy = 2.*3 <= Dy <= 32.*plain kernels.*no count form"),
    ("PSVO", dict(count_emission=True, BSim_wide_obs=True, Dy=1), r"Dy = 1.*3 <= Dy <= 32.*plain kernels.*no count form"),
    ("PSVO", dict(count_emission=True, Dy=3), r"Dy = 3 with PSVO / PSVOwR.*Dy <= 2"),
    ("PSVOwR", dict(count_emission=True, BSim_wide_obs=True, Dy=3), "PSVOwR"),
    ("AESMC", dict(count_emission=True, Dy=3, output_cov=True, diag_cov=True), "output_cov"),
    ("AESMC", dict(count_emission=True, Dy=3, q1_layers="32,32", g_layers="32,32"), "one hidden layer"),
    ("AESMC", dict(count_emission=True, Dy=33), r"Dy = 33.*3 <= Dy <= 32"),
], ids=["both-flags", "Dy2", "Dy1-PSVO", "PSVO-no-flag", "PSVOwR", "output_cov", "two-layers", "Dy33"])
def test_refusals(obj, kw, word):
    with pytest.raises(ValueError, match=word):
        _objective(obj, **kw)


def test_loader_checks_the_counts(monkeypatch):
    from psvo_amd import runner
    from psvo_amd.flags import Flags
    good = np.random.RandomState(0).poisson(2.0, size=(3, 7, 4)).astype(np.float64)
    runner.check_counts(good)
    neg = good.copy()
    neg[1, 2, 3] = -2.0
    with pytest.raises(ValueError, match=r"obs_train holds negative values \(minimum -2\.0\)"):
        runner.check_counts(neg, "obs_train")
    frac = good.copy()
    frac[2, 0, 1] = 1.5
    frac[2, 5, 0] = 0.25
    with pytest.raises(ValueError, match=r"obs_test holds non-integer values \(first: 1\.5 at index \(2, 0, 1\)\)"):
        runner.check_counts(frac, "obs_test")
    bad = good.copy()
    bad[0, 0, 0] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        runner.check_counts(bad)
    # _dataset runs the check under the flag, once per split, and only under the flag
    hid = np.zeros((3, 7, 2))
    monkeypatch.setattr(runner, "load_data", lambda *a, **k: (hid, hid, good, frac))
    F = Flags(count_emission=True, Dy=4)
    with pytest.raises(ValueError, match="obs_test holds non-integer"):
        runner._dataset(F)
    monkeypatch.setattr(runner, "load_data", lambda *a, **k: (hid, hid, neg, good))
    with pytest.raises(ValueError, match="obs_train holds negative"):
        runner._dataset(Flags(count_emission=True, Dy=4))
    assert runner._dataset(Flags(Dy=4))[2] is neg
    monkeypatch.setattr(runner, "load_data", lambda *a, **k: (hid, hid, good, good))
    assert runner._dataset(Flags(count_emission=True, Dy=4))[3] is good


def test_count_emitter():
    from psvo_amd.utils.data_generator import PoissonEmitter, count_loading, generate_dataset
    C, d = count_loading(10)
    assert C.shape == (10, 2) and np.allclose(C[0], [1.0, 0.0]) and np.allclose(d, 1.0)
    k = 3
    assert np.allclose(C[k], [math.cos(2 * math.pi * k / 10), math.sin(2 * math.pi * k / 10)])
    assert count_loading(10, 3).__getitem__(0).shape == (10, 3) and np.all(count_loading(10, 3)[0][:, 2] == 0)
    g = PoissonEmitter(C, d)
    x = np.array([0.7, -1.2])
    assert np.allclose(g.rate(x), np.log1p(np.exp(C @ x + 1.0)))
    # draws: integers from numpy's global generator, reproduced by its seed
    np.random.seed(11)
    a = np.stack([g.sample(x) for _ in range(4000)])
    np.random.seed(11)
    b = np.stack([g.sample(x) for _ in range(4000)])
    assert np.array_equal(a, b) and np.array_equal(a, np.floor(a)) and a.min() >= 0
    lam = g.rate(x)
    assert np.all(np.abs(a.mean(0) - lam) <= 5 * np.sqrt(lam / 4000))          # five standard errors of a Poisson mean
    assert np.all(np.abs(a.var(0) - lam) <= 0.2 * lam + 0.05)                   # variance equal to the mean
    # as g= of generate_dataset; the runner's generated data
    np.random.seed(3)
    ht, hv, yt, yv = generate_dataset(2, 1, 6, model="fhn", Dy=10, g=g)
    assert yt.shape == (2, 6, 10) and yv.shape == (1, 6, 10) and np.array_equal(yt, np.floor(yt)) and yt.min() >= 0
    from psvo_amd import runner
    from psvo_amd.flags import Flags
    np.random.seed(3)
    data = runner._dataset(Flags(generateTrainingData=True, count_emission=True, Dy=10, n_train=2, n_test=1, time=6))
    assert np.array_equal(data[2], yt) and np.array_equal(data[3], yv)


def test_log_prob_is_the_poisson_pmf():
    from psvo_amd.distribution.poisson import count_poisson, tf_poisson
    from tests import count_reference as CR
    FLAGS, model, smc = _objective("AESMC", count_emission=True, Dx=3, Dy=5)
    torch.manual_seed(2)
    Hh.perturb_(model)
    g = model.g_dist
    assert isinstance(g, count_poisson) and isinstance(g, tf_poisson)
    assert torch.equal(g.get_sigma(), torch.ones(5))
    x = torch.randn(6, 4, 3, dtype=torch.float64) * 2
    y = CR.counts(6, 4, 5, 9)
    y[0, 0] = torch.tensor([0.0, 1.0, 50.0, 1000.0, 10000.0], dtype=torch.float64)
    model.double()
    lam = g.mean(x)
    assert lam.shape == (6, 4, 5) and float(lam.detach().min()) > 0
    want = torch.nn.functional.softplus(model.g_tran.transform(x)[0]) + 1e-6
    assert torch.equal(lam, want)
    lp = g.log_prob(x, y)
    assert lp.shape == (6, 4)
    closed = (y * lam.log() - lam - torch.lgamma(y + 1)).sum(-1)
    assert torch.allclose(lp, closed, rtol=1e-14, atol=1e-12)
    # the fp64 reference the GPU tests use is the same function
    ref = CR.CountEmission(model.export_reference_layout(torch.float64)["g"])
    assert torch.allclose(ref.log_prob(x, y), lp, rtol=1e-13, atol=1e-11)
    assert torch.allclose(ref.mean(x), lam, rtol=1e-14)
    # differentiable, and the gradient reaches the emission network
    lp.sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in model.g_tran.parameters())
    stats = pytest.importorskip("scipy.stats")
    pmf = stats.poisson.logpmf(y.numpy(), lam.detach().numpy()).sum(-1)
    assert np.allclose(lp.detach().numpy(), pmf, rtol=1e-10, atol=1e-9)
