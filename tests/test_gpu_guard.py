"""The gradient guard on the GPU (include/psvo_hip.h: psvo_grad_sumsq + psvo_adam_step_guarded; psvo_amd.optim.TFAdam with
clip_norm / skip_nonfinite; the trainer's --clip_norm and --skip_nonfinite_steps): the norm against torch in fp64, bit identity
with psvo_adam_step whenever neither clip nor skip fires, the clipped update against the fp64 Adam formula, skipped steps that
touch nothing, run-to-run reproducibility, the committed ill-conditioned state, and the trainer end to end."""
import ctypes
import glob
import math
import os
import pickle

import numpy as np
import pytest
import torch

from tests import helpers as Hh

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 3e-3, 0.9, 0.999, 1e-8
APPLIED, CLIPPED, SKIPPED, CONSEC, LAST, LARGEST = range(6)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from psvo_amd import _lib
    return _lib, _lib.load()


def _slice(n, G):
    """floats per workgroup of psvo_grad_sumsq (the header's S)"""
    return (-(-n // G) + 3) // 4 * 4


def _sumsq(g):
    L, lib = _lib()
    G = lib.psvo_grad_norm_blocks(g.numel())
    partial = torch.full((G,), -1.0, device="cuda", dtype=torch.float64)
    L.check(lib.psvo_grad_sumsq(_p(g), g.numel(), _p(partial), _stream()), "psvo_grad_sumsq")
    return partial


class _Adam:
    """params / m / v of one flat vector, stepped through the raw C entry points"""

    def __init__(self, p0):
        self.p, self.m, self.v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        self.n = p0.numel()
        self.state = torch.zeros(8, device="cuda", dtype=torch.float64)
        self.partial = torch.zeros(_lib()[1].psvo_grad_norm_blocks(self.n), device="cuda", dtype=torch.float64)

    def plain(self, g, step, scale=-1.0):
        L, lib = _lib()
        L.check(lib.psvo_adam_step(_p(self.p), _p(g), _p(self.m), _p(self.v), self.n, LR, B1, B2, EPS, step, scale, _stream()),
                "psvo_adam_step")

    def guarded(self, g, step, clip, skip, scale=-1.0):
        L, lib = _lib()
        L.check(lib.psvo_grad_sumsq(_p(g), self.n, _p(self.partial), _stream()), "psvo_grad_sumsq")
        L.check(lib.psvo_adam_step_guarded(_p(self.p), _p(g), _p(self.m), _p(self.v), self.n, LR, B1, B2, EPS, step, scale,
                                           clip, int(skip), _p(self.partial), _p(self.state), _stream()),
                "psvo_adam_step_guarded")

    def bits(self):
        torch.cuda.synchronize()
        return [t.view(torch.int32).cpu().clone() for t in (self.p, self.m, self.v)]

    def stats(self):
        return self.state.cpu().tolist()


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [True, False], ids=["with1e25", "plain"])
@pytest.mark.parametrize("n", [1, 255, 22426, 1000003])
def test_norm_matches_torch_fp64(built_lib, n, big):
    """sum of squares in double: only the final roundings are left, relative error <= 1e-6 -- also with entries of 1e25, whose
    squares (1e50) an fp32 sum could not hold; every workgroup's partial is the sum over the slice the header names"""
    g = torch.randn(n, generator=torch.Generator().manual_seed(n))
    if big:
        for i in sorted({0, n // 2, n - 1}):
            g[i] = 1e25 if i % 2 == 0 else -1e25
    want = g.double().pow(2).sum().sqrt().item()
    if big:
        assert not math.isfinite(g.pow(2).sum().item())             # (the fp32 sum of squares does overflow)
    gd = g.cuda()
    partial = _sumsq(gd).cpu()
    G, S = partial.numel(), _slice(n, partial.numel())
    got = partial.sum().sqrt().item()
    print("n=%d big=%s norm %.9e torch fp64 %.9e rel %.2e" % (n, big, got, want, abs(got - want) / want))
    assert abs(got - want) <= 1e-6 * want
    for k in range(G):
        w = g[k * S:(k + 1) * S].double().pow(2).sum().item()
        assert abs(partial[k].item() - w) <= 1e-11 * max(w, 1e-300)      # (both are double sums of <= 4096 exact products), (k, partial[k].item(), w)
    # a gradient vector that does not start on a 16-byte boundary takes the scalar loop: same slices, same contract
    buf = torch.zeros(n + 1, device="cuda")
    buf[1:].copy_(gd)
    off = _sumsq(buf[1:]).cpu()
    assert abs(off.sum().sqrt().item() - want) <= 1e-6 * want
    # and the norm the guarded step records is |grad_scale| * that
    a = _Adam(torch.zeros(n, device="cuda"))
    a.guarded(gd, 1, 0.0, 0, scale=-0.5)
    st = a.stats()
    assert abs(st[LAST] - 0.5 * want) <= 1e-6 * 0.5 * want and st[LARGEST] == st[LAST] and st[APPLIED] == 1


@pytest.mark.parametrize("clip,skip", [(1e30, 1), (0.0, 1), (1e30, 0), (0.0, 0)])
@pytest.mark.parametrize("n", [255, 22426, 1000003])
def test_bit_identical_to_plain_adam_when_nothing_fires(built_lib, n, clip, skip):
    gen = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=gen).cuda()
    a, b = _Adam(p0), _Adam(p0)
    for t in range(1, 6):
        g = (torch.randn(n, generator=gen) * 10.0 ** (t - 3)).cuda()
        a.plain(g, t, scale=-0.5)
        b.guarded(g, t, clip, skip, scale=-0.5)
        assert _same_bits(a.bits(), b.bits()), t
    st = b.stats()
    assert st[APPLIED] == 5 and st[CLIPPED] == 0 and st[SKIPPED] == 0 and st[CONSEC] == 0
    assert st[LARGEST] >= st[LAST] > 0


def test_clipped_step_matches_fp64_formula(built_lib):
    """test_adam_matches_tf_formula (tests/test_gpu_golden.py) with the gradient rescaled to the clip norm first: same
    tolerance"""
    from psvo_amd.optim import FlatParams, TFAdam
    torch.manual_seed(0)
    lin = torch.nn.Linear(7, 5).cuda()
    flat = FlatParams(lin)
    CLIP = 0.5
    opt = TFAdam(flat, clip_norm=CLIP)
    assert opt.guarded
    p = flat.flat.double().cpu().clone()
    m = torch.zeros_like(p); v = torch.zeros_like(p)
    clipped = 0
    for t in range(1, 7):
        g = torch.randn(flat.numel) * (1e-3 if t == 4 else 1.0)    # (step 4: far below the clip norm, applied as it is)
        flat.grad.copy_(g.cuda())
        opt.step(3e-3, world_size=2)
        ge = -g.double() / 2                       # maximise, summed over 2 ranks
        norm = ge.norm().item()
        if norm > CLIP:
            ge = ge * (CLIP / norm)
            clipped += 1
        m = 0.9 * m + 0.1 * ge; v = 0.999 * v + 0.001 * ge * ge
        lr_t = 3e-3 * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        p = p - lr_t * m / (v.sqrt() + 1e-8)
        assert torch.allclose(flat.flat.double().cpu(), p, atol=1e-6)
        assert abs(opt.guard_stats()["last_norm"] - norm) <= 1e-6 * norm
    st = opt.guard_stats()
    assert clipped == 5 and st["clipped"] == 5 and st["applied"] == 6 and st["skipped"] == 0
    assert lin.weight.data_ptr() == flat.flat.data_ptr()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_nonfinite_step_is_skipped(built_lib, where, bad):
    _, lib = _lib()
    n = 22426
    G = lib.psvo_grad_norm_blocks(n)
    S = _slice(n, G)
    assert G == 6 and (G - 1) * S < n
    at = {"first": 5, "middle": (G // 2) * S + 17, "last": n - 1}[where]
    assert at // S == {"first": 0, "middle": G // 2, "last": G - 1}[where]
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=gen).cuda()
    good = [torch.randn(n, generator=gen).cuda() for _ in range(3)]
    poisoned = good[1].clone()
    poisoned[at] = bad
    a, ref, off = _Adam(p0), _Adam(p0), _Adam(p0)
    a.guarded(good[0], 1, 0.0, 1)
    ref.plain(good[0], 1)
    before = a.bits()
    assert _same_bits(before, ref.bits())
    for k in (1, 2):                                               # two poisoned steps in a row
        a.guarded(poisoned, 1 + k, 0.0, 1)
        assert _same_bits(a.bits(), before)
        st = a.stats()
        assert st[APPLIED] == 1 and st[SKIPPED] == k and st[CONSEC] == k
        assert not math.isfinite(st[LAST]) and math.isfinite(st[LARGEST]) and st[LARGEST] > 0
    a.guarded(good[2], 4, 0.0, 1)                                  # (a skipped step still advances `step`)
    ref.plain(good[2], 4)
    after = a.bits()
    assert not _same_bits(after, before) and _same_bits(after, ref.bits())
    st = a.stats()
    assert st[APPLIED] == 2 and st[SKIPPED] == 2 and st[CONSEC] == 0 and math.isfinite(st[LAST])
    # a clip norm does not change the decision: still skipped
    a.guarded(poisoned, 5, 10.0, 1)
    assert _same_bits(a.bits(), after) and a.stats()[SKIPPED] == 3 and a.stats()[CLIPPED] == 0
    # guard off: the poisoned gradient goes through exactly as psvo_adam_step puts it through
    off.guarded(poisoned, 1, 0.0, 0)
    ref2 = _Adam(p0)
    ref2.plain(poisoned, 1)
    assert _same_bits(off.bits(), ref2.bits())
    assert off.stats()[APPLIED] == 1 and off.stats()[SKIPPED] == 0
    assert not bool(torch.isfinite(off.p[at]))


def test_optimizer_with_both_flags_off_is_the_plain_step(built_lib):
    from psvo_amd.optim import FlatParams, TFAdam
    torch.manual_seed(0)
    la, lb = torch.nn.Linear(7, 5).cuda(), torch.nn.Linear(7, 5).cuda()
    lb.load_state_dict(la.state_dict())
    fa, fb = FlatParams(la), FlatParams(lb)
    oa, ob = TFAdam(fa), TFAdam(fb, skip_nonfinite=True)
    assert not oa.guarded and oa.guard_stats() is None and not hasattr(oa, "state") and ob.guarded
    for t in range(3):
        g = torch.randn(fa.numel).cuda()
        if t == 1:
            g[3] = float("inf")
        fa.grad.copy_(g); fb.grad.copy_(g)
        oa.step(3e-3); ob.step(3e-3)
    assert not bool(torch.isfinite(fa.flat).all())                 # unguarded: the parameters are gone
    assert bool(torch.isfinite(fb.flat).all())
    assert ob.guard_stats() == dict(ob.guard_stats(), applied=2, skipped=1, clipped=0, consecutive_skipped=0)


def test_two_runs_are_bit_identical(built_lib):
    n = 1000003
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=gen).cuda()
    gs = [torch.randn(n, generator=gen).cuda() for _ in range(3)]
    runs = []
    for _ in range(2):
        a = _Adam(p0)
        parts = []
        for t, g in enumerate(gs, 1):
            a.guarded(g, t, 10.0, 1)
            parts.append(a.partial.view(torch.int64).cpu().clone())
        runs.append((a.bits(), parts, a.stats()))
    assert _same_bits(runs[0][0], runs[1][0])
    assert all(torch.equal(x, y) for x, y in zip(runs[0][1], runs[1][1]))
    assert runs[0][2] == runs[1][2] and runs[0][2][CLIPPED] == 3


# ------------------------------------------------------------------------------------------------------------------
def test_illconditioned_state_one_clipped_step(built_lib):
    """tests/golden/fhn_illconditioned_state.npz, recipe of test_illconditioned_state_is_fp32s_own_error: the oracle's forward
    pass for the teacher indices, then the HIP gradient -- fp32 rounding error of norm ~1.9e5 around a true gradient of norm
    3.6e2.  One step from zero moments with clip_norm = 10 leaves ||m|| <= (1 - beta1) 10 and max v <= (1 - beta2) 100; the
    unguarded step puts ||m|| > 100 into the moments."""
    from oracle import psvo_oracle as O
    from psvo_amd.model import SSM
    from psvo_amd.optim import FlatParams, TFAdam
    from psvo_amd.SMC.PSVO import PSVO
    from tests import notebook_curve as NC
    st = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fhn_illconditioned_state.npz"))
    FLAGS = NC.notebook_flags(seed=3, epochs=1)
    torch.manual_seed(3)
    model = SSM(FLAGS).cuda()
    fp = FlatParams(model)
    assert fp.numel == st["flat"].size
    fp.flat.copy_(torch.tensor(st["flat"]).cuda())
    obs = torch.tensor(st["obs"][None]).double()
    fl = Hh.oracle_flags(FLAGS, "PSVO")
    noise = O.make_noise(fl, 1, 200, seed=int(st["noise_seed"]))
    _, ref0 = Hh.run_oracle(model, FLAGS, "PSVO", obs, noise)
    nz = Hh.noise_to_hip({**noise, "idx_f": ref0["idx_f"], "idx_b": ref0["idx_b"]}, "cuda")
    for key in ("u_f", "u_b"):
        nz.pop(key, None)
    fp.zero_grad()
    z, _ = PSVO(model, FLAGS).get_log_ZSMC(obs.float().cuda(), None, noise=nz)
    z.backward()
    torch.cuda.synchronize()
    norm = fp.grad.double().norm().item()
    print("HIP gradient norm on the ill-conditioned state: %.4g" % norm)
    assert norm >= 1e3
    flat0 = fp.flat.clone()
    CLIP = 10.0
    opt = TFAdam(fp, clip_norm=CLIP)
    opt.step(FLAGS.lr)
    s = opt.guard_stats()
    m_norm, v_max = opt.m.double().norm().item(), opt.v.double().max().item()
    print("guarded: ||m|| %.6g  max v %.6g  stats %s" % (m_norm, v_max, s))
    assert m_norm <= (1 - opt.beta1) * CLIP * (1 + 1e-5)
    assert v_max <= (1 - opt.beta2) * CLIP ** 2 * (1 + 1e-5)
    assert s["clipped"] == 1 and s["applied"] == 1 and s["skipped"] == 0
    assert abs(s["last_norm"] - norm) <= 1e-6 * norm
    assert bool(torch.isfinite(fp.flat).all())
    fp.flat.copy_(flat0)
    plain = TFAdam(fp)
    plain.step(FLAGS.lr)
    m_plain = plain.m.double().norm().item()
    print("unguarded: ||m|| %.6g" % m_plain)
    assert m_plain > 100.0


# ------------------------------------------------------------------------------------------------------------------
def _train_small(tmp_path, **flags):
    from oracle import psvo_oracle as O
    from psvo_amd.model import SSM
    from psvo_amd.SMC.PSVO import PSVO
    from psvo_amd.trainer import trainer
    hid, obs = O.fhn_synthetic(12, 30, seed=0)
    FLAGS = Hh.make_flags("PSVO", n_particles=16, n_particles_for_BSim_proposal=4, batch_size=4, time=30, epoch=4,
                          lr=1e-2, MSE_steps=5, saving_num=4, rslt_dir_name="t", **flags)
    torch.manual_seed(0); np.random.seed(0)
    model = SSM(FLAGS).cuda()
    smc = PSVO(model, FLAGS)
    smc.generator = torch.Generator(device="cuda").manual_seed(1)
    tr = trainer(model, smc, FLAGS)
    rlt = str(tmp_path) + "/rslts/t/run/"
    os.makedirs(rlt)
    tr.init_data_saving(rlt)
    hist, _ = tr.train(obs[:8].numpy(), obs[8:].numpy(), hid[:8].numpy(), hid[8:].numpy(), print_freq=1)
    metrics = {}
    for path in glob.glob(tr.epoch_data_DIR + "metric_*.p"):
        with open(path, "rb") as f:
            metrics[int(path.rsplit("_", 1)[1][:-2])] = pickle.load(f)
    return tr, hist, metrics


@pytest.mark.parametrize("hipgraph", ["1", "0"])
def test_trainer_with_clip_norm(built_lib, tmp_path, monkeypatch, capsys, hipgraph):
    """the configuration of test_trainer_improves_elbo with --clip_norm and --skip_nonfinite_steps, the local step replayed from
    a hipGraph and issued eagerly: the ELBO improves, metric_<iter>.p carries the guard's counts and they add up to the steps"""
    monkeypatch.setenv("PSVO_HIPGRAPH", hipgraph)
    monkeypatch.chdir(tmp_path)
    tr, hist, metrics = _train_small(tmp_path, clip_norm=10.0, skip_nonfinite_steps=True)
    steps = 4 * 2                                                    # 4 epochs of 8 sequences in batches of 4
    assert len(hist["log_ZSMC_trains"]) == 5
    print("train ELBO", hist["log_ZSMC_trains"], "guard", tr.guard_intervals)
    assert hist["log_ZSMC_trains"][-1] > hist["log_ZSMC_trains"][0]
    assert sorted(metrics) == [1, 2, 3, 4]
    for m in metrics.values():
        assert {"log_ZSMC_train", "log_ZSMC_test", "R_square_train", "R_square_test"} <= set(m)
        assert {"guard_last_norm", "guard_max_norm", "guard_applied", "guard_clipped", "guard_skipped"} <= set(m)
        assert m["guard_applied"] + m["guard_skipped"] == 2 and 0 <= m["guard_clipped"] <= m["guard_applied"]
    assert sum(m["guard_applied"] + m["guard_skipped"] for m in metrics.values()) == steps
    total = tr.optimizer.guard_stats()
    assert total["applied"] + total["skipped"] == steps == tr.optimizer.t
    assert total["clipped"] == sum(m["guard_clipped"] for m in metrics.values())
    assert len(tr.guard_intervals) == 5 and tr.guard_intervals[0]["guard_applied"] == 0      # (the evaluation before training)
    assert capsys.readouterr().out.count("gradient guard:") == 5
    graphs = tr.__dict__.get("_graphs", {})
    assert (len(graphs) == 1 and all(g is not False for g in graphs.values())) if hipgraph == "1" else not graphs


def test_trainer_with_the_flags_off_adds_no_key(built_lib, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    tr, hist, metrics = _train_small(tmp_path)
    assert not tr.optimizer.guarded and tr.guard_intervals == []
    for m in metrics.values():
        assert set(m) == {"log_ZSMC_train", "log_ZSMC_test", "R_square_train", "R_square_test"}
    assert "gradient guard" not in capsys.readouterr().out


def test_trainer_stops_when_every_step_of_an_interval_is_skipped(built_lib, tmp_path, monkeypatch, capsys):
    """every gradient of the run is given a NaN entry (behind the all-reduce, where the optimizer takes it): every step is
    skipped, the parameters stay bit for bit what they were, and the first evaluation after an interval without one applied
    step ends the training with a message"""
    from psvo_amd import dp
    monkeypatch.chdir(tmp_path)
    real = dp.all_reduce_sum_

    def poisoned(grad):
        real(grad)
        grad[grad.numel() // 2] = float("nan")
    monkeypatch.setattr(dp, "all_reduce_sum_", poisoned)
    tr, hist, metrics = _train_small(tmp_path, skip_nonfinite_steps=True)
    out = capsys.readouterr().out
    assert "was skipped" in out and "stop training" in out
    assert len(hist["log_ZSMC_trains"]) == 2                         # before training, after epoch 1 -- and no further
    assert tr.optimizer.t == 2
    s = tr.optimizer.guard_stats()
    assert s["skipped"] == 2 and s["applied"] == 0 and s["consecutive_skipped"] == 2 and not math.isfinite(s["last_norm"])
    assert metrics[1]["guard_skipped"] == 2 and metrics[1]["guard_applied"] == 0
    assert float(tr.optimizer.m.abs().max()) == 0.0 and float(tr.optimizer.v.abs().max()) == 0.0
    assert bool(torch.isfinite(tr.flat.flat).all())
