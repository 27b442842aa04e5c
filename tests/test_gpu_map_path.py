"""The MAP trajectory (psvo_map_path, --MAP_path) on the GPU: the kernels directly on synthetic particle systems, through the
filter objectives, beside training, and through runner.main.

What is asserted, per launch (check_outputs):
  * the kernel's outputs are consistent with each other EXACTLY: path[T-1] is the lowest argmax of delta[T-1], path[t-1] =
    bp[t][path[t]], Xmap is the gather bit for bit, max_j delta[t] = 0, bp[0] = arange, every index in [0, N);
  * one step in fp64 GIVEN the kernel's own delta[t-1] (tests/map_reference.one_step): with s[j,k] = delta[t-1][k] + l64[j,k] a
    backpointer is off where it differs from the lowest fp64 argmax; its distance max_k s - s[j,bp] is at most
    32 2^-24 (1 + |s[j,bp]|) -- (Dx + 3) roundings of magnitude |s| for each of two candidates, times 2 -- and at most
    max(3, 2 %) of the entries are off; delta[t][j] + lmax[t] equals G64[j] + s[j,bp] to the same bound plus 8 2^-24 |G64[j]|;
  * against the fp64 reference by the smoother's rule, err_hip <= 8 err_32 + 8 2^-24 max|ref| with err_32 the fp32 CPU
    restatement against fp64 (K = 8: profiles/ffbs_smoother.md, the same pair arithmetic): delta over the finite entries, and
    the running sums of lmax with the floor 8 2^-24 sum_t |lmax64|;
  * optimality: 0 <= opt64 - J64(path_hip) <= 2 (the bound on delta above).
Every figure is printed before it is asserted (pytest -s shows them).
"""
import glob
import pickle

import pytest
import torch

from tests import helpers as Hh
from tests import map_reference as R

pytestmark = pytest.mark.gpu

ULP = R.ULP
K = 8
_ids = [R.case_id(c) for c in R.DIRECT]


def _launch(k, obs=None):
    from psvo_amd import ops
    T, B, Dx, N, _ = k["shape"]
    desc = ops.make_desc(B, T, N, 1, Dx, k["Dy"], k["H"], emission=k["emission"])
    cu = lambda v: None if v is None else v.cuda()
    filt = {"X": cu(k["X"]), "Fm": cu(k["Fm"])}
    out = ops.map_path(desc, filt, [w.cuda() for w in k["g"]], cu(k["sig_f"]), cu(k["sig_g"]), cu(k["fm0"]), cu(k["fsig0"]),
                       cu(k["obs"] if obs is None else obs))
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in out.items()}


def check_outputs(tag, inp, out, r64, r32):
    """the rules of the module docstring; inp: X, Fm, sig_f, fm0, fsig0 (fp32, CPU); out: the kernel's dict on the CPU"""
    X, Fm, sig_f = inp["X"], inp["Fm"], inp["sig_f"]
    T, B, Dx, N = X.shape
    delta, lmax, bp, path, Xmap = (out[n] for n in ("delta", "lmax", "bp", "path", "Xmap"))
    # ---- exact consistency ----
    assert bp.dtype == torch.int32 and path.dtype == torch.int32
    assert int(bp.min()) >= 0 and int(bp.max()) < N and int(path.min()) >= 0 and int(path.max()) < N
    assert torch.isfinite(delta).all() and torch.isfinite(lmax).all()
    assert torch.equal(bp[0].long(), torch.arange(N).expand(B, N))
    assert float(delta.max(-1).values.abs().max()) == 0.0
    assert torch.equal(path.long(), R.backtrack(delta, bp))
    assert torch.equal(Xmap, R.gather(X, path))
    # ---- one step in fp64 on the kernel's own delta[t-1] ----
    step = R.one_step(delta, bp, X, Fm, sig_f)
    bound = 32 * ULP * (1 + step["s_bp"].abs())
    n_off, worst = int(step["off"].sum()), float((step["dist"] / bound).max()) if T > 1 else 0.0
    d_hip = delta.double() + lmax.double().unsqueeze(-1)
    G64 = r64["G"]
    s0 = R.log_prior(X[0].double(), inp["fm0"].double(), inp["fsig0"].double()).unsqueeze(0)
    s_all = torch.cat([s0, step["s_bp"]])                                                 # (T, B, N): what G is added to
    d_err = (d_hip - (G64 + s_all)).abs()
    d_bound = 32 * ULP * (1 + s_all.abs()) + 8 * ULP * G64.abs()
    print("map-step %s off %d of %d (allowed %d) worst distance / bound %.3f  worst |d - d64| / bound %.3f"
          % (tag, n_off, step["off"].numel(), max(3, int(0.02 * step["off"].numel())), worst, float((d_err / d_bound).max())))
    # ---- the smoother's rule against the fp64 reference ----
    fin = torch.isfinite(r64["delta"])
    e_hip = float((delta.double() - r64["delta"])[fin].abs().max())
    e_32 = float((r32["delta"].double() - r64["delta"])[fin].abs().max())
    floor = 8 * ULP * float(r64["delta"][fin].abs().max())
    run = lambda v: torch.cumsum(v.double(), 0)
    c_hip = float((run(lmax) - run(r64["lmax"])).abs().max())
    c_32 = float((run(r32["lmax"]) - run(r64["lmax"])).abs().max())
    c_floor = 8 * ULP * float(r64["lmax"].abs().sum(0).max())
    print("map-yardstick %s delta err_hip %.3e err_32 %.3e floor %.3e | sum lmax err_hip %.3e err_32 %.3e floor %.3e"
          % (tag, e_hip, e_32, floor, c_hip, c_32, c_floor))
    # ---- optimality ----
    opt = r64["lmax"].sum(0)
    gap = opt - R.joint64(path, X, Fm, sig_f, inp["fm0"], inp["fsig0"], G64)
    same = bool(torch.equal(path.long(), r64["path"]))
    print("map-optimality %s gap max %.3e min %.3e allowed %.3e path == fp64 path: %s"
          % (tag, float(gap.max()), float(gap.min()), 2 * (K * e_32 + floor), same))
    assert bool((step["dist"] <= bound).all())
    assert n_off <= max(3, int(0.02 * step["off"].numel()))
    assert bool((d_err <= d_bound).all())
    assert e_hip <= K * e_32 + floor
    assert c_hip <= K * c_32 + c_floor
    assert float(gap.min()) >= -1e-9 * (1 + float(opt.abs().max()))
    assert float(gap.max()) <= 2 * (K * e_32 + floor)


@pytest.mark.parametrize("c", R.DIRECT, ids=_ids)
def test_kernel_against_fp64(built_lib, c):
    k = R.case(c)
    out = _launch(k)
    check_outputs(R.case_id(c), k, out, k["ref64"], k["ref32"])
    if k["kind"] == "tie":
        assert torch.equal(out["bp"].long(), k["ref64"]["bp"]) and torch.equal(out["path"].long(), k["ref64"]["path"])
        assert int(out["bp"][1:].max()) < k["shape"][3] // 2 and int(out["path"].max()) < k["shape"][3] // 2


@pytest.mark.parametrize("c", R.INSTANCES, ids=[R.case_id(c) for c in R.INSTANCES])
def test_every_instantiation(built_lib, c):
    k = R.case(c)
    check_outputs(R.case_id(c), k, _launch(k), k["ref64"], k["ref32"])


def test_a_row_with_nothing_observed_acts_through_G_alone(built_lib):
    """one whole observation row set to NaN: the other sequence and the earlier steps are bit-identical, the step's backpointers
    too (they do not read G), and the step's d is the pair maximum alone -- lmax by the one-step bound with G = 0"""
    k = R.case(R.DIRECT[2])
    t0, b0 = 3, 0
    obs = k["obs"].clone()
    obs[t0, b0] = float("nan")
    base, out = _launch(k), _launch(k, obs=obs)
    for n in ("delta", "lmax", "bp"):
        assert torch.equal(out[n][:, 1 - b0], base[n][:, 1 - b0]), n
        assert torch.equal(out[n][:t0, b0], base[n][:t0, b0]), n
    assert torch.equal(out["bp"][t0], base["bp"][t0])
    assert not torch.equal(out["lmax"][t0, b0], base["lmax"][t0, b0])
    step = R.one_step(out["delta"], out["bp"], k["X"], k["Fm"], k["sig_f"])
    s = step["s_bp"][t0 - 1, b0]                                                          # (N,)
    d = out["delta"][t0, b0].double() + out["lmax"][t0, b0].double()
    err = (d - s).abs() / (32 * ULP * (1 + s.abs()))
    lerr = abs(float(out["lmax"][t0, b0]) - float(s.max())) / (32 * ULP * (1 + abs(float(s.max()))))
    print("map-nan-row d against the pair maximum alone, worst / bound %.3f; lmax %.3f" % (float(err.max()), lerr))
    assert float(err.max()) <= 1.0 and lerr <= 1.0
    r64 = R.map_path(**{**{n: k[n] for n in ("X", "Fm", "sig_f", "fm0", "fsig0", "g", "sig_g", "emission")}, "obs": obs})
    assert float(r64["G"][t0, b0].abs().max()) == 0.0


@pytest.mark.parametrize("c", R.DIRECT, ids=_ids)
def test_two_launches_are_bit_identical(built_lib, c):
    from psvo_amd import _lib
    k = R.case(c)
    a, b = _launch(k), _launch(k)
    with Hh.tuning(_lib.PSVO_TUNE_DETERMINISTIC, 1):
        d1, d2 = _launch(k), _launch(k)
    for n in a:
        assert torch.equal(a[n], b[n]) and torch.equal(d1[n], d2[n]) and torch.equal(a[n], d1[n]), n


def test_ops_map_path_refuses_bad_arguments(built_lib):
    from psvo_amd import ops
    k = R.case(R.DIRECT[1])
    T, B, Dx, N, _ = k["shape"]
    cu = lambda v: v.cuda()
    good = dict(filt={"X": cu(k["X"]), "Fm": cu(k["Fm"])}, g=[cu(w) for w in k["g"]], sig_f=cu(k["sig_f"]), sig_g=cu(k["sig_g"]),
                fm0=cu(k["fm0"]), fsig0=cu(k["fsig0"]), obs=cu(k["obs"]))
    desc = ops.make_desc(B, T, N, 1, Dx, k["Dy"], k["H"], emission=k["emission"])
    ops.map_path(desc, **good)
    bad = [("obs", good["obs"][:, :, :1].contiguous(), "shape"), ("obs", good["obs"].double(), "float32"),
           ("sig_f", good["sig_f"][:1].contiguous(), "shape"), ("fm0", good["fm0"][:1].contiguous(), "shape"),
           ("fsig0", good["fsig0"].cpu(), "HBM"), ("sig_g", None, "count emission only"), ("obs", None, "needs")]
    for name, val, word in bad:
        with pytest.raises(ValueError, match=word):
            ops.map_path(desc, **dict(good, **{name: val}))
    with pytest.raises(ValueError, match="shape"):
        ops.map_path(desc, **dict(good, filt={"X": good["filt"]["X"], "Fm": good["filt"]["Fm"][:, :, :, :N - 1].contiguous()}))
    with pytest.raises(ValueError, match="shape"):
        ops.map_path(desc, **dict(good, g=[good["g"][0], good["g"][1], good["g"][2][:, :1].contiguous(), good["g"][3]]))
    x600 = torch.zeros(T, B, Dx, 600, device="cuda")
    with pytest.raises(ValueError, match="N = 600.*N <= 512"):
        ops.map_path(ops.make_desc(B, T, 600, 1, Dx, k["Dy"], k["H"], emission=k["emission"]), **dict(good, filt={"X": x600, "Fm": x600}))
    torch.cuda.synchronize()


# ---- through the model ---------------------------------------------------------------------------------------------------
MODEL_CASES = [
    # (objective, B, T, N, M, Dx, Dy, H, bootstrap, two_q), extra flags
    (("AESMC", 2, 6, 16, 1, 2, 1, 32, True, True), {}),
    (("IWAE", 2, 8, 96, 1, 3, 1, 16, False, True), {}),                 # weights carried, never resampled
    (("SVO", 2, 6, 24, 1, 2, 2, 32, False, False), {}),
    (("AESMC", 2, 6, 40, 1, 3, 10, 32, True, True), {}),                # the wide-observation filter
    (("AESMC", 2, 6, 16, 1, 2, 2, 32, True, True), dict(missing_obs=True)),
    (("AESMC", 2, 6, 32, 1, 2, 1, 32, True, True), dict(resample_ess=0.5)),
]
_mid = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else ",".join(sorted(v)) or "plain"


def _setup(case, extra, **more):
    from tests.test_gpu_ffbs import _setup as setup
    FLAGS, model, cls, obs, noise = setup(*case, **extra, **more)
    if extra.get("missing_obs"):
        gen = torch.Generator().manual_seed(8)
        gaps = (torch.rand(obs.shape, generator=gen) < 0.3)
        gaps[0, 2] = True                                               # one whole row
        obs = obs.masked_fill(gaps.cuda(), float("nan"))
    return FLAGS, model, cls, obs, noise


def _with(cls, model, FLAGS, obj, **kw):
    return cls(model, Hh.make_flags(obj, **{**FLAGS.as_dict(), **kw}))


@pytest.mark.parametrize("case,extra", MODEL_CASES, ids=_mid)
def test_map_path_behind_the_filter_objectives(built_lib, case, extra):
    obj, B, T, N, M, Dx, Dy = case[:7]
    FLAGS, model, cls, obs, noise = _setup(case, extra, MAP_path=True)
    smc = cls(model, FLAGS)
    assert smc.MAP_path is True
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs, None, noise=noise)
        z0, log0 = _with(cls, model, FLAGS, obj, MAP_path=False).get_log_ZSMC(obs, None, noise=noise)
    torch.cuda.synchronize()
    # everything else is untouched
    assert torch.equal(z, z0) and torch.equal(log["Xs"], log0["Xs"])
    assert set(log) - set(log0) == {"X_map", "map_index", "map_score", "map"} and set(log0) <= set(log)
    for n in ("X", "Fm", "logW", "Xanc"):
        assert torch.equal(log["filter"][n], log0["filter"][n]), n
    mp = log["map"]
    assert log["X_map"].shape == (B, T, Dx) and log["X_map"].dtype == torch.float32
    assert log["map_index"].shape == (B, T) and log["map_index"].dtype == torch.int32
    assert log["map_score"].shape == (B,) and log["map_score"].dtype == torch.float64
    assert mp["delta"].shape == (T, B, N) and mp["lmax"].shape == (T, B) and mp["bp"].shape == (T, B, N)
    assert torch.equal(log["X_map"], mp["Xmap"].transpose(0, 1)) and torch.equal(log["map_index"], mp["path"].transpose(0, 1))
    assert torch.equal(log["map_score"], mp["lmax"].double().sum(0))
    # what the kernel was given: the filter's own particles and t = 0 term, the observations as the filter saw them
    assert torch.equal(mp["obs"].isnan(), obs.transpose(0, 1).isnan())
    assert torch.equal(mp["obs"][~mp["obs"].isnan()], obs.transpose(0, 1)[~obs.transpose(0, 1).isnan()])
    if extra.get("missing_obs"):
        assert mp["obs"].isnan().any() and torch.equal(log["missing"], obs.isnan())
    dist = model.q1_dist if FLAGS.use_bootstrap else model.f_dist
    assert torch.allclose(mp["sig_f"], dist.get_sigma().detach().float(), rtol=1e-6, atol=0)
    # the reference on the filter's outputs
    cpu = lambda v: None if v is None else v.detach().cpu()
    inp = dict(X=cpu(log["filter"]["X"]), Fm=cpu(log["filter"]["Fm"]), sig_f=cpu(mp["sig_f"]), fm0=cpu(mp["fm0"]),
               fsig0=cpu(mp["fsig0"]), obs=cpu(mp["obs"]), g=[cpu(w) for w in mp["g"]], sig_g=cpu(mp["sig_g"]),
               emission=smc._emission_code())
    r64, r32 = R.map_path(dtype=torch.float64, **inp), R.map_path(dtype=torch.float32, **inp)
    out = {n: cpu(mp[n]) for n in ("delta", "lmax", "bp", "path", "Xmap")}
    check_outputs(_mid(case) + ("+" + _mid(extra) if extra else ""), inp, out, r64, r32)
    assert torch.equal(cpu(log["X_map"]), R.gather(inp["X"], out["path"]).transpose(0, 1))

    # no random number is drawn: the objective's generator ends where it ends without the flag
    states = []
    for on in (True, False):
        s = _with(cls, model, FLAGS, obj, MAP_path=on)
        s.generator = torch.Generator(device="cuda").manual_seed(5)
        with torch.no_grad():
            _, lg = s.get_log_ZSMC(obs, None)
        states.append((s.generator.get_state().clone(), lg["Xs"].clone()))
    assert torch.equal(states[0][0], states[1][0]) and torch.equal(states[0][1], states[1][1])


def test_beside_both_smoothers(built_lib):
    """--FFBS --FFBSi --MAP_path: all three run, and log["Xs"] is bit-identical to the run without --MAP_path under the same seed"""
    case, extra = MODEL_CASES[0]
    obj, B, T, N, M, Dx = case[:6]
    FLAGS, model, cls, obs, _ = _setup(case, extra, FFBS=True, FFBSi=True, MAP_path=True)
    logs = []
    for on in (True, False):
        smc = _with(cls, model, FLAGS, obj, MAP_path=on)
        smc.generator = torch.Generator(device="cuda").manual_seed(11)
        with torch.no_grad():
            logs.append(smc.get_log_ZSMC(obs, None)[1])
    torch.cuda.synchronize()
    a, b = logs
    for n in ("Xs", "Xs_filter", "Xs_marginal", "X_smooth_mean", "path_logq", "path_distinct"):
        assert torch.equal(a[n], b[n]), n
    assert "X_map" in a and "smoother" in a and "paths" in a and "X_map" not in b
    assert a["X_map"].shape == (B, T, Dx)
    X = a["filter"]["X"]
    assert torch.equal(a["X_map"], R.gather(X.cpu(), a["map"]["path"].cpu()).transpose(0, 1).cuda())


@pytest.mark.parametrize("case,extra", [MODEL_CASES[0], MODEL_CASES[2]], ids=["AESMC", "SVO"])
def test_training_is_unaffected(built_lib, monkeypatch, case, extra):
    """under autograd the kernel is not launched; ELBO and every parameter gradient are bit-identical with and without --MAP_path"""
    from psvo_amd import ops
    obj = case[0]
    FLAGS, model, cls, obs, noise = _setup(case, extra, MAP_path=True)

    def refuse(*a, **k):
        raise AssertionError("ops.map_path was called under autograd")
    monkeypatch.setattr(ops, "map_path", refuse)
    res = []
    for on in (True, False):
        smc = _with(cls, model, FLAGS, obj, MAP_path=on)
        assert smc.MAP_path is on
        model.zero_grad(set_to_none=True)
        z, log = smc.get_log_ZSMC(obs, None, noise=noise)
        z.backward()
        torch.cuda.synchronize()
        assert "X_map" not in log and "map" not in log
        res.append((z.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 4
    for n, g in res[0][1].items():
        assert torch.equal(g, res[1][1][n]), n


@pytest.mark.parametrize("obj,kw,word", [
    ("PSVO", {}, r"--MAP_path with --PSVO / --PSVOwR"),
    ("PSVOwR", {}, r"--MAP_path with --PSVO / --PSVOwR"),
    ("AESMC", dict(output_cov=True, diag_cov=True), r"--MAP_path with output_cov"),
    ("SVO", dict(q1_layers="32,32", g_layers="32,32"), r"--MAP_path with per-particle MLP layers.*one hidden layer"),
    ("IWAE", dict(Dx=3, Dy=33), r"Dy = 33.*Dy <= 32"),
], ids=["PSVO", "PSVOwR", "output_cov", "two-layers", "Dy33"])
def test_refusals_on_the_device(built_lib, obj, kw, word):
    from psvo_amd.model import SSM
    from psvo_amd.SMC.AESMC import AESMC
    from psvo_amd.SMC.IWAE import IWAE
    from psvo_amd.SMC.PSVO import PSVO
    from psvo_amd.SMC.PSVOwR import PSVOwR
    from psvo_amd.SMC.SVO import SVO
    FLAGS = Hh.make_flags(obj, MAP_path=True, **kw)
    model = SSM(FLAGS).cuda()
    with pytest.raises(ValueError, match=word):
        {"AESMC": AESMC, "IWAE": IWAE, "PSVO": PSVO, "PSVOwR": PSVOwR, "SVO": SVO}[obj](model, FLAGS)


def test_runner_end_to_end(built_lib, tmp_path, monkeypatch):
    """runner.main --noPSVO --AESMC --MAP_path for two tiny epochs: both metric keys are in metric_<iter>.p, X_map and map_index
    in trajectory_<epoch>.p"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    monkeypatch.chdir(tmp_path)
    runner.main(parse_flags(["--noPSVO", "--AESMC", "--MAP_path", "--generateTrainingData", "--time=20", "--n_train=4",
                             "--n_test=4", "--batch_size=2", "--n_particles=16", "--epoch=2"]))
    torch.cuda.synchronize()
    metrics = glob.glob(str(tmp_path / "rslts" / "epoch_data" / "**" / "metric_*.p"), recursive=True)
    assert metrics
    for path in metrics:
        with open(path, "rb") as fh:
            m = pickle.load(fh)
        for split in ("train", "test"):
            assert isinstance(m["map_score_" + split], float) and m["map_score_" + split] == m["map_score_" + split]
    traj = glob.glob(str(tmp_path / "rslts" / "epoch_data" / "**" / "trajectory_*.p"), recursive=True)
    assert traj
    for path in traj:
        with open(path, "rb") as fh:
            t = pickle.load(fh)
        assert t["Xs"].shape == (4, 20, 16, 2) and t["X_map"].shape == (4, 20, 2) and t["map_index"].shape == (4, 20)
        assert 0 <= t["map_index"].min() and t["map_index"].max() < 16
