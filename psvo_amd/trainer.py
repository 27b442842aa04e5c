"""trainer -- the reference's training driver (src/trainer.py:21-395) for the MI355X path: same public surface
(constructor, init_data_saving, train, evaluate, evaluate_R_square, adjust_lr, saving_feed_dict, the metric /
trajectory pickles and their keys) and the same schedule semantics, written for this stack.

TensorFlow graph/session plumbing has no equivalent: `fetches` are names ("log_ZSMC", "Xs", "y_hat", "y") instead of
graph tensors and feed dicts are keyed by model.obs / model.hidden ("obs" / "hidden").  Matplotlib output (quiver,
R-square plots) is presentation only and not built.

Data parallelism (new relative to the reference): with W ranks every mini-batch of
FLAGS.batch_size sequences is sharded FLAGS.batch_size / W per rank; one flat all-reduce of the gradient per step,
identical Adam update on every rank (checked bit for bit every print_freq epochs); evaluation batches are dealt
round-robin over the ranks and gathered.

Gradient guard (new relative to the reference's trainer; FLAGS.clip_norm, FLAGS.skip_nonfinite_steps, both off by default): the
optimizer clips by the global norm and leaves non-finite steps out on the device (psvo_amd.optim.TFAdam).  The norm is taken
after the all-reduce, so every rank decides alike.  At every evaluation the counts since the previous one are printed, go into
metric_<iter>.p under the guard_* keys, and an interval in which every step was skipped stops the training.

Marginal smoother (FLAGS.FFBS, off by default; SVO / AESMC / IWAE): every evaluation then runs psvo_ffbs_smooth behind the filter
(psvo_amd.SMC.SVO), so "Xs", the k-step predictions and the saved trajectories come from the smoothed particles; the mean and the
minimum of the smoothed weights' effective sample size over each split are printed and go into metric_<iter>.p as
ffbs_ess_mean_<split> / ffbs_ess_min_<split>.  Training steps are untouched.

Backward-sampled trajectories (FLAGS.FFBSi, off by default; SVO / AESMC / IWAE): every evaluation then runs psvo_ffbs_sample
behind the filter, so "Xs", the k-step predictions and the saved trajectories are whole paths, as under PSVO; the mean and the
minimum over each split of the number of distinct particles the N paths pass through are printed and go into metric_<iter>.p
as ffbsi_distinct_mean_<split> / ffbsi_distinct_min_<split>.  Training steps are untouched.

MAP trajectory (FLAGS.MAP_path, off by default; SVO / AESMC / IWAE): every evaluation then also runs psvo_map_path behind the
filter; the mean over each split of the path's joint log-density per time step, map_score / T, is printed and goes into
metric_<iter>.p as map_score_<split>; trajectory_<epoch>.p gains X_map (saving_num, T, Dx) and map_index (saving_num, T) of the saved
sequences.  "Xs" and everything derived from it are unchanged.  Training steps are untouched.

Adaptive resampling (FLAGS.resample_ess, off by default; SVO / AESMC): training and evaluation run the adaptive filter kernels;
at every evaluation the share of (sequence, step) pairs that resampled and the mean / minimum of ESS / N over each split are
printed and go into metric_<iter>.p as adaptive_rate_<split>, adaptive_ess_mean_<split>, adaptive_ess_min_<split>.

Particle forecast (FLAGS.particle_forecast, off by default; every objective): every evaluation then also runs
psvo_particle_forecast on the evaluation's own cloud (SVO.particle_forecast) for k = 0 .. MSE_steps; per horizon the mean predictive
log-density over the (sequence, origin) pairs whose target lies inside the data, the R-square of the predictive mean and the
calibration mean((y - y_mean)^2 / y_var) (about 1 when calibrated) are printed and go into metric_<iter>.p as forecast_lpd_<split>,
forecast_R_square_<split>, forecast_calibration_<split>; y_hat_<epoch>.p gains y_mean and y_var of the saved sequences.
Training steps are untouched.

Missing observations (FLAGS.missing_obs, off by default; SVO / AESMC / IWAE, and PSVO with FLAGS.BSim_missing_obs): a NaN observation
was not made; training and evaluation run the missing-observation filter kernels (PSVO: and the missing-observation backward
simulation behind them), and the ELBO bounds the log-density of the observed entries.  The k-step R-square takes
residuals and the centring mean over observed targets only; at every evaluation the share of missing entries of each split is
printed and goes into metric_<iter>.p as missing_share_<split>.  y_hat at k = 0 is the model's imputation and is saved as before.
With FLAGS.resample_ess_missing_obs the adaptive metrics above are reported beside it; with FLAGS.particle_forecast_missing_obs the
forecast metrics are taken over observed targets (_forecast_metrics) and forecast_lpd_per_entry_<split> is added.
"""
import math
import os
import pickle
import time

import numpy as np
import torch

from . import autograd, dp
from .optim import FlatParams, TFAdam


class StopTraining(Exception):
    pass


def _shuffle(*arrays):
    """sklearn.utils.shuffle(obs, hidden) of the reference (trainer.py:146): one shared permutation
    drawn from numpy's global RNG (seeded by FLAGS.seed, runner.py:42)."""
    perm = np.random.permutation(len(arrays[0]))
    return tuple(a[perm] for a in arrays)


def _r_square(y_hat, y, missing_obs=False):
    """1 - SS_res / SS_tot with the total sum of squares taken around the mean over the evaluation set (axis 0), per
    time step and feature -- the reference's definition (trainer.py:325-329).
    missing_obs (FLAGS.missing_obs): a NaN target was not observed -- residuals and the centring mean are taken over the observed
    targets only (a (time step, feature) that no sequence observed contributes nothing to either sum)."""
    if missing_obs:
        seen = ~np.isnan(y)
        n = seen.sum(axis=0, keepdims=True)
        y0 = np.where(seen, y, 0.0)
        mean = y0.sum(axis=0, keepdims=True) / np.maximum(n, 1)
        resid = np.where(seen, y_hat - y0, 0.0)
        centred = np.where(seen, y0 - mean, 0.0)
        return 1.0 - float(np.square(resid).sum()) / float(np.square(centred).sum())
    resid = y_hat - y
    centred = y - y.mean(axis=0, keepdims=True)
    return 1.0 - float(np.square(resid).sum()) / float(np.square(centred).sum())


def _forecast_metrics(y_mean, y_var, lpd, obs, missing_obs=False):
    """(lpd, R-square, calibration) per horizon k = 0 .. K of a particle forecast over one split: y_mean, y_var (n,T,K+1,Dy),
    lpd (n,T,K+1), obs (n,T,Dy).  Horizon k pairs origin t with obs[:, t + k], t + k < T; a horizon with no such pair (K >= T)
    is NaN.  R-square as _r_square defines it.
    missing_obs (FLAGS.missing_obs with FLAGS.particle_forecast_missing_obs): a NaN in obs was not observed and lpd scores the
    observed entries of its target row.  A pair is valid when its target row has an observed entry: the mean lpd is over the
    valid pairs, R-square is _r_square(.., missing_obs=True), the calibration is over observed entries, a horizon without an
    observed target is NaN, and a fourth array is returned, lpd per entry = sum lpd / sum observed entries over the valid pairs
    (rows of different completeness are scores of different dimension, which the plain mean mixes)."""
    n, T, K1, _ = y_mean.shape
    out = np.full((4 if missing_obs else 3, K1), np.nan)
    for k in range(min(K1, T)):
        y, m, v = obs[:, k:], y_mean[:, :T - k, k], y_var[:, :T - k, k]
        if missing_obs:
            seen = ~np.isnan(y)
            n_obs = seen.sum(axis=-1)                   # (n, T - k) observed entries of every target row
            pairs = n_obs > 0
            if not pairs.any():
                continue
            lp = lpd[:, :T - k, k]
            out[0, k] = float(np.mean(lp[pairs]))
            out[1, k] = _r_square(m, y, missing_obs=True)
            out[2, k] = float(np.mean((np.square(np.where(seen, y, 0.0) - m) / v)[seen]))
            out[3, k] = float(np.sum(lp[pairs])) / float(np.sum(n_obs))
            continue
        out[0, k] = float(np.mean(lpd[:, :T - k, k]))
        out[1, k] = _r_square(m, y)
        out[2, k] = float(np.mean(np.square(y - m) / v))
    return tuple(out)


def _collate(per_batch, keepdims):
    """values of ONE fetch over the evaluation batches -> one array (or list of arrays for a list-valued fetch)"""
    first = per_batch[0]
    if isinstance(first, np.ndarray):
        return np.stack(per_batch) if keepdims else np.concatenate(per_batch)
    if isinstance(first, list):                       # k-step predictions: one array per horizon
        return [np.concatenate(col) for col in zip(*per_batch)]
    return np.asarray(per_batch)                      # scalars (log_ZSMC of each batch)


class trainer:
    INPUTS = "inputs"       # feed key of the exogenous inputs (FLAGS.Di > 0), beside self.obs / self.hidden

    # schedule state, reference names (trainer.py:63-80): bestCost = index of the best validation ELBO so far,
    # *_count = evaluations since it improved
    def __init__(self, model, SMC, FLAGS):
        self.model, self.SMC, self.FLAGS = model, SMC, FLAGS
        for name in ("Dx", "Dy", "time", "n_particles", "MSE_steps"):
            setattr(self, name, getattr(FLAGS, name))
        self.save_res = False
        self.draw_quiver_during_training = False
        self.init_placeholder()
        self.init_training_param()
        self.device = next(model.parameters()).device
        self.flat = None
        self.optimizer = None

    def init_placeholder(self):
        self.obs = self.model.obs
        self.hidden = self.model.hidden

    def init_training_param(self):
        F = self.FLAGS
        self.batch_size, self.lr, self.epoch = F.batch_size, F.lr, F.epoch
        self.early_stop_patience = F.early_stop_patience
        self.lr_reduce_factor, self.lr_reduce_patience, self.min_lr = F.lr_reduce_factor, F.lr_reduce_patience, F.min_lr
        self.bestCost = self.early_stop_count = self.lr_reduce_count = 0

    def init_data_saving(self, RLT_DIR):
        F = self.FLAGS
        self.save_res, self.RLT_DIR = True, RLT_DIR
        self.save_trajectory, self.save_y_hat, self.saving_num = F.save_trajectory, F.save_y_hat, F.saving_num
        self.save_tensorboard, self.save_model = F.save_tensorboard, F.save_model
        self.log_ZSMC_trains, self.log_ZSMC_tests, self.R_square_trains, self.R_square_tests = [], [], [], []
        # per-epoch artefacts live in a sibling tree: .../rslts/<...> -> .../rslts/epoch_data/<...> (trainer.py:93-95)
        parts = RLT_DIR.split("/")
        at = parts.index("rslts") + 1
        self.epoch_data_DIR = "/".join(parts[:at] + ["epoch_data"] + parts[at:])

    # ------------------------------------------------------------------------------------------
    def _to_dev(self, a):
        return torch.as_tensor(np.asarray(a), dtype=torch.float32, device=self.device)

    def _local(self, a):
        """this rank's shard of one mini-batch (contiguous, equal shards)"""
        lo, hi = dp.shard(len(a))
        return a[lo:hi]

    def train_step(self, obs_batch, hidden_batch, lr, inputs_batch=None):
        """one sess.run(train_op) of the reference (trainer.py:147-151).  inputs_batch: the exogenous inputs of the batch
        (FLAGS.Di > 0), moved and sliced with the observations.

        On the GPU the local part of the step (zero the gradient buffer, objective, reverse pass: ~90 launches on three
        streams) is captured once per batch shape into a hipGraph and replayed with the batch copied into static
        buffers; the gradient all-reduce and Adam (whose step count and learning rate change) stay outside the graph.
        PSVO_HIPGRAPH=0, or a failed capture, issues everything eagerly."""
        obs = self._to_dev(self._local(obs_batch))
        hidden = self._to_dev(self._local(hidden_batch))
        inputs = None if inputs_batch is None else self._to_dev(self._local(inputs_batch))
        extra = {} if inputs is None else {"inputs": inputs}
        log_ZSMC = self._graphed_local_step(obs, hidden, inputs)
        if log_ZSMC is None:
            self.flat.zero_grad()
            log_ZSMC, _ = self.SMC.get_log_ZSMC(obs, hidden, **extra)
            with autograd.deferred_join():
                log_ZSMC.backward()
        dp.all_reduce_sum_(self.flat.grad)
        self.optimizer.step(lr, world_size=dp.world_size())
        return log_ZSMC.detach()

    def _graphed_local_step(self, obs, hidden, inputs=None):
        """replay (capturing on first use) the hipGraph of the local step for this batch shape; None = run eagerly.
        inputs (FLAGS.Di > 0): a static buffer beside the observations'."""
        import os
        if (not obs.is_cuda or os.environ.get("PSVO_HIPGRAPH", "1") == "0"
                or getattr(self.SMC, "generator", None) is None):
            return None      # (a CPU generator cannot be registered with the graph)
        graphs = self.__dict__.setdefault("_graphs", {})
        key = (tuple(obs.shape), tuple(hidden.shape)) + (() if inputs is None else (tuple(inputs.shape),))
        g = graphs.get(key)
        if g is None:
            try:
                from .graph import GraphedStep
                s_obs, s_hidden = obs.clone(), hidden.clone()
                s_inputs = None if inputs is None else inputs.clone()
                s_extra = {} if inputs is None else {"inputs": s_inputs}

                def local_step():
                    self.flat.zero_grad()
                    z, _ = self.SMC.get_log_ZSMC(s_obs, s_hidden, **s_extra)
                    with autograd.deferred_join():
                        z.backward()
                    return z.detach()
                g = (GraphedStep(local_step, generators=[self.SMC.generator]), s_obs, s_hidden, s_inputs)
            except Exception as exc:     # fall back to eager issue for this shape from now on
                if dp.rank() == 0:
                    print("hipGraph capture of the training step failed (%s: %s); issuing eagerly"
                          % (type(exc).__name__, str(exc)[:100]))
                torch.cuda.synchronize()
                g = False
            graphs[key] = g
        if g is False:
            return None
        step, s_obs, s_hidden, s_inputs = g
        s_obs.copy_(obs)
        s_hidden.copy_(hidden)
        if s_inputs is not None:
            s_inputs.copy_(inputs)
        return step()

    def train(self, obs_train, obs_test, hidden_train, hidden_test, print_freq, inputs_train=None, inputs_test=None):
        """inputs_train / inputs_test (n, T, Di): the exogenous inputs of a model with FLAGS.Di > 0; they are shuffled, sliced
        and moved with the observations wherever those are."""
        self.obs_train, self.obs_test = obs_train, obs_test
        self.hidden_train, self.hidden_test = hidden_train, hidden_test
        if int(getattr(self.SMC, "Di", 0) or 0) > 0 and (inputs_train is None or inputs_test is None):
            raise ValueError("--Di = %d: train() needs inputs_train and inputs_test beside the observations" % self.SMC.Di)
        self.inputs_train, self.inputs_test = inputs_train, inputs_test

        assert self.batch_size % dp.world_size() == 0, "batch_size must split evenly over the ranks"
        self.flat = FlatParams(self.model)
        dp.broadcast_(self.flat.flat)
        self.optimizer = TFAdam(self.flat, clip_norm=getattr(self.FLAGS, "clip_norm", 0.0),     # tf.train.AdamOptimizer(lr), trainer.py:117
                                skip_nonfinite=getattr(self.FLAGS, "skip_nonfinite_steps", False))
        self._guard_seen = {"applied": 0, "clipped": 0, "skipped": 0}
        self.guard_intervals = []                                # one dict of guard_* numbers per evaluation (guard on)
        log = {"Xs": "Xs", "y_hat": "y_hat"}
        verbose = dp.rank() == 0
        check_exchange = getattr(self.SMC, "check_exchange", None)   # (PSVOwR: sticky flag of the kernels' bounded polls)

        for i in range(self.epoch):
            start = time.time()
            if i == 0:
                self.evaluate_and_save_metrics(i)

            if inputs_train is None:
                obs_train, hidden_train = _shuffle(obs_train, hidden_train)
            else:       # (one shared permutation, the same draw from numpy's generator as without inputs)
                obs_train, hidden_train, inputs_train = _shuffle(obs_train, hidden_train, inputs_train)
            for j in range(0, len(obs_train), self.batch_size):
                if inputs_train is None:
                    self.train_step(obs_train[j:j + self.batch_size], hidden_train[j:j + self.batch_size], self.lr)
                else:
                    self.train_step(obs_train[j:j + self.batch_size], hidden_train[j:j + self.batch_size], self.lr,
                                    inputs_batch=inputs_train[j:j + self.batch_size])
            if check_exchange is not None:
                check_exchange()                                 # every epoch: a timed-out exchange means garbage gradients

            if (i + 1) % print_freq == 0:
                if not dp.replicas_in_sync(self.flat.flat):
                    raise RuntimeError("data-parallel replicas diverged (parameters differ between ranks)")
                try:
                    self.evaluate_and_save_metrics(i)
                    self.adjust_lr(i, print_freq)
                except StopTraining:
                    break
                if self.save_res:
                    self._save_epoch_samples(i + 1, obs_test, hidden_test, verbose)
            if verbose:
                print("epoch {:<4} took {:.3f} seconds".format(i + 1, time.time() - start))

        if verbose:
            print("finished training...")
        metrics = {}
        if self.save_res:
            metrics = {k: getattr(self, k) for k in ("log_ZSMC_trains", "log_ZSMC_tests", "R_square_trains", "R_square_tests")}
        return metrics, log

    def _save_epoch_samples(self, epoch, obs_test, hidden_test, write):
        """trajectory_<epoch>.p / y_hat_<epoch>.p for the first saving_num held-out sequences (trainer.py:170-186) and, for
        two-dimensional latents, lattice_val_<epoch>.p -- the data behind the reference's quiver plot (trainer.py:337-361),
        which its notebook reads back (notebooks/PSVO.ipynb: `lattice_dict["X_trajs"], ["X"], ["nextX"]`)."""
        self.saving_feed_dict = {self.obs: obs_test[:self.saving_num], self.hidden: hidden_test[:self.saving_num]}
        if getattr(self, "inputs_test", None) is not None:
            self.saving_feed_dict[self.INPUTS] = self.inputs_test[:self.saving_num]
        Xs_val = None
        forecast = bool(getattr(self.SMC, "forecast", False))
        map_path = bool(getattr(self.SMC, "MAP_path", False))
        for flag, fetch, stem in ((self.save_trajectory, "Xs", "trajectory"), (self.save_y_hat, "y_hat", "y_hat")):
            if not flag:
                continue
            extra = {}
            if forecast and fetch == "y_hat":      # (FLAGS.particle_forecast: the predictive moments beside the point forecast)
                val, extra["y_mean"], extra["y_var"] = self.evaluate([fetch, "forecast_y_mean", "forecast_y_var"],
                                                                     self.saving_feed_dict, average=False)
            elif map_path and fetch == "Xs":       # (FLAGS.MAP_path: the decoded path beside the cloud)
                val, extra["X_map"], extra["map_index"] = self.evaluate([fetch, "X_map", "map_index"], self.saving_feed_dict,
                                                                        average=False)
            else:
                val = self.evaluate(fetch, self.saving_feed_dict, average=False)      # (collective: every rank takes part)
            if fetch == "Xs":
                Xs_val = val
            if write:
                with open(self.epoch_data_DIR + "{}_{}.p".format(stem, epoch), "wb") as f:
                    pickle.dump(dict({fetch: val}, **extra), f)
        if self.Dx == 2 and Xs_val is not None:      # (the reference draws from the trajectories it has just saved)
            lattice = self.quiver_lattice(Xs_val)
            if write:
                with open(self.epoch_data_DIR + "lattice_val_{}.p".format(epoch), "wb") as f:
                    pickle.dump(lattice, f)

    def quiver_lattice(self, Xs_val, shape=(25, 25), margin=0.05):
        """{"X_trajs", "X", "nextX"} of trainer.draw_2D_quiver_plot (trainer.py:337-361) without the figure: the particle-mean
        trajectories (saving_num, T, 2), a 25 x 25 lattice over their bounding box and f.mean on it (SMC.get_nextX).  The
        reference takes the box from the axes of its plot of those trajectories, i.e. the data range widened by matplotlib's
        default 5 % margin on either side; that is restated here."""
        X_trajs = np.mean(np.asarray(Xs_val), axis=2)[:self.saving_num]
        lo, hi = X_trajs.reshape(-1, 2).min(axis=0), X_trajs.reshape(-1, 2).max(axis=0)
        pad = margin * (hi - lo)
        x1 = np.linspace(lo[0] - pad[0], hi[0] + pad[0], num=shape[0])
        x2 = np.linspace(lo[1] - pad[1], hi[1] + pad[1], num=shape[1])
        X = np.stack(np.meshgrid(x1, x2), axis=-1)                         # (25, 25, 2), trainer.define2Dlattice
        with torch.no_grad():
            nextX = self.SMC.get_nextX(self._to_dev(X.reshape(-1, 2))).reshape(shape[1], shape[0], 2).cpu().numpy()
        return {"X_trajs": X_trajs, "X": X, "nextX": nextX}

    def close_session(self):
        """the reference closes its tf.Session here (trainer.py:197-198).  Here: release the captured hipGraphs of the training
        step at a quiescent point -- after a device synchronisation, by the caller -- instead of whenever the cycle collector
        reaches this object, which may be in the middle of another trainer's replays (runner.main calls it on its way out)."""
        graphs = self.__dict__.pop("_graphs", None)
        if graphs:
            torch.cuda.synchronize()
            graphs.clear()

    def evaluate_and_save_metrics(self, iter_num, y_hat_N_BxTxDy=None, y_N_BxTxDy=None):
        """ELBO and k-step R-square on the training and held-out sets; appended to the histories and pickled as
        metric_<iter>.p with the reference's keys (trainer.py:201-241).  A non-finite training ELBO stops training."""
        ffbs = bool(getattr(self.SMC, "FFBS", False))
        ffbsi = bool(getattr(self.SMC, "FFBSi", False))
        adaptive = bool(getattr(self.SMC, "resample_ess", 0.0))
        forecast = bool(getattr(self.SMC, "forecast", False))
        missing = bool(getattr(self.SMC, "missing_obs", False))
        map_path = bool(getattr(self.SMC, "MAP_path", False))
        fetches = (["log_ZSMC", "y_hat", "y"] + (["ess", "resampled"] if adaptive else []) + (["ess_smooth"] if ffbs else [])
                   + (["path_distinct"] if ffbsi else []) + (["map_score"] if map_path else []))
        if forecast:       # (last, so that the fetches ahead of them keep their places)
            fetches += ["forecast_y_mean", "forecast_y_var", "forecast_lpd"]
        m, ess = {}, {}
        for split, obs, hid in (("train", self.obs_train, self.hidden_train), ("test", self.obs_test, self.hidden_test)):
            feed = {self.obs: obs, self.hidden: hid}
            if getattr(self, "inputs_" + split, None) is not None:
                feed[self.INPUTS] = getattr(self, "inputs_" + split)
            elbos, y_hat, y, *rest = self.evaluate(fetches, feed)
            if forecast:
                fc, rest = rest[-3:], rest[:-3]
                lpd, rsq, cal, *per_entry = _forecast_metrics(*fc, np.asarray(obs, dtype=np.float32), missing_obs=missing)
                ess["forecast_lpd_" + split], ess["forecast_R_square_" + split] = lpd, rsq
                ess["forecast_calibration_" + split] = cal
                if missing:     # (FLAGS.particle_forecast_missing_obs: the score per observed entry)
                    ess["forecast_lpd_per_entry_" + split] = per_entry[0]
            if map_path:    # (behind the forecast's three, ahead of everything else: the fetches before it keep their places)
                score, rest = rest[-1], rest[:-1]
                ess["map_score_" + split] = float(np.mean(np.asarray(score, dtype=np.float64) / np.asarray(obs).shape[1]))
            if adaptive:
                frac, rest = np.asarray(rest[0]) / float(self.n_particles), rest[1:]
                ess["adaptive_rate_" + split] = float(np.mean(rest[0]))
                ess["adaptive_ess_mean_" + split], ess["adaptive_ess_min_" + split] = float(np.mean(frac)), float(np.min(frac))
                rest = rest[1:]
            if ffbs:
                ess["ffbs_ess_mean_" + split], ess["ffbs_ess_min_" + split] = float(np.mean(rest[0])), float(np.min(rest[0]))
            if ffbsi:
                ess["ffbsi_distinct_mean_" + split], ess["ffbsi_distinct_min_" + split] = float(np.mean(rest[-1])), float(np.min(rest[-1]))
            if missing:     # the share of entries of this split that were not observed
                ess["missing_share_" + split] = float(np.mean(np.isnan(np.asarray(obs, dtype=np.float64))))
            m["log_ZSMC_" + split] = np.mean(elbos)
            m["R_square_" + split] = self.evaluate_R_square(y_hat, y)

        if dp.rank() == 0:
            print()
            print("iter", iter_num + 1)
            print("Train log_ZSMC: {:>7.3f}, valid log_ZSMC: {:>7.3f}".format(m["log_ZSMC_train"], m["log_ZSMC_test"]))
            print("Train, Valid k-step Rsq:\n", m["R_square_train"], "\n", m["R_square_test"])
            if missing:
                print("missing observations: share of entries not observed train {:.1%}, valid {:.1%}"
                      .format(ess["missing_share_train"], ess["missing_share_test"]))
            if adaptive:
                print("adaptive resampling (ESS < {:g} N): resampled steps train {:.1%}, valid {:.1%}; ESS / N mean / min: train "
                      "{:.3f} / {:.3f}, valid {:.3f} / {:.3f}"
                      .format(self.SMC.resample_ess, ess["adaptive_rate_train"], ess["adaptive_rate_test"],
                              ess["adaptive_ess_mean_train"], ess["adaptive_ess_min_train"],
                              ess["adaptive_ess_mean_test"], ess["adaptive_ess_min_test"]))
            if ffbs:
                print("FFBS effective sample size (of {} particles), mean / min: train {:.2f} / {:.2f}, valid {:.2f} / {:.2f}"
                      .format(self.n_particles, ess["ffbs_ess_mean_train"], ess["ffbs_ess_min_train"],
                              ess["ffbs_ess_mean_test"], ess["ffbs_ess_min_test"]))
            if ffbsi:
                print("FFBSi distinct particles per step (of {}), mean / min: train {:.2f} / {:.0f}, valid {:.2f} / {:.0f}"
                      .format(self.n_particles, ess["ffbsi_distinct_mean_train"], ess["ffbsi_distinct_min_train"],
                              ess["ffbsi_distinct_mean_test"], ess["ffbsi_distinct_min_test"]))

            if map_path:
                print("MAP path: joint log-density per time step, train {:.4f}, valid {:.4f}"
                      .format(ess["map_score_train"], ess["map_score_test"]))

            if forecast:
                print("particle forecast, k = 0 .. {}: predictive log-density train, valid:\n".format(self.MSE_steps),
                      ess["forecast_lpd_train"], "\n", ess["forecast_lpd_test"])
                print("particle forecast Rsq train, valid:\n", ess["forecast_R_square_train"], "\n", ess["forecast_R_square_test"])
                print("particle forecast calibration (1 = calibrated) train, valid:\n", ess["forecast_calibration_train"], "\n",
                      ess["forecast_calibration_test"])
                if missing:
                    print("particle forecast predictive log-density per observed entry train, valid:\n",
                          ess["forecast_lpd_per_entry_train"], "\n", ess["forecast_lpd_per_entry_test"])

        if not math.isfinite(m["log_ZSMC_train"]):
            print("Nan in log_ZSMC, stop training")
            raise StopTraining()

        guard = self._guard_interval()
        if self.save_res:
            for key, val in m.items():
                getattr(self, key + "s").append(val)
            if dp.rank() == 0:
                os.makedirs(self.epoch_data_DIR, exist_ok=True)
                with open(self.epoch_data_DIR + "metric_{}.p".format(iter_num + 1), "wb") as f:
                    pickle.dump(dict(m, **guard, **ess), f)
        if guard and guard["guard_skipped"] > 0 and guard["guard_applied"] == 0:
            msg = ("every one of the {} training steps since the last evaluation had a non-finite gradient norm and was "
                   "skipped: the model can no longer produce a finite gradient, stop training".format(guard["guard_skipped"]))
            if dp.rank() == 0:
                print(msg)
            raise StopTraining(msg)
        return m["log_ZSMC_train"], m["log_ZSMC_test"], m["R_square_train"], m["R_square_test"]

    def _guard_interval(self):
        """{} with the guard off; else the optimizer's counts since the previous evaluation and its last / largest finite
        gradient norm, as the guard_* keys of metric_<iter>.p (one device read; printed by rank 0; every rank holds the same
        numbers because every rank steps on the same all-reduced gradient)"""
        stats = self.optimizer.guard_stats() if self.optimizer is not None else None
        if stats is None:
            return {}
        out = {"guard_last_norm": stats["last_norm"], "guard_max_norm": stats["max_norm"]}
        for key in ("applied", "clipped", "skipped"):
            out["guard_" + key] = stats[key] - self._guard_seen[key]
            self._guard_seen[key] = stats[key]
        self.guard_intervals.append(out)
        if dp.rank() == 0:
            print("gradient guard: last norm {:.4g}, largest norm {:.4g}; since the last evaluation {} steps applied "
                  "({} of them clipped), {} skipped".format(out["guard_last_norm"], out["guard_max_norm"], out["guard_applied"],
                                                            out["guard_clipped"], out["guard_skipped"]))
        return out

    def adjust_lr(self, iter_num, print_freq):
        """Plateau schedule on the held-out ELBO history (trainer.py:244-270): whenever the best evaluation moves, both
        patience counters restart; while the latest evaluation is not the best one, each counter advances, training stops
        when early_stop_count * print_freq hits early_stop_patience exactly, and the learning rate is multiplied by
        lr_reduce_factor (floored at min_lr) each time lr_reduce_count * print_freq hits lr_reduce_patience."""
        history = self.log_ZSMC_tests
        best, latest = int(np.argmax(history)), len(history) - 1
        if best != self.bestCost:
            self.bestCost, self.early_stop_count, self.lr_reduce_count = best, 0, 0
        talk = dp.rank() == 0
        if talk:
            print("best valid cost on iter: {}\n".format(self.bestCost * print_freq))

        if best != latest:
            self.early_stop_count += 1
            self.lr_reduce_count += 1
            if self.early_stop_count * print_freq == self.early_stop_patience:
                if talk:
                    print("valid cost not improving. stopping training...")
                raise StopTraining()
            if self.lr_reduce_count * print_freq == self.lr_reduce_patience:
                self.lr_reduce_count = 0
                self.lr = max(self.lr * self.lr_reduce_factor, self.min_lr)
                if talk:
                    print("valid cost not improving. reduce learning rate to {}".format(self.lr))
        elif self.save_model and talk:
            os.makedirs(self.RLT_DIR + "model/", exist_ok=True)
            print("Test log_ZSMC improves to {}, save model".format(history[-1]))
            torch.save(self.model.state_dict(), self.RLT_DIR + "model/model_epoch_{}.pt".format(iter_num + 1))

    # ------------------------------------------------------------------------------------------
    def _run(self, names, obs, hidden, inputs=None):
        """one forward evaluation of a batch (sess.run(fetches) of the reference); inputs: its exogenous inputs (FLAGS.Di > 0)"""
        with torch.no_grad():
            obs_d = self._to_dev(obs)
            extra = {} if inputs is None else {"inputs": self._to_dev(inputs)}
            log_ZSMC, log = self.SMC.get_log_ZSMC(obs_d, self._to_dev(hidden), **extra)
            out = {"log_ZSMC": float(log_ZSMC)}
            if any(n in names for n in ("Xs", "y_hat", "y")):
                Xs = log["Xs"]
                out["Xs"] = Xs.contiguous().cpu().numpy()
                if "y_hat" in names or "y" in names:
                    y_hat, y = self.SMC.n_step_prediction(self.MSE_steps, Xs, obs_d, **extra)
                    out["y_hat"] = [v.cpu().numpy() for v in y_hat]
                    out["y"] = [v.cpu().numpy() for v in y]
            if any(n.startswith("forecast_") for n in names):       # FLAGS.particle_forecast only
                fc = self.SMC.particle_forecast(self.MSE_steps, log["Xs"], obs_d, **extra)
                out["forecast_y_mean"] = fc["y_mean"].contiguous().cpu().numpy()      # (B, T, K+1, Dy)
                out["forecast_y_var"] = fc["y_var"].contiguous().cpu().numpy()
                out["forecast_lpd"] = fc["lpd"].contiguous().cpu().numpy()            # (B, T, K+1); 0 where t + k >= T
            if "ess" in names:
                out["ess"] = log["ess"].contiguous().cpu().numpy()                    # (B, T); FLAGS.resample_ess only
            if "resampled" in names:
                out["resampled"] = log["resampled"].contiguous().cpu().numpy()        # (B, T) bool
            if "ess_smooth" in names:
                out["ess_smooth"] = log["ess_smooth"].contiguous().cpu().numpy()      # (B, T); FLAGS.FFBS only
            if "path_distinct" in names:
                out["path_distinct"] = log["path_distinct"].contiguous().cpu().numpy()      # (B, T) int32; FLAGS.FFBSi only
            if "map_score" in names:
                out["map_score"] = log["map_score"].cpu().numpy()                     # (B,) fp64; FLAGS.MAP_path only
            if "X_map" in names:
                out["X_map"] = log["X_map"].contiguous().cpu().numpy()                # (B, T, Dx)
            if "map_index" in names:
                out["map_index"] = log["map_index"].contiguous().cpu().numpy()        # (B, T) int32
        return [out[n] for n in names]

    def evaluate(self, fetches, feed_dict_w_batches={}, average=False, keepdims=False):
        """Evaluate `fetches` (a name or a list of names) over feed_dict_w_batches in mini-batches of batch_size (a short
        last batch is evaluated as it is) and join the results: arrays are concatenated over the batch axis (stacked with
        keepdims), list-valued fetches element-wise, scalars become a vector with one entry per batch; `average` then takes
        the mean over the leading axis.  Semantics of the reference's trainer.evaluate (trainer.py:272-320).
        With W ranks the batches are dealt round-robin (batch k to rank k mod W) and gathered, so every rank returns the
        full result."""
        single = not isinstance(fetches, list)
        names = [fetches] if single else list(fetches)
        obs_all, hid_all = feed_dict_w_batches[self.obs], feed_dict_w_batches[self.hidden]
        v_all = feed_dict_w_batches.get(self.INPUTS)          # the exogenous inputs (FLAGS.Di > 0), or None
        n = len(obs_all)
        assert n >= self.batch_size
        starts = list(range(0, n, self.batch_size))
        W, r = dp.world_size(), dp.rank()
        cut = lambda s: {} if v_all is None else {"inputs": v_all[s:s + self.batch_size]}
        mine = {k: self._run(names, obs_all[s:s + self.batch_size], hid_all[s:s + self.batch_size], **cut(s))
                for k, s in enumerate(starts) if k % W == r}
        if W > 1:
            import torch.distributed as dist
            parts = [None] * W
            dist.all_gather_object(parts, mine)
            mine = {k: v for part in parts for k, v in part.items()}
        rows = [mine[k] for k in range(len(starts))]

        res = [_collate([row[i] for row in rows], keepdims) for i in range(len(names))]
        if average:
            res = [[np.mean(a, axis=0) for a in x] if isinstance(x, list) else np.mean(x, axis=0) for x in res]
        return res[0] if single else res

    def evaluate_R_square(self, y_hat, y):
        """R-square of the k-step-ahead predictions, k = 0 .. MSE_steps (trainer.py:322-335): one number per horizon"""
        missing = bool(getattr(getattr(self, "SMC", None), "missing_obs", False))
        return np.array([_r_square(np.asarray(p), np.asarray(t), missing) for p, t in zip(y_hat, y)])
