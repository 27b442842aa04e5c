"""SVO -- mirror of reference src/SMC/SVO.py:6-409.

The forward particle filter (SVO.SMC, :60-180, with sample_from_2_dist :182-232 and
resample_X / get_resample_idx :243-300) runs as ONE persistent HIP kernel
(psvo_filter_forward, psvo_amd/csrc/filter_fwd.hip).  This class only prepares what does not
depend on the particles -- encoder features and the hoisted q0 / q2 means, B*T rows -- and
permutes the result to the reference's (batch, time, particles, Dx).
"""
import torch

from .. import ops
from ..autograd import (FilterAdaptiveFunction, FilterCovFunction, FilterFunction, FilterWobsAdaptiveFunction,
                        FilterWobsFunction, FilterWobsInputAdaptiveFunction, FilterWobsInputFunction,
                        FilterWobsMissingAdaptiveFunction, FilterWobsMissingBsimFunction, FilterWobsMissingFunction)


def check_resample_ess(raw, never_resamples=False, backward_simulation=False, output_cov=False, Dy=1, plain_dy=2,
                       wide_obs=False, layers=(), wobs_max_dy=32, missing_obs=False, inputs=False):
    """--resample_ess as a float: 0.0 = off, else the ESS threshold tau as a fraction of N, 0 < tau <= 1.  ValueError, naming
    the limit, for a threshold outside that range and for everything the adaptive kernels do not cover (runner.main calls this
    on the flags before it touches a device, SVO.__init__ on the model it is given).  `wide_obs`: --resample_ess_wide_obs, the
    adaptive wide-observation kernels for plain_dy < Dy <= wobs_max_dy (`layers`: the hidden layers of the per-particle MLPs,
    one each there); no effect at Dy <= plain_dy or with the threshold off.  `missing_obs`: --missing_obs with
    --resample_ess_missing_obs, the adaptive missing-observation kernels at every width check_missing_obs accepts (which also
    checks width and depth there); `wide_obs` is not needed and has no effect then.  `inputs`: --Di > 0 with
    --resample_ess_inputs, the adaptive input-driven kernels at every width check_inputs accepts (which also checks width and
    depth there); `wide_obs` is not needed then either."""
    tau = float(0.0 if raw is None else raw)
    if tau == 0.0:
        return 0.0
    if not (0.0 < tau <= 1.0):
        raise ValueError("--resample_ess = %r: the ESS threshold is a fraction of the particle count, 0 < tau <= 1 "
                         "(0 = off: resample at every step)" % (raw,))
    if never_resamples:
        raise ValueError("--resample_ess with --IWAE: IWAE never resamples, so there is no resampling decision to make; "
                         "use --AESMC or --SVO")
    if backward_simulation:
        raise ValueError("--resample_ess with --PSVO / --PSVOwR: the backward-simulation kernels assume a filter that "
                         "resamples at every step; adaptive resampling covers the filter objectives (SVO, AESMC) only")
    if output_cov:
        raise ValueError("--resample_ess with output_cov: the state-dependent-scale kernels (psvo_filter_forward_cov) have "
                         "no adaptive form; adaptive resampling takes state-independent scales only")
    if missing_obs or inputs:
        return tau
    if Dy > plain_dy and not wide_obs:
        raise ValueError("--resample_ess with Dy = %d: without --resample_ess_wide_obs the adaptive kernels are the plain filter "
                         "kernels, which take Dy <= %d; pass --resample_ess_wide_obs for the adaptive wide-observation kernels "
                         "(3 <= Dy <= %d)" % (Dy, plain_dy, wobs_max_dy))
    if Dy > wobs_max_dy:
        raise ValueError("--resample_ess --resample_ess_wide_obs with Dy = %d: the adaptive wide-observation kernels take "
                         "3 <= Dy <= %d" % (Dy, wobs_max_dy))
    if Dy > plain_dy:
        deep = [v for v in (_layer_list(s) for s in layers) if len(v) != 1]
        if deep:
            raise ValueError("--resample_ess --resample_ess_wide_obs with Dy = %d and per-particle MLP layers %s: the adaptive "
                             "wide-observation kernels take one hidden layer per MLP; two hidden layers run for Dy <= %d only"
                             % (Dy, deep, plain_dy))
    return tau


def check_missing_obs(on, missing_rate=0.0, backward_simulation=False, resample_ess=0.0, particle_forecast=False,
                      output_cov=False, Dy=1, layers=(), wobs_max_dy=32, resample_ess_missing_obs=False,
                      particle_forecast_missing_obs=False, bsim_missing_obs=False, cross_chain=False):
    """--missing_obs (a NaN observation is an entry that was not observed) as a bool.  ValueError, naming the limit, for
    everything the missing-observation kernels (psvo_filter_forward_wobs_missing) do not cover and for a --missing_rate that is
    no probability or has nothing to act on (runner.main calls this on the flags before it touches a device, SVO.__init__ on the
    model it is given).  `layers`: the hidden layers of the per-particle MLPs, one each.  `resample_ess_missing_obs`
    (--resample_ess_missing_obs): --resample_ess runs on psvo_filter_forward_wobs_missing_adaptive; `particle_forecast_missing_obs`
    (--particle_forecast_missing_obs): --particle_forecast runs on psvo_particle_forecast_missing.  Neither has an effect without
    --missing_obs, and without them the two combinations stay refused.  `bsim_missing_obs` (--BSim_missing_obs): PSVO runs its
    backward simulation on psvo_bsim_forward_wobs_missing / psvo_bsim_backward_wobs_missing behind that filter; without it
    PSVO stays refused, and PSVOwR (`cross_chain`: the objective resamples across chains) stays refused with it.  No effect
    without --missing_obs."""
    rate = float(0.0 if missing_rate is None else missing_rate)
    if not (0.0 <= rate < 1.0):
        raise ValueError("--missing_rate = %r: the probability of knocking an entry out lies in [0, 1)" % (missing_rate,))
    if not on:
        if rate != 0.0:
            raise ValueError("--missing_rate without --missing_obs: the knocked-out entries are NaN, which only the "
                             "missing-observation route scores; pass --missing_obs")
        return False
    limit = "missing observations run on psvo_filter_forward_wobs_missing, the filter of SVO / AESMC / IWAE"
    if backward_simulation and not bsim_missing_obs:
        raise ValueError("--missing_obs with --PSVO / --PSVOwR: %s; the backward-simulation kernels evaluate the emission too and "
                         "have no missing-observation form" % limit)
    if backward_simulation:
        # --BSim_missing_obs: psvo_bsim_forward_wobs_missing behind the missing-observation filter, PSVO only
        limit = ("missing observations under PSVO run on psvo_filter_forward_wobs_missing and psvo_bsim_forward_wobs_missing "
                 "(--BSim_missing_obs)")
        if cross_chain:
            raise ValueError("--missing_obs --BSim_missing_obs with --PSVOwR: --BSim_missing_obs covers PSVO only; the cross-chain "
                             "resampling kernels of PSVOwR have no missing-observation form")
        if float(resample_ess or 0.0) != 0.0:
            raise ValueError("--missing_obs --BSim_missing_obs with --resample_ess under --PSVO: the backward-simulation kernels "
                             "assume a filter that resamples at every step; the adaptive missing-observation kernels cover the "
                             "filter objectives (SVO, AESMC) only")
    if float(resample_ess or 0.0) != 0.0 and not resample_ess_missing_obs:
        raise ValueError("--missing_obs with --resample_ess: %s, which resamples at every step (or never); the adaptive kernels "
                         "have no missing-observation form" % limit)
    if particle_forecast and not particle_forecast_missing_obs:
        raise ValueError("--missing_obs with --particle_forecast: the forecast's predictive log-density (lpd) scores whole "
                         "observation rows; it has no missing-observation form")
    if output_cov:
        raise ValueError("--missing_obs with output_cov: %s, which takes state-independent scales; the state-dependent-scale "
                         "kernels have no missing-observation form" % limit)
    if Dy > wobs_max_dy or Dy < 1:
        raise ValueError("--missing_obs with Dy = %d: %s, which takes 1 <= Dy <= %d; no fallback path exists"
                         % (Dy, limit, wobs_max_dy))
    deep = [v for v in (_layer_list(s) for s in layers) if len(v) != 1]
    if deep:
        raise ValueError("--missing_obs with per-particle MLP layers %s: %s, which takes one hidden layer per MLP; two hidden "
                         "layers have no missing-observation form" % (deep, limit))
    return True


def check_inputs(Di, backward_simulation=False, resample_ess=0.0, particle_forecast=False, output_cov=False, Dy=1, layers=(),
                 wobs_max_dy=32, particle_forecast_inputs=False, resample_ess_inputs=False):
    """--Di (the width of the exogenous input v_t that drives f and q1) as an int, 0 = off.  ValueError, naming the limit, for a
    negative width and for everything the input-driven kernels (psvo_filter_forward_wobs_input) do not cover (runner.main calls
    this on the flags before it touches a device, SVO.__init__ on the model it is given).  `layers`: the hidden layers of the
    per-particle MLPs, one each.  `particle_forecast_inputs` (--particle_forecast_inputs): --particle_forecast runs on
    psvo_particle_forecast_input; `resample_ess_inputs` (--resample_ess_inputs): --resample_ess runs on
    psvo_filter_forward_wobs_input_adaptive (SVO, AESMC).  Without them the two combinations stay refused, and neither has an
    effect at Di = 0."""
    Di = int(0 if Di is None else Di)
    if Di < 0:
        raise ValueError("--Di = %d: the input dimension is a count, Di >= 0 (0 = autonomous dynamics)" % Di)
    if Di == 0:
        return 0
    limit = "exogenous inputs run on psvo_filter_forward_wobs_input, the filter of SVO / AESMC / IWAE"
    if backward_simulation:
        raise ValueError("--Di with --PSVO / --PSVOwR: %s; the backward simulations' own proposal networks have no input form"
                         % limit)
    if float(resample_ess or 0.0) != 0.0 and not resample_ess_inputs:
        raise ValueError("--Di with --resample_ess: %s, which resamples at every step (or never); the adaptive kernels have no "
                         "input form" % limit)
    if particle_forecast and not particle_forecast_inputs:
        raise ValueError("--Di with --particle_forecast: the forecast kernel (psvo_particle_forecast) propagates the cloud through "
                         "an autonomous f; it has no input form")
    if output_cov:
        raise ValueError("--Di with output_cov: %s, which takes state-independent scales; the state-dependent-scale kernels have "
                         "no input form" % limit)
    deep = [v for v in (_layer_list(s) for s in layers) if len(v) != 1]
    if deep:
        raise ValueError("--Di with per-particle MLP layers %s: %s, which takes one hidden layer per MLP; two hidden layers have "
                         "no input form" % (deep, limit))
    if Dy > wobs_max_dy or Dy < 1:
        raise ValueError("--Di with Dy = %d: %s, which takes 1 <= Dy <= %d; no fallback path exists" % (Dy, limit, wobs_max_dy))
    return Di


def check_map_path(on, backward_simulation=False, output_cov=False, Dy=1, layers=(), wobs_max_dy=32):
    """--MAP_path (the most probable trajectory through the filter's particles, psvo_map_path) as a bool.  ValueError, naming the
    limit, for everything the kernel does not cover (runner.main calls this on the flags before it touches a device, SVO.__init__
    on the model it is given).  `layers`: the hidden layers of the per-particle MLPs, one each."""
    if not on:
        return False
    limit = "--MAP_path runs on the MAP-path kernel (psvo_map_path) behind the filter of SVO / AESMC / IWAE"
    if backward_simulation:
        raise ValueError("--MAP_path with --PSVO / --PSVOwR: %s; PSVO and PSVOwR already return backward-simulation "
                         "trajectories" % limit)
    if output_cov:
        raise ValueError("--MAP_path with output_cov: %s, which takes a state-independent transition scale; the "
                         "state-dependent-scale kernels have no MAP-path form" % limit)
    if Dy > wobs_max_dy or Dy < 1:
        raise ValueError("--MAP_path with Dy = %d: %s, which takes 1 <= Dy <= %d; no fallback path exists"
                         % (Dy, limit, wobs_max_dy))
    deep = [v for v in (_layer_list(s) for s in layers) if len(v) != 1]
    if deep:
        raise ValueError("--MAP_path with per-particle MLP layers %s: %s, which takes one hidden layer per MLP; two hidden "
                         "layers have no MAP-path form" % (deep, limit))
    return True


def _layer_list(spec):
    """a *_layers flag ("32" / "32,32") or a list of widths -> list of ints"""
    if isinstance(spec, str):
        return [int(v) for v in spec.split(",") if v.strip()]
    return [int(v) for v in spec]


class SVO:
    # the objective runs a backward simulation behind the filter (PSVO, PSVOwR): those kernels evaluate MLP_g for Dy <= 2 only
    uses_backward_simulation = False
    # ... and has a wide-observation form of it (PSVO: csrc/bsim_wobs.hip), taken when FLAGS.BSim_wide_obs asks for it
    has_wide_backward_simulation = False
    # the objective never resamples (IWAE): there is no decision for FLAGS.resample_ess to make
    never_resamples = False
    # observation widths of the plain filter kernels / of the wide-observation ("wobs") kernels (csrc/filter_wobs.hip)
    _PLAIN_DY, _WOBS_MAX_DY = 2, 32

    def __init__(self, model, FLAGS, name="log_ZSMC"):
        self.model = model
        # missing observations (FLAGS.missing_obs, not in the reference): a NaN observation is left out of the emission density
        self.missing_obs = self._route_missing_obs(model, FLAGS)
        # exogenous inputs (FLAGS.Di, not in the reference): f and q1 are driven by a given input v_t; 0 = off.  The input route
        # is the missing-observation filter with a bias row per step, so it owns every width and emission form as that one does
        self.Di = self._route_inputs(model, FLAGS)
        self.wide_obs = self._route_wide_obs(model, bool(getattr(FLAGS, "BSim_wide_obs", False)), self.missing_obs or self.Di > 0)

        # SSM distributions
        self.q0 = model.q0_dist
        self.q1 = model.q1_dist
        self.q2 = model.q2_dist
        self.f = model.f_dist
        self.g = model.g_dist

        self.n_particles = FLAGS.n_particles
        self.q_uses_true_X = FLAGS.q_uses_true_X

        # bidirectional RNN as full sequence observations encoder
        self.X0_use_separate_RNN = FLAGS.X0_use_separate_RNN
        self.use_stack_rnn = FLAGS.use_stack_rnn

        self.smooth_obs = True
        self.resample_particles = True
        # marginal particle smoother behind the filter at evaluation time (FLAGS.FFBS; psvo_ffbs_smooth)
        self.FFBS = bool(getattr(FLAGS, "FFBS", False))
        # backward-sampled trajectories behind the filter at evaluation time (FLAGS.FFBSi; psvo_ffbs_sample)
        self.FFBSi = bool(getattr(FLAGS, "FFBSi", False))

        # adaptive resampling (FLAGS.resample_ess, not in the reference): 0 = off, else the ESS threshold as a fraction of N
        self.resample_ess = self._route_resample_ess(model, FLAGS)

        # k-step predictive distribution of the evaluation's cloud (FLAGS.particle_forecast, not in the reference;
        # psvo_particle_forecast); FLAGS.forecast_noise off = every particle propagated without transition noise
        self.forecast = self._route_forecast(model, bool(getattr(FLAGS, "particle_forecast", False)))
        self.forecast_noise = bool(getattr(FLAGS, "forecast_noise", True))
        # ... on gappy data (FLAGS.particle_forecast_missing_obs; _route_missing_obs refused the combination without it):
        # psvo_particle_forecast_missing scores the observed entries of every target row
        self.forecast_missing = bool(self.missing_obs and self.forecast)
        # the most probable trajectory through the filter's particles at evaluation time (FLAGS.MAP_path, not in the reference;
        # psvo_map_path)
        self.MAP_path = self._route_map_path(model, bool(getattr(FLAGS, "MAP_path", False)))

        self.name = name
        self.generator = None        # torch.Generator on the compute device; None = global RNG

    @classmethod
    def _route_missing_obs(cls, model, FLAGS):
        """True when the filter of this objective runs on psvo_filter_forward_wobs_missing / psvo_filter_backward_wobs_missing
        (FLAGS.missing_obs, carried by the model; every 1 <= Dy <= 32, Dy <= 2 included, and all three emission forms).  What
        those kernels do not cover is refused here, up front."""
        trans = [t for t in (getattr(model, "q1_tran", None), getattr(model, "g_tran", None),
                             None if getattr(model, "use_bootstrap", True) else getattr(model, "f_tran", None)) if t is not None]
        if cls.uses_backward_simulation:    # (FLAGS.BSim_missing_obs: the backward simulation evaluates MLP_f and MLP_q1inv too)
            trans += [t for t in (getattr(model, "f_tran", None), getattr(model, "q1_inv_tran", None)) if t is not None]
        return check_missing_obs(bool(getattr(model, "missing_obs", False) or getattr(FLAGS, "missing_obs", False)),
                                 bsim_missing_obs=bool(getattr(FLAGS, "BSim_missing_obs", False)),
                                 cross_chain=cls.uses_backward_simulation and not cls.has_wide_backward_simulation,
                                 missing_rate=getattr(FLAGS, "missing_rate", 0.0),
                                 backward_simulation=cls.uses_backward_simulation,
                                 resample_ess=getattr(FLAGS, "resample_ess", 0.0),
                                 particle_forecast=bool(getattr(FLAGS, "particle_forecast", False)),
                                 output_cov=bool(getattr(model, "output_cov", False)), Dy=getattr(model, "Dy", cls._PLAIN_DY),
                                 layers=[t.Dhs for t in dict.fromkeys(trans)], wobs_max_dy=cls._WOBS_MAX_DY,
                                 resample_ess_missing_obs=bool(getattr(FLAGS, "resample_ess_missing_obs", False)),
                                 particle_forecast_missing_obs=bool(getattr(FLAGS, "particle_forecast_missing_obs", False)))

    @classmethod
    def _route_inputs(cls, model, FLAGS):
        """FLAGS.Di (carried by the model) as an int: 0, or the input width of a filter that runs on
        psvo_filter_forward_wobs_input / psvo_filter_backward_wobs_input.  What those kernels do not cover is refused here."""
        trans = [t for t in (getattr(model, "q1_tran", None), getattr(model, "g_tran", None),
                             None if getattr(model, "use_bootstrap", True) else getattr(model, "f_tran", None)) if t is not None]
        return check_inputs(getattr(model, "Di", 0) or getattr(FLAGS, "Di", 0), backward_simulation=cls.uses_backward_simulation,
                            resample_ess=getattr(FLAGS, "resample_ess", 0.0),
                            particle_forecast=bool(getattr(FLAGS, "particle_forecast", False)),
                            output_cov=bool(getattr(model, "output_cov", False)), Dy=getattr(model, "Dy", cls._PLAIN_DY),
                            layers=[t.Dhs for t in dict.fromkeys(trans)], wobs_max_dy=cls._WOBS_MAX_DY,
                            particle_forecast_inputs=bool(getattr(FLAGS, "particle_forecast_inputs", False)),
                            resample_ess_inputs=bool(getattr(FLAGS, "resample_ess_inputs", False)))

    @classmethod
    def _route_wide_obs(cls, model, bsim_wide_obs=False, missing_obs=False):
        """True when the filter of this objective runs on the wide-observation kernels (model.Dy > 2: psvo_filter_forward_wobs /
        psvo_filter_backward_wobs / psvo_mlp_wgrad_wobs) -- and, for PSVO under FLAGS.BSim_wide_obs (`bsim_wide_obs`), its
        backward simulation on psvo_bsim_forward_wobs / psvo_bsim_backward_wobs.  What those kernels do not cover is refused
        here, up front.  Without the flag PSVO stays refused: making it the default is a one-line change here."""
        Dy = getattr(model, "Dy", cls._PLAIN_DY)          # (a bare model object without widths has nothing to route)
        if getattr(model, "count_emission", False):
            # the count emission (psvo_desc.emission = 2) exists in the wide-observation kernels only
            if getattr(model, "poisson_emission", False):
                raise ValueError("--count_emission with --poisson_emission: one emission at a time -- count_emission is the "
                                 "Poisson likelihood of counts, poisson_emission the reference's unit-scale normal around "
                                 "the rate")
            if Dy <= cls._PLAIN_DY and not missing_obs:
                raise ValueError("--count_emission with Dy = %d: the count emission runs on the wide-observation kernels, which "
                                 "take 3 <= Dy <= %d; the plain kernels (Dy <= %d) have no count form"
                                 % (Dy, cls._WOBS_MAX_DY, cls._PLAIN_DY))
        if missing_obs and cls.uses_backward_simulation:
            # PSVO under FLAGS.BSim_missing_obs (_route_missing_obs has accepted it, or refused it, by now): the wide backward
            # simulation in its missing-observation form at every width, Dy <= 2 included; FLAGS.BSim_wide_obs is not needed
            return True
        if Dy <= cls._PLAIN_DY or missing_obs:      # (missing observations: _route_missing_obs has routed the filter)
            return False
        limit = "observations wider than Dy = %d run on the wide-observation filter kernels" % cls._PLAIN_DY
        if Dy > cls._WOBS_MAX_DY:
            raise ValueError("Dy = %d: %s, which take 3 <= Dy <= %d; no fallback path exists" % (Dy, limit, cls._WOBS_MAX_DY))
        if cls.uses_backward_simulation and not bsim_wide_obs:
            raise ValueError("Dy = %d with PSVO / PSVOwR: %s of the filter objectives (SVO, AESMC, IWAE); the backward-simulation "
                             "kernels evaluate the emission network for Dy <= %d only (PSVO: pass --BSim_wide_obs for the "
                             "wide-observation backward simulation)" % (Dy, limit, cls._PLAIN_DY))
        if cls.uses_backward_simulation and not cls.has_wide_backward_simulation:
            raise ValueError("Dy = %d with PSVOwR: --BSim_wide_obs covers PSVO only; the cross-chain resampling kernels of PSVOwR "
                             "evaluate the emission network for Dy <= %d only" % (Dy, cls._PLAIN_DY))
        if model.output_cov:
            raise ValueError("Dy = %d with output_cov: %s, which take state-independent scales; the state-dependent-scale "
                             "kernels take Dy <= %d" % (Dy, limit, cls._PLAIN_DY))
        trans = [model.q1_tran, model.g_tran] + ([] if model.use_bootstrap else [model.f_tran])
        if cls.uses_backward_simulation:
            trans += [t for t in (model.f_tran, getattr(model, "q1_inv_tran", None)) if t is not None]
        deep = [t.Dhs for t in dict.fromkeys(trans) if len(t.Dhs) != 1]
        if deep:
            raise ValueError("Dy = %d with per-particle MLP layers %s: %s, which take one hidden layer per MLP; two hidden "
                             "layers run for Dy <= %d only" % (Dy, deep, limit, cls._PLAIN_DY))
        return True

    @classmethod
    def _route_forecast(cls, model, on=True):
        """`on` when the particle forecast (psvo_particle_forecast) covers this model.  What the kernel does not cover is refused
        here, up front: it evaluates MLP_f and MLP_g with one hidden layer each, state-independent scales, Dy <= 32."""
        if not on:
            return False
        Dy = getattr(model, "Dy", cls._PLAIN_DY)
        limit = "--particle_forecast runs on the particle-forecast kernel (psvo_particle_forecast)"
        if Dy > cls._WOBS_MAX_DY:
            raise ValueError("Dy = %d: %s, which takes 1 <= Dy <= %d; no fallback path exists" % (Dy, limit, cls._WOBS_MAX_DY))
        if getattr(model, "output_cov", False):
            raise ValueError("output_cov: %s, which takes state-independent scales; the state-dependent-scale kernels have no "
                             "forecast form" % limit)
        trans = [t for t in (getattr(model, "f_tran", None), getattr(model, "g_tran", None)) if t is not None]
        deep = [t.Dhs for t in dict.fromkeys(trans) if len(t.Dhs) != 1]
        if deep:
            raise ValueError("per-particle MLP layers %s: %s, which takes one hidden layer per MLP (f and g)" % (deep, limit))
        return True

    @classmethod
    def _route_map_path(cls, model, on=True):
        """`on` when the MAP-path kernel (psvo_map_path) covers this model and objective.  What it does not cover is refused
        here, up front: it evaluates MLP_g with one hidden layer, a state-independent transition scale, Dy <= 32, and it reads
        the particle system of a filter objective."""
        trans = [t for t in (getattr(model, "q1_tran", None), getattr(model, "g_tran", None),
                             None if getattr(model, "use_bootstrap", True) else getattr(model, "f_tran", None)) if t is not None]
        return check_map_path(on, backward_simulation=cls.uses_backward_simulation,
                              output_cov=bool(getattr(model, "output_cov", False)), Dy=getattr(model, "Dy", cls._PLAIN_DY),
                              layers=[t.Dhs for t in dict.fromkeys(trans)], wobs_max_dy=cls._WOBS_MAX_DY)

    @classmethod
    def _route_resample_ess(cls, model, FLAGS):
        """FLAGS.resample_ess as a float: 0.0 (off: resampling at every step, or never for IWAE) or the threshold tau of
        psvo_filter_forward_adaptive, 0 < tau <= 1.  What the adaptive kernels do not cover is refused here, up front.  With
        FLAGS.resample_ess_wide_obs a model on the wide-observation route (_route_wide_obs has accepted it, or refused it, by
        now) takes psvo_filter_forward_wobs_adaptive; without the flag Dy > 2 stays refused: making it the default is a
        one-line change here."""
        trans = [t for t in (getattr(model, "q1_tran", None), getattr(model, "g_tran", None),
                             None if getattr(model, "use_bootstrap", True) else getattr(model, "f_tran", None)) if t is not None]
        return check_resample_ess(getattr(FLAGS, "resample_ess", 0.0), never_resamples=cls.never_resamples,
                                  backward_simulation=cls.uses_backward_simulation,
                                  output_cov=bool(getattr(model, "output_cov", False)), Dy=getattr(model, "Dy", cls._PLAIN_DY),
                                  plain_dy=cls._PLAIN_DY, wide_obs=bool(getattr(FLAGS, "resample_ess_wide_obs", False)),
                                  layers=[t.Dhs for t in dict.fromkeys(trans)], wobs_max_dy=cls._WOBS_MAX_DY,
                                  missing_obs=bool((getattr(model, "missing_obs", False) or getattr(FLAGS, "missing_obs", False))
                                                   and getattr(FLAGS, "resample_ess_missing_obs", False)),
                                  inputs=bool((getattr(model, "Di", 0) or getattr(FLAGS, "Di", 0))
                                              and getattr(FLAGS, "resample_ess_inputs", False)))

    # ------------------------------------------------------------------------------------------
    def get_log_ZSMC(self, obs, hidden, noise=None, inputs=None):
        """obs (batch, time, Dy), hidden (batch, time, Dx) -> (log_ZSMC scalar, {"Xs": (B,T,N,Dx)}).

        With FLAGS.Di > 0 `inputs` (batch, time, Di) is the exogenous input: x_{t+1} ~ f(. | x_t, v_t) with the proposal
        q1(. | x_t, v_t), the t = 0 terms evaluated with a zero input; the emission, q0, q2 and the encoders do not see it
        (psvo_filter_forward_wobs_input).  ValueError when it is missing or mis-shaped; log["filter"] keeps its keys.

        `noise` optionally injects the random draws in the HBM layout of include/psvo_hip.h:
        eps_f (T,B,Dx,N), u_f (T,B,N) or idx_f (T,B,N) int32; with FLAGS.FFBS also u_s (T,B,N) or idx_s (T,B,N) int32, the
        draws of the smoothed particles.  With FLAGS.resample_ess also rs_f (T,B) int32, teacher-forced resampling decisions.

        With FLAGS.resample_ess (adaptive resampling) log["ess"] (B,T) is the effective sample size of every step's weights,
        log["resampled"] (B,T) bool whether the sequence resampled there and log["filter"]["rs"] (T,B) int32 the same in the
        kernel's layout; log["Xs"] is the multinomial draw of every step whatever the decision (an equally weighted sample).

        With FLAGS.missing_obs a NaN in `obs` is an entry that was not observed: the filter leaves its term out of the emission
        density (psvo_filter_forward_wobs_missing), the proposal side reads 0 in its place, log_ZSMC bounds the log-density of
        the observed entries and log["missing"] (B,T,Dy) bool is the mask; log["filter"] keeps its keys.

        With FLAGS.FFBS and autograd not recording (evaluation, trajectory saving, prediction) the marginal smoother runs
        behind the filter: log["Xs"] then holds particles resampled by the SMOOTHED weights (the filtered ones move to
        log["Xs_filter"]), and log["X_smooth_mean"] (B,T,Dx), log["ess_smooth"] (B,T), log["logW_smooth"] (T,B,N) and
        log["smoother"] (the kernel's output dict in its own layout, with the drawn indices) are added.
        Under autograd nothing changes: the smoother has no gradient and is not launched.

        With FLAGS.FFBSi, under the same condition, N trajectories are backward-sampled from the filter's particle system
        (noise: u_p (T,B,N) or idx_p (T,B,N) int32): log["Xs"] then holds whole paths, log["Xs"][b, :, n, :] one draw from the
        joint smoothing distribution, as PSVO returns them; log["Xs_filter"] keeps the filtered cloud, log["path_logq"] (T,B,N)
        is the log-probability of every pick given the path's successor, log["path_distinct"] (B,T) the number of different
        particles the N paths pass through, log["paths"] the kernel's output dict.  With FLAGS.FFBS as well both kernels run
        and the smoother's per-step draws move to log["Xs_marginal"].

        With FLAGS.MAP_path, under the same condition, the most probable trajectory through the filter's particles is decoded
        (psvo_map_path; no random number is drawn): log["X_map"] (B,T,Dx) is the path, log["map_index"] (B,T) int32 the particle
        it takes at every step, log["map_score"] (B,) fp64 its joint log-density log p(x*, observed y) and log["map"] the
        kernel's output dict in its own layout (delta, lmax, bp, path, Xmap) with what the kernel was given beside it (g, sig_f,
        sig_g, fm0, fsig0, obs).  log["Xs"] and every other key are unchanged.
        """
        batch_size, time, _ = obs.shape
        self.Dx, self.batch_size, self.time = self.model.Dx, batch_size, time

        log = {}
        self._release()
        self._sigmas = self.model.sigmas()          # every scale vector of this evaluation, one fused launch
        if self.Di:
            filt = self.SMC(hidden, obs, noise=noise, inputs=self._check_input_rows(inputs, batch_size, time))
        elif inputs is not None:
            raise ValueError("get_log_ZSMC: inputs given to a model without an input channel (--Di = 0)")
        else:
            filt = self.SMC(hidden, obs, noise=noise)
        log_ZSMC = self.compute_log_ZSMC(filt["lse"])
        # (T, B, Dx, N) -> (batch_size, time, n_particles, Dx)
        log["Xs"] = filt["Xanc"].permute(1, 0, 3, 2)
        log["filter"] = filt
        if self.missing_obs:
            log["missing"] = self._missing              # (B, T, Dy) bool
        if filt.get("rs") is not None:
            log["ess"] = filt["ess"].transpose(0, 1)
            log["resampled"] = filt["rs"].transpose(0, 1) != 0
        if self.FFBS and not torch.is_grad_enabled():
            self._smooth(filt, log, noise or {})
        if self.FFBSi and not torch.is_grad_enabled():
            self._sample_paths(filt, log, noise or {})
        if self.MAP_path and not torch.is_grad_enabled():
            self._map_path(filt, log)
        self._release()
        return log_ZSMC, log

    def _check_input_rows(self, inputs, batch_size, time):
        """the exogenous input of an evaluation with FLAGS.Di > 0: (batch, time, Di), else ValueError"""
        if inputs is None:
            raise ValueError("--Di = %d: the model's transitions are driven by an input; pass inputs (batch, time, Di)" % self.Di)
        if tuple(inputs.shape) != (batch_size, time, self.Di):
            raise ValueError("--Di = %d: inputs must be (batch, time, Di) = %s, got %s"
                             % (self.Di, (batch_size, time, self.Di), tuple(inputs.shape)))
        return inputs

    def _input_share(self, v_TB, p):
        """hb[t,b,:] = v_TB[t,b,:] W1[Dx:] (time, B, H) of the MLP tuple `p` at the kernels' width: the input's share of its first
        layer"""
        return v_TB @ p[0][self.Dx:]

    def _state_rows(self, p):
        """the MLP tuple `p` with the state's rows W1[:Dx] of its first layer alone, as the input-driven kernels take it"""
        return None if p is None else (p[0][:self.Dx],) + tuple(p[1:])

    def _transition_scale(self, filt):
        """the constant scale the filter weighted the transition with (sigma_q1 when f shares q1's network, else sigma_f), or
        None under output_cov, where the filter left a scale per particle in filt["Fs"]"""
        if filt.get("Fs") is not None:
            return None
        return _c(self._sigma(self.q1 if self.model.use_bootstrap else self.f))

    def _smooth(self, filt, log, noise):
        """forward filtering, backward smoothing on the particle system `filt` (psvo_ffbs_smooth): the transition scale is the
        one the filter weighted with -- per particle under output_cov, else sigma_q1 when f shares q1's network, else sigma_f"""
        T, B, N = self.time, self.batch_size, self.n_particles
        sig_f = self._transition_scale(filt)
        u, idx_in = noise.get("u_s"), noise.get("idx_s")
        if u is None and idx_in is None:
            u = self._rand(T, B, N, device=filt["X"].device)
        sm = ops.ffbs_smooth(self._desc(), filt, sig_f=sig_f, u=u, idx_in=idx_in)
        log["Xs_filter"] = log["Xs"]
        log["Xs"] = sm["Xs"].permute(1, 0, 3, 2)                       # (T, B, Dx, N) -> (batch_size, time, n_particles, Dx)
        log["X_smooth_mean"] = sm["Xmean"].transpose(0, 1)
        log["ess_smooth"] = sm["ess"].transpose(0, 1)
        log["logW_smooth"] = sm["logWs"]
        log["smoother"] = sm

    def _sample_paths(self, filt, log, noise):
        """forward filtering, backward simulation on the particle system `filt` (psvo_ffbs_sample), with the scale of _smooth"""
        T, B, N = self.time, self.batch_size, self.n_particles
        u, idx_in = noise.get("u_p"), noise.get("idx_p")
        if u is None and idx_in is None:
            u = self._rand(T, B, N, device=filt["X"].device)
        paths = ops.ffbs_sample(self._desc(), filt, sig_f=self._transition_scale(filt), u=u, idx_in=idx_in)
        if "Xs_filter" in log:                                          # (FLAGS.FFBS too: log["Xs"] holds the smoother's draws)
            log["Xs_marginal"] = log["Xs"]
        else:
            log["Xs_filter"] = log["Xs"]
        log["Xs"] = paths["Xs"].permute(1, 0, 3, 2)                     # (T, B, Dx, N) -> (batch_size, time, n_particles, Dx)
        log["path_logq"] = paths["logq"]
        log["path_distinct"] = paths["distinct"].transpose(0, 1)
        log["paths"] = paths

    def _map_path(self, filt, log):
        """the MAP trajectory through the particle system `filt` (psvo_map_path): the transition scale of _smooth, the t = 0
        transition term the filter was given and the observations as the filter saw them (NaN = not observed)"""
        model = self.model
        desc = ops.make_desc(self.batch_size, self.time, self.n_particles, 1, model.Dx, model.Dy, self._kernel_width()[0],
                             bootstrap=model.use_bootstrap, emission=self._emission_code(), layers=1)
        g = _c(self._mlp_params(model.g_tran))
        given = {"sig_f": self._transition_scale(filt), "sig_g": _c(self._sigma(self.g)), "fm0": _c(self._fm0),
                 "fsig0": _c(self._fsig0), "obs": self._obs_TB}
        mp = ops.map_path(desc, filt, g, **given)
        log["X_map"] = mp["Xmap"].transpose(0, 1)                       # (T, B, Dx) -> (batch_size, time, Dx)
        log["map_index"] = mp["path"].transpose(0, 1)
        log["map_score"] = mp["lmax"].double().sum(0)
        log["map"] = dict(mp, g=g, **given)                             # (beside the outputs: what the kernel was given)

    def _release(self):
        """drop what one evaluation cached on the object (scale vectors, hoisted means, features, stream context).

        These tensors carry autograd history; kept until the next call they keep the previous evaluation's graph alive, and
        with it the parameters' gradient accumulators, which remember the stream they were created on.  The next evaluation
        would reuse them: issued under a hipGraph capture on another stream the engine then synchronises that old stream
        into the capture, where it is never joined back (hipStreamEndCapture crashes on ROCm 7.2 instead of reporting it)."""
        self._sigmas = self._m0 = self._sig0 = self._fm0 = self._fsig0 = self._obs_TB = self._ov = self._missing = None
        self.preprocessed_X0 = self.preprocessed_obs = None

    # hidden widths the kernels are instantiated for (template parameter H of csrc/*.hip)
    _KERNEL_H = (16, 32, 64)

    def _particle_mlps(self):
        """the MLPs evaluated per particle INSIDE the kernels (one or two hidden layers each; hip_params() raises otherwise)"""
        m = self.model
        trans = [m.q1_tran, m.g_tran]
        if not m.use_bootstrap:
            trans.append(m.f_tran)
        if getattr(m, "q1_inv_tran", None) is not None and hasattr(self, "q1_inv"):
            trans.append(m.q1_inv_tran)
        return trans

    def _kernel_width(self):
        """(H the kernels run at, whether any per-particle MLP layer is narrower than that, hidden layers per MLP).

        The kernels take ONE hidden width and ONE depth (1 or 2 hidden layers: psvo_desc.layers) for all per-particle MLPs
        of a launch.  Other widths the flags can reach (q1_layers=50, g_layers=16 beside q1_layers=32, "64,32", ...) run at
        the next instantiated width with zero-padded hidden units: a padded unit is relu(x . 0 + 0) = 0 times a zero row of
        the next kernel, so values and the gradients of the real entries are unchanged (the padding is
        `torch.nn.functional.pad` on the parameters: autograd slices the padded gradient back).  Wider than 64 has no
        kernel, and MLPs of different depth cannot be padded to a common one (an extra relu layer is not the identity):
        ValueError."""
        cached = self.__dict__.get("_kw")
        if cached is None:
            params = [t.hip_params() for t in self._particle_mlps()]
            depths = sorted(set(1 if len(p) == 4 else 2 for p in params))
            if len(depths) != 1:
                raise ValueError("per-particle MLPs (q1 / f / g / q1_inv) with different numbers of hidden layers %s: the "
                                 "kernels take one depth per launch; no fallback path exists"
                                 % [t.Dhs for t in self._particle_mlps()])
            layers = depths[0]
            widths = [w for p in params for w in ((p[0].shape[1],) if layers == 1 else (p[0].shape[1], p[4].shape[1]))]
            avail = self._KERNEL_H if layers == 1 else self._KERNEL_H[1:]      # (two layers: 32 and 64)
            fit = [H for H in avail if H >= max(widths)]
            if not fit:
                raise ValueError("per-particle MLP hidden width %d exceeds the widest kernel instantiation (%d); "
                                 "no fallback path exists" % (max(widths), self._KERNEL_H[-1]))
            cached = self._kw = (fit[0], any(w != fit[0] for w in widths), layers)
        return cached

    def _mlp_params(self, tran):
        """(W1, b1, W2, b2[, Wh, bh]) of a per-particle MLP at the kernels' hidden width"""
        p = tran.hip_params()
        H = self._kernel_width()[0]
        F = torch.nn.functional
        W1, b1, W2, b2 = p[:4]
        if len(p) == 4:
            pad = H - W1.shape[1]
            if pad:
                W1, b1, W2 = F.pad(W1, (0, pad)), F.pad(b1, (0, pad)), F.pad(W2, (0, 0, 0, pad))
            return W1, b1, W2, b2
        Wh, bh = p[4:]
        p1, p2 = H - W1.shape[1], H - Wh.shape[1]
        if p1 or p2:
            W1, b1 = F.pad(W1, (0, p1)), F.pad(b1, (0, p1))
            Wh, bh = F.pad(Wh, (0, p2, 0, p1)), F.pad(bh, (0, p2))
            W2 = F.pad(W2, (0, 0, 0, p2))
        return W1, b1, W2, b2, Wh, bh

    @staticmethod
    def _mlp_args(*mlps):
        """positional layout of the autograd nodes: four tensors per MLP (None for an absent one), then -- two hidden
        layers -- (Wh, bh) per MLP behind everything else.  Returns (first, extra)."""
        first, extra = [], []
        two = any(p is not None and len(p) == 6 for p in mlps)
        for p in mlps:
            first += list(p[:4]) if p is not None else [None] * 4
            if two:
                extra += list(p[4:6]) if p is not None else [None] * 2
        return first, extra

    def _desc(self, M=1):
        d = self._make_desc(M, self._kernel_width()[0])
        d._ov = getattr(self, "_ov", None)          # stream-overlap context of this evaluation (PSVO only)
        return d

    def _sigma(self, dist):
        sig = getattr(self, "_sigmas", None)
        if sig is None or id(dist) not in sig:      # (tf_poisson has no scale vector: constant ones)
            return dist.get_sigma()
        return sig[id(dist)]

    def _gbuf(self, tran):
        """slice of the flat gradient buffer a native backward may accumulate this MLP's gradient into (None when the
        kernels run on padded copies of the weights: the padded gradient then goes back through autograd)"""
        if tran is None or self._kernel_width()[1]:
            return None
        return tran.__dict__.get("_flat_grad")

    def _make_desc(self, M, H):
        return ops.make_desc(self.batch_size, self.time, self.n_particles, M, self.model.Dx, self.model.Dy, H,
                             resample=self.resample_particles, two_q=self.model.use_2_q,
                             bootstrap=self.model.use_bootstrap, emission=self._emission_code(),
                             layers=self._kernel_width()[2])

    def _emission_code(self):
        """psvo_desc.emission: 2 = count (Poisson) emission, 1 = tf_poisson (unit-scale normal around the rate), 0 = normal"""
        return 2 if getattr(self.model, "count_emission", False) else int(getattr(self.model, "poisson_emission", False))

    def _randn(self, *shape, device):
        return torch.randn(*shape, device=device, dtype=torch.float32, generator=self.generator)

    def _rand(self, *shape, device):
        return torch.rand(*shape, device=device, dtype=torch.float32, generator=self.generator)

    def _filter_draws(self, noise, dev):
        """the filter's randomness (eps (T,B,Dx,N), u (T,B,N) or None, idx_in): noise["eps_f"], ["u_f"] / ["idx_f"], or drawn, eps first"""
        T, B, N = self.time, self.batch_size, self.n_particles
        eps = noise.get("eps_f")
        if eps is None:
            eps = self._randn(T, B, self.Dx, N, device=dev)
        u, idx_in = noise.get("u_f"), noise.get("idx_f")
        if self.resample_particles and u is None and idx_in is None:
            u = self._rand(T, B, N, device=dev)
        return eps, u, idx_in

    def SMC(self, hidden, obs, q_cov=1.0, noise=None, inputs=None):
        """SVO.py:60-180.  Returns the kernel's output dict: X (pre-resampling, Xs_ta),
        Xanc (X_ancestors_ta), Fm, logW (log_Ws_ta), idx, lse -- all (T, B, ...)-major.
        inputs (B,T,Di): the exogenous input of a model with FLAGS.Di > 0."""
        if self.q_uses_true_X:
            # debug proposal around the true latents (SVO.py:73-77,127-131); run_flag forces it off
            # whenever use_2_q is set (runner.py:38-39)
            raise NotImplementedError("q_uses_true_X is a debugging aid outside the MI355X hot-path scope")
        model = self.model
        if model.output_cov:
            return self._SMC_cov(obs, noise)
        dev = obs.device
        noise = noise or {}

        feat_TB = None
        if self.missing_obs:
            # the observed mask, once.  The kernel alone gets the NaN-carrying rows; the proposal side (q0, q2, the encoders, the X0
            # feature) gets the observations with missing entries set to 0 -- the bound holds for any proposal
            observed = torch.isfinite(obs)
            self._missing = ~observed
            obs_TB = obs.masked_fill(self._missing, float("nan")).transpose(0, 1).contiguous().float()
            obs = obs.masked_fill(self._missing, 0.0)
            feat_TB = obs.transpose(0, 1).contiguous().float()
        preprocessed_X0, preprocessed_obs = self.preprocess_obs(obs)
        both = model.use_bootstrap and model.use_2_q
        if feat_TB is None:
            obs_TB = feat_TB = obs.transpose(0, 1).contiguous().float()
        self._obs_TB = obs_TB                                                  # (reused by the backward simulation)
        if not self.smooth_obs and both and obs.dtype == torch.float32 and not self.missing_obs:
            # obs[:, 0] itself is the X0 feature (SVO.py:322-324, no X0_transformer in this wiring): row 0 of the
            # (T, B, Dy) copy the kernels need anyway is the same data, contiguous -- no second copy launch
            preprocessed_X0 = obs_TB[0]
        self.preprocessed_X0, self.preprocessed_obs = preprocessed_X0, preprocessed_obs

        # ---- hoisted, particle-independent terms (B*T rows) ------------------------------------
        m0 = self.q0.mean(preprocessed_X0)                                    # (B, Dx)
        sig0 = self._sigma(self.q0)
        if both:
            fm0, fsig0 = m0, sig0                                             # f_0 is q0's own density
        else:
            fm0, fsig0 = self.f.mean(preprocessed_X0), self._sigma(self.f)    # SVO.py:91-92
        mu2 = sig_q2 = None
        if model.use_2_q:
            if preprocessed_obs is obs:
                # raw observations as features (AESMC / IWAE / PSVO): rows in (T, B) order give mu2 in the kernels' layout
                # directly -- no transposed copy of the output, none of its gradient
                mu2 = self.q2.mean(feat_TB)                                    # (T, B, Dx)
            else:
                mu2 = self.q2.mean(preprocessed_obs).transpose(0, 1).contiguous()
            sig_q2 = self._sigma(self.q2)

        eps, u, idx_in = self._filter_draws(noise, dev)

        q1p = self._mlp_params(model.q1_tran)
        fp = None if model.use_bootstrap else self._mlp_params(model.f_tran)
        hb = None
        if self.Di:
            # the input's share of the hidden pre-activation does not depend on the particle: hb[t,b,:] = v[b,t,:] W1[Dx:], one
            # small matrix product per network on the B T rows (torch differentiates it: d W1[Dx:] and d v come from d hb); the
            # kernels take W1[:Dx] and add hb to b1 step by step.  (W1 is padded to the kernel width: zeros in hb beyond it.)
            v_TB = inputs.transpose(0, 1).contiguous().float()
            hb = (self._input_share(v_TB, q1p), None if fp is None else self._input_share(v_TB, fp))
            q1p, fp = self._state_rows(q1p), self._state_rows(fp)
        first, extra = self._mlp_args(q1p, fp, self._mlp_params(model.g_tran))
        sig_f = None if model.use_bootstrap else self._sigma(self.f)
        self._m0, self._sig0, self._fm0, self._fsig0 = m0, sig0, fm0, fsig0
        desc = self._desc()
        gb = (self._gbuf(model.q1_tran), None if model.use_bootstrap else self._gbuf(model.f_tran), self._gbuf(model.g_tran))
        desc._gbufs = gb if (gb[0] is not None and gb[2] is not None and (model.use_bootstrap or gb[1] is not None)) else None
        # one opaque autograd node: psvo_filter_forward / psvo_filter_backward, or their wide-observation forms (Dy > 2)
        node = FilterFunction
        if self.wide_obs:
            node, desc._gbufs = FilterWobsFunction, None
        if self.missing_obs:        # psvo_filter_forward_wobs_missing / _backward_wobs_missing at every 1 <= Dy <= 32
            node, desc._gbufs = FilterWobsMissingFunction, None
            if self.uses_backward_simulation:       # (PSVO, FLAGS.BSim_missing_obs: Fm and logW carry gradients back)
                node = FilterWobsMissingBsimFunction
        if self.Di and self.resample_ess:
            # psvo_filter_forward_wobs_input_adaptive / _backward_wobs_input_adaptive (FLAGS.resample_ess_inputs): the input
            # route below with the decision per (step, sequence) made by the kernel
            desc._gbufs = None
            lse, Fm, logW, X, Xanc, idx, rs, ess = FilterWobsInputAdaptiveFunction.apply(
                desc, obs_TB, eps, u, idx_in, self.resample_ess, noise.get("rs_f"),
                *first, self._sigma(self.q1), sig_q2, sig_f, self._sigma(self.g), mu2, m0, sig0, fm0, fsig0, *extra, *hb)
            return {"lse": lse, "Fm": Fm, "logW": logW, "X": X, "Xanc": Xanc, "idx": idx, "eps": eps, "u": u,
                    "rs": rs, "ess": ess}
        if self.Di:                 # psvo_filter_forward_wobs_input / _backward_wobs_input: the same envelope, a bias row per step
            desc._gbufs = None
            lse, Fm, logW, X, Xanc, idx = FilterWobsInputFunction.apply(
                desc, obs_TB, eps, u, idx_in,
                *first, self._sigma(self.q1), sig_q2, sig_f, self._sigma(self.g), mu2, m0, sig0, fm0, fsig0, *extra, *hb)
            return {"lse": lse, "Fm": Fm, "logW": logW, "X": X, "Xanc": Xanc, "idx": idx, "eps": eps, "u": u}
        if self.resample_ess:
            # psvo_filter_forward_adaptive / psvo_filter_backward_adaptive: the decision per (step, sequence) is the kernel's
            # (wide observations, FLAGS.resample_ess_wide_obs: psvo_filter_forward_wobs_adaptive / _backward_wobs_adaptive)
            # (missing observations, FLAGS.resample_ess_missing_obs: psvo_filter_forward_wobs_missing_adaptive and its reverse)
            desc._gbufs = None
            node = FilterWobsAdaptiveFunction if self.wide_obs else FilterAdaptiveFunction
            if self.missing_obs:
                node = FilterWobsMissingAdaptiveFunction
            lse, Fm, logW, X, Xanc, idx, rs, ess = node.apply(
                desc, obs_TB, eps, u, idx_in, self.resample_ess, noise.get("rs_f"),
                *first, self._sigma(self.q1), sig_q2, sig_f, self._sigma(self.g), mu2, m0, sig0, fm0, fsig0, *extra)
            return {"lse": lse, "Fm": Fm, "logW": logW, "X": X, "Xanc": Xanc, "idx": idx, "eps": eps, "u": u,
                    "rs": rs, "ess": ess}
        lse, Fm, logW, X, Xanc, idx = node.apply(
            desc, obs_TB, eps, u, idx_in,
            *first, self._sigma(self.q1), sig_q2, sig_f, self._sigma(self.g), mu2, m0, sig0, fm0, fsig0, *extra)
        return {"lse": lse, "Fm": Fm, "logW": logW, "X": X, "Xanc": Xanc, "idx": idx, "eps": eps, "u": u}

    def _mlp_params_cov(self, tran):
        """(W1, b1, W_mu, b_mu, W_sigma, b_sigma) of a per-particle MLP with the covariance head, at the kernels' width"""
        W1, b1, Wm, bm, Ws, bs = tran.hip_params_cov()
        pad = self._kernel_width()[0] - W1.shape[1]
        if pad:
            F = torch.nn.functional
            W1, b1 = F.pad(W1, (0, pad)), F.pad(b1, (0, pad))
            Wm, Ws = F.pad(Wm, (0, 0, 0, pad)), F.pad(Ws, (0, 0, 0, pad))
        return W1, b1, Wm, bm, Ws, bs

    def _SMC_cov(self, obs, noise):
        """SVO.SMC with state-dependent diagonal scales (FLAGS.output_cov and FLAGS.diag_cov; src/transformation/MLP.py:40-46,
        58-61, src/distribution/mvn.py:66-71): psvo_filter_forward_cov / psvo_filter_backward_cov.  The hoisted distributions
        (q0, q2 and, outside the default wiring, f on the X0 feature) hand over mean AND scale per row; the per-particle
        MLPs carry their second head into the kernel."""
        model = self.model
        Dx, B = self.Dx, self.batch_size
        dev = obs.device
        noise = noise or {}
        if self._kernel_width()[2] != 1:
            raise ValueError("output_cov with two hidden layers per particle MLP: the state-dependent-scale kernels take one "
                             "hidden layer (psvo_filter_forward_cov); no fallback path exists")

        preprocessed_X0, preprocessed_obs = self.preprocess_obs(obs)
        both = model.use_bootstrap and model.use_2_q
        obs_TB = obs.transpose(0, 1).contiguous().float()
        self._obs_TB = obs_TB
        self.preprocessed_X0, self.preprocessed_obs = preprocessed_X0, preprocessed_obs

        m0, sig0 = self.q0.mean_and_sigma(preprocessed_X0, self._sigma(self.q0))            # (B, Dx) each
        if both:
            fm0, fsig0 = m0, sig0
        else:
            fm0, fsig0 = self.f.mean_and_sigma(preprocessed_X0, self._sigma(self.f))        # SVO.py:91-92
        mu2 = sig2 = None
        if model.use_2_q:
            if preprocessed_obs is obs:
                mu2, sig2 = self.q2.mean_and_sigma(obs_TB, self._sigma(self.q2))            # (T, B, Dx)
            else:
                mu2, sig2 = (v.transpose(0, 1).contiguous()
                             for v in self.q2.mean_and_sigma(preprocessed_obs, self._sigma(self.q2)))

        eps, u, idx_in = self._filter_draws(noise, dev)

        q1p = self._mlp_params_cov(model.q1_tran)
        fp = (None,) * 6 if model.use_bootstrap else self._mlp_params_cov(model.f_tran)
        gp = self._mlp_params_cov(model.g_tran)
        self._m0, self._sig0 = m0, sig0
        lse, Fm, Fs, logW, X, Xanc, idx = FilterCovFunction.apply(
            self._desc(), obs_TB, eps, u, idx_in, *q1p, *fp, *gp,
            self._sigma(self.q1), None if model.use_bootstrap else self._sigma(self.f), self._sigma(self.g),
            mu2, sig2, m0, sig0.expand(B, Dx), fm0, fsig0.expand(B, Dx))
        return {"lse": lse, "Fm": Fm, "Fs": Fs, "logW": logW, "X": X, "Xanc": Xanc, "idx": idx, "eps": eps, "u": u}

    def compute_log_ZSMC(self, lse):
        """SVO.py:302-311: mean_b sum_t logsumexp_n log_Ws[t, n, b]; `lse` (T, B) is the per-step
        logsumexp the filter kernel already produced."""
        if lse.requires_grad:
            return lse.sum(0).mean()
        return ops.elbo_filter(self._desc(), lse).mean()

    def preprocess_obs(self, obs):
        """SVO.py:313-331 -> (preprocessed_X0 (B, E0), preprocessed_obs (B, T, E))."""
        if not self.smooth_obs:
            preprocessed_obs = obs
            preprocessed_X0 = obs[:, 0]
        else:
            preprocessed_X0, preprocessed_obs = self.preprocess_obs_w_bRNN(obs)
        if not (self.model.use_bootstrap and self.model.use_2_q):
            preprocessed_X0 = self.model.X0_transformer(preprocessed_X0)
        return preprocessed_X0, preprocessed_obs

    def preprocess_obs_w_bRNN(self, obs, need_X0=True):
        """SVO.py:333-369 (use_stack_rnn): bi-LSTM encodings (B, T, 2Dh) and the X0 feature
        concat(out[:, -1], out[:, 0]) (B, 4Dh).  `need_X0=False` skips the separate X0 encoder
        when the caller discards its output (PSVO.BS_preprocess_obs, reference PSVO.py:80)."""
        y_smoother, X0_smoother = self.model.bRNN
        outputs = y_smoother(obs)
        preprocessed_obs = outputs
        if not need_X0:
            return None, preprocessed_obs
        if self.X0_use_separate_RNN:
            outputs = X0_smoother(obs)
        if self.use_stack_rnn:
            preprocessed_X0 = torch.cat([outputs[:, -1], outputs[:, 0]], dim=-1)            # (B, 4Dh), SVO.py:360-367
        else:
            Dh = outputs.shape[-1] // 2                                                     # outputs = [fw | bw]
            preprocessed_X0 = torch.cat([outputs[:, -1, :Dh], outputs[:, 0, Dh:]], dim=-1)  # (B, 2Dh)
        return preprocessed_X0, preprocessed_obs

    def n_step_prediction(self, n_steps, hidden, obs, inputs=None):
        """SVO.py:371-404: k-step predictions from the particle mean.  With FLAGS.Di > 0 `inputs` (B,T,Di) drives f: the state
        of origin t at horizon k meets v_{t+k}."""
        batch_size, time, _, _ = hidden.shape
        assert n_steps < time, "n_steps = {} >= time".format(n_steps)
        if getattr(self, "Di", 0):
            inputs = self._check_input_rows(inputs, batch_size, time)
        elif inputs is not None:
            raise ValueError("n_step_prediction: inputs given to a model without an input channel (--Di = 0)")
        x_BxTmkxDz = hidden.mean(dim=2)
        y_hat_N_BxTxDy = []
        for k in range(n_steps):
            y_hat_N_BxTxDy.append(self.g.mean(x_BxTmkxDz))
            if inputs is not None:
                x_BxTmkxDz = self.f.mean(x_BxTmkxDz[:, :-1], inputs=inputs[:, k:time - 1])
                continue
            x_BxTmkxDz = self.f.mean(x_BxTmkxDz[:, :-1])
        y_hat_N_BxTxDy.append(self.g.mean(x_BxTmkxDz))
        y_N_BxTxDy = [obs[:, k:, :] for k in range(n_steps + 1)]
        return y_hat_N_BxTxDy, y_N_BxTxDy

    def particle_forecast(self, n_steps, hidden, obs, noise=None, inputs=None):
        """k-step predictive distribution of the cloud `hidden` (B,T,N,Dx), as log["Xs"] is, for k = 0 .. n_steps from every
        origin t (psvo_particle_forecast; not in the reference).  Every particle is pushed through f -- q1's network and scale
        when f shares them -- with transition noise: noise["eps_p"] (n_steps,T,B,Dx,N) injects the standard normals, else they
        are drawn here; with FLAGS.forecast_noise off every particle is propagated noise-free.  The particles are equally
        weighted (log["Xs"] is a resampled cloud, or whole paths).  n_steps >= T is valid: forecasts past the end of the data
        are outputs too.  Evaluation only: no gradient, and under autograd the kernel is not launched (ValueError).

        Returns {"y_mean", "y_var": (B,T,n_steps+1,Dy), "x_mean": (B,T,n_steps+1,Dx), "lpd": (B,T,n_steps+1) the predictive
        log-density of obs[b, t+k] (0 where t + k >= T), "valid": (T,n_steps+1) bool, t + k < T, "forecast": the kernel's
        output dict in its own layout}.  `n_step_prediction` beside it stays the reference's metric.

        With FLAGS.missing_obs and FLAGS.particle_forecast_missing_obs (psvo_particle_forecast_missing) a non-finite entry of `obs`
        was not observed: "lpd" sums the observed entries of the target row and is 0 where it has none, "n_observed" (B,T,n_steps+1)
        int is the number of observed entries of obs[b, t+k] (0 outside the data) and "valid" narrows to (B,T,n_steps+1): the
        target lies inside the data and has at least one observed entry.

        With FLAGS.Di > 0 (FLAGS.particle_forecast_inputs; psvo_particle_forecast_input) `inputs` (B,Tv,Di), Tv >= T, drives f: the
        state of origin t at horizon k meets v_{t+k}, as in n_step_prediction; rows T .. Tv-1 are inputs planned past the data,
        and where t + k >= Tv the input is zero.  ValueError when it is missing or mis-shaped.  The returned keys are unchanged."""
        if torch.is_grad_enabled():
            raise ValueError("particle_forecast has no gradient: call it under torch.no_grad() (evaluation only)")
        self._route_forecast(self.model)
        B, T, N, Dx = hidden.shape
        K = int(n_steps)
        H, _, layers = self._kernel_width()
        if layers != 1:
            raise ValueError("particle_forecast with two hidden layers per particle MLP: psvo_particle_forecast takes one hidden "
                             "layer; no fallback path exists")
        model = self.model
        X = _c(hidden.permute(1, 0, 3, 2))                 # (T,B,Dx,N): no copy when `hidden` is a view of a kernel-layout tensor
        obs_TB = obs.transpose(0, 1).contiguous().float()
        missing = bool(getattr(self, "forecast_missing", False))
        if missing:                                        # (as SMC does: whatever is not finite was not observed)
            observed = torch.isfinite(obs_TB)              # (T,B,Dy)
            obs_TB = obs_TB.masked_fill(~observed, float("nan"))
        noise = noise or {}
        eps = noise.get("eps_p")
        if eps is None and self.forecast_noise and K > 0:
            eps = self._randn(K, T, B, Dx, N, device=X.device)
        f_tran, f_dist = (model.q1_tran, self.q1) if model.use_bootstrap else (model.f_tran, self.f)
        desc = ops.make_desc(B, T, N, 1, Dx, model.Dy, H, bootstrap=model.use_bootstrap, emission=self._emission_code(), layers=1)
        fp, extra = _c(self._mlp_params(f_tran)), {"missing": True} if missing else {}
        if getattr(self, "Di", 0):
            # the bias rows of SMC, over the Tv rows given (self.Dx: get_log_ZSMC sets it, and this call may come before any)
            if inputs is None:
                self._check_input_rows(inputs, B, T)
            if inputs.dim() != 3 or inputs.shape[0] != B or inputs.shape[1] < T or inputs.shape[2] != self.Di:
                raise ValueError("--Di = %d: particle_forecast inputs must be (batch, Tv, Di) = (%d, Tv >= %d, %d), got %s"
                                 % (self.Di, B, T, self.Di, tuple(inputs.shape)))
            self.Dx = Dx
            extra = {"hb_f": _c(self._input_share(inputs.transpose(0, 1).contiguous().float(), fp))}
            fp = self._state_rows(fp)
        elif inputs is not None:
            raise ValueError("particle_forecast: inputs given to a model without an input channel (--Di = 0)")
        fc = ops.particle_forecast(desc, K, fp, _c(self._mlp_params(model.g_tran)),
                                   _c(self._sigma(f_dist)), _c(self._sigma(self.g)), X, obs=obs_TB, eps=eps,
                                   **extra)      # (without the flags: the call as it always was)
        t = torch.arange(T, device=X.device)
        out = {"y_mean": fc["ymean"].permute(2, 1, 0, 3), "y_var": fc["yvar"].permute(2, 1, 0, 3),
               "x_mean": fc["xmean"].permute(2, 1, 0, 3), "lpd": fc["lpd"].permute(2, 1, 0),
               "valid": (t[:, None] + torch.arange(K + 1, device=X.device)[None, :]) < T, "forecast": fc}
        if missing:
            tk = t[:, None] + torch.arange(K + 1, device=X.device)[None, :]              # (T,K+1) target step
            cnt = observed.sum(-1).to(torch.int32)                                       # (T,B)
            n_obs = cnt[tk.clamp(max=T - 1)] * out["valid"][:, :, None].to(torch.int32)  # (T,K+1,B)
            out["n_observed"] = n_obs.permute(2, 0, 1)
            out["valid"] = out["n_observed"] > 0
        return out

    def get_nextX(self, X):
        """SVO.py:406-409 (quiver plots)."""
        return self.f.mean(X)


def _c(x):
    """detach + make contiguous fp32 (tensors or tuples of tensors); None passes through."""
    if x is None:
        return None
    if isinstance(x, (tuple, list)):
        return tuple(_c(v) for v in x)
    return x.detach().float().contiguous()
