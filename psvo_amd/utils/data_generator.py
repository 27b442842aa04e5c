"""Simulated data sets for the runner's `generateTrainingData` switch (reference src/utils/data_generator.py:28-85).

generate_dataset(n_train, n_test, time, model="fhn" | "lorenz", Dy, f=None, g=None, x_0_in=None, lb, ub)
    -> hidden_train (n_train, time, Dx), hidden_test (n_test, time, Dx), obs_train (n_train, time, Dy), obs_test (n_test, time, Dy)

Contract kept from the reference (cited lines: its files)
  * the latent path is deterministic: one step = the ODE integrated by scipy's odeint over [0, dt] from the previous state
    (src/transformation/fhn.py:26-35, lorenz.py) -- FHN (a, b, c, I, dt) = (1, 0.95, 0.05, 1, 0.15), Lorenz
    (sigma, rho, beta, dt) = (10, 28, 8/3, 0.01);
  * the emission is y_t = G x_t + chol(cov) z with z ~ N(0, I_Dy) drawn from numpy's GLOBAL generator
    (src/distribution/mvn.py:10-19): G = [[1, 0]], cov = 0.01 I (FHN); G = [[1, 0, 0]], cov = 0.4 I (Lorenz);
  * order of the random draws (it fixes the data for a given np.random.seed): per sequence -- training sequences first -- the
    initial state x_0 ~ U(lb, ub)^Dx, then one emission draw per time step, t = 0 first;
  * `f` / `g` may be supplied: anything with a `.sample(x)` method (the reference's distribution objects) or a plain callable.
PoissonEmitter is such a `g`: counts y ~ Poisson(softplus(C x + d)) for the count emission (FLAGS.count_emission).

Exogenous inputs (FLAGS.Di = 1, FHN only; not in the reference, whose generator carries an unused `Di`): with `input_dim=1` the
injected current of step t -> t + 1 is I + v_t, v a per-sequence piecewise-constant pulse train (pulse_train) drawn from numpy's
GLOBAL generator right after the sequence's x_0, and generate_dataset returns v_train, v_test (n, time, 1) behind its four arrays.
"""
import numpy as np
from scipy.integrate import odeint

FHN_PARAMS = (1.0, 0.95, 0.05, 1.0, 0.15)              # a, b, c, I, dt
LORENZ_PARAMS = (10.0, 28.0, 8.0 / 3.0, 0.01)          # sigma, rho, beta, dt


def _advance(rhs, state, dt):
    """the state one step of length dt later (odeint over the two-point grid [0, dt], as the reference does)"""
    return odeint(rhs, state, np.array([0.0, dt]))[1]


def _fhn_step(X_prev, params, v=0.0):
    a, b, c, I, dt = params
    I = I + v                   # (an exogenous input adds to the injected current over the step)
    return _advance(lambda X, t: (X[0] - X[0] ** 3 / 3.0 - X[1] + I, a * (b * X[0] - c * X[1])), X_prev, dt)


def _lorenz_step(X_prev, params):
    sigma, rho, beta, dt = params
    return _advance(lambda X, t: (sigma * (X[1] - X[0]), X[0] * (rho - X[2]) - X[1], X[0] * X[1] - beta * X[2]), X_prev, dt)


class _Deterministic:
    """x -> step(x): the reference's dirac_delta around an ODE transformation"""

    def __init__(self, step, params):
        self._step, self._params = step, params

    def sample(self, x, v=None):
        return self._step(x, self._params) if v is None else self._step(x, self._params, float(v[0]))


class _LinearGaussian:
    """x -> G x + chol(cov) z: the reference's numpy mvn around a linear transformation"""

    def __init__(self, G, cov):
        self._G, self._chol = np.asarray(G, dtype=float), np.linalg.cholesky(cov)

    def sample(self, x):
        mean = self._G @ x
        return mean + self._chol @ np.random.randn(mean.shape[0])


class PoissonEmitter:
    """x -> Poisson(softplus(C x + d)): counts, drawn from numpy's GLOBAL generator like the Gaussian emission (not in the
    reference's generator; its numpy `poisson.sample` draws np.random.poisson the same way).  Usable as `g=` of
    generate_dataset; `rate(x)` is the mean."""

    def __init__(self, C, d):
        self._C, self._d = np.asarray(C, dtype=float), np.asarray(d, dtype=float)

    def rate(self, x):
        return np.logaddexp(0.0, self._C @ np.asarray(x, dtype=float) + self._d)

    def sample(self, x):
        return np.random.poisson(self.rate(x)).astype(float)


def count_loading(Dy, Dx=2):
    """(C (Dy, Dx), d (Dy,)) of the runner's generated count data: row k of C is (cos, sin)(2 pi k / Dy) -- the outputs look at
    the first two latent coordinates from Dy evenly spaced directions, further columns are zero -- and d = 1"""
    ang = 2.0 * np.pi * np.arange(Dy) / Dy
    C = np.zeros((Dy, Dx))
    C[:, 0], C[:, 1] = np.cos(ang), np.sin(ang)
    return C, np.ones(Dy)


_MODELS = {   # name: (Dx, transition step, its parameters, emission matrix, emission variance)
    "fhn": (2, _fhn_step, FHN_PARAMS, [[1.0, 0.0]], 0.01),
    "lorenz": (3, _lorenz_step, LORENZ_PARAMS, [[1.0, 0.0, 0.0]], 0.4),
}


def _sampler(obj):
    return obj.sample if hasattr(obj, "sample") else obj


def pulse_train(time, Di, low=5, high=15, amplitude=1.0, p_on=0.5):
    """(time, Di): per channel, consecutive segments of low .. high steps, each a pulse of height U(-amplitude, amplitude) with
    probability p_on, else 0.  Draws per segment, in order: its length, whether it is on, its height (always drawn)."""
    v = np.zeros((time, Di))
    for d in range(Di):
        t = 0
        while t < time:
            n = np.random.randint(low, high + 1)
            on = np.random.uniform() < p_on
            height = np.random.uniform(-amplitude, amplitude)
            v[t:t + n, d] = height if on else 0.0
            t += n
    return v


def generate_hidden_obs(time, Dx, Dy, x_0, f, g, v=None):
    """one sequence: X[0] = x_0, X[t] = f(X[t-1]); Y[t] = g(X[t]) (src/utils/data_generator.py:12-26); v (time, Di):
    X[t] = f(X[t-1], v[t-1])"""
    step, emit = _sampler(f), _sampler(g)
    X, Y = np.empty((time, Dx)), np.empty((time, Dy))
    state = np.asarray(x_0, dtype=float)
    for t in range(time):
        if t:
            state = step(state) if v is None else step(state, v[t - 1])
        X[t], Y[t] = state, emit(state)
    return X, Y


def knock_out(obs, rate):
    """a float copy of `obs` with every entry replaced by NaN independently with probability `rate` (FLAGS.missing_rate): one
    uniform per entry from numpy's GLOBAL generator, like everything else here, so FLAGS.seed reproduces the mask; rate 0 draws
    nothing and leaves no NaN"""
    out = np.array(obs, dtype=float)
    if rate > 0.0:
        out[np.random.uniform(size=out.shape) < rate] = np.nan
    return out


def generate_dataset(n_train, n_test, time, model="lorenz", Dy=1, Di=1, f=None, g=None, x_0_in=None, lb=-2.5, ub=2.5,
                     input_dim=0):
    """(`Di` is the reference's argument, unused there and here; `input_dim` > 0 switches the exogenous input on)"""
    if model not in _MODELS:
        raise ValueError("Unknown model {}".format(model))
    if input_dim and (model != "fhn" or input_dim != 1 or f is not None):
        raise ValueError("generated exogenous inputs: the FHN model with its own transition and one input channel (the injected "
                         "current, --Di=1) only; got model %r, Di = %r" % (model, input_dim))
    Dx, step, params, G, var = _MODELS[model]
    f = f if f is not None else _Deterministic(step, params)
    g = g if g is not None else _LinearGaussian(G, var * np.eye(Dy))
    if x_0_in is None and (lb is None or ub is None):
        raise AssertionError("must specify x_0 or (lb and ub)")

    hidden = np.zeros((n_train + n_test, time, Dx))
    obs = np.zeros((n_train + n_test, time, Dy))
    inputs = np.zeros((n_train + n_test, time, input_dim))
    for i in range(n_train + n_test):
        x_0 = np.random.uniform(low=lb, high=ub, size=Dx) if x_0_in is None else x_0_in
        if input_dim:
            inputs[i] = pulse_train(time, input_dim)
            hidden[i], obs[i] = generate_hidden_obs(time, Dx, Dy, x_0, f, g, v=inputs[i])
        else:
            hidden[i], obs[i] = generate_hidden_obs(time, Dx, Dy, x_0, f, g)
    if input_dim:
        return hidden[:n_train], hidden[n_train:], obs[:n_train], obs[n_train:], inputs[:n_train], inputs[n_train:]
    return hidden[:n_train], hidden[n_train:], obs[:n_train], obs[n_train:]
