"""Host side of the wide-observation path (no GPU): flag parsing, the routing decision of the filter objectives, the refusals
raised up front, and the committed data slices."""
import os

import numpy as np
import pytest

from tests import helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _objective(obj, **kw):
    from psvo_amd.model import SSM
    from psvo_amd.SMC.AESMC import AESMC
    from psvo_amd.SMC.IWAE import IWAE
    from psvo_amd.SMC.PSVO import PSVO
    from psvo_amd.SMC.PSVOwR import PSVOwR
    from psvo_amd.SMC.SVO import SVO
    cls = {"SVO": SVO, "PSVO": PSVO, "AESMC": AESMC, "IWAE": IWAE, "PSVOwR": PSVOwR}[obj]
    flags = dict(Dx=3, Dy=10, n_particles=8, n_particles_for_BSim_proposal=4, batch_size=2, time=5, q0_layers="16",
                 q1_layers="16", q2_layers="16", f_layers="16", g_layers="16", y_smoother_Dhs="8", X0_smoother_Dhs="8")
    flags.update(kw)
    FLAGS = Hh.make_flags(obj, **flags)
    return cls(SSM(FLAGS), FLAGS)


def test_flag():
    from psvo_amd.flags import parse_flags
    F = parse_flags(["--noPSVO", "--AESMC", "--Dy=10", "--Dx=3", "--datadir=data/lorenz/", "--datadict=lorenzdatadict_py3"])
    assert (F.Dy, F.Dx, F.AESMC, F.PSVO) == (10, 3, True, False)
    assert F.datadir + F.datadict == "data/lorenz/lorenzdatadict_py3"


@pytest.mark.parametrize("obj", ["SVO", "AESMC", "IWAE"])
@pytest.mark.parametrize("Dy,wide", [(1, False), (2, False), (3, True), (10, True), (17, True), (32, True)])
def test_routing(obj, Dy, wide):
    from psvo_amd.autograd import FilterWobsFunction          # (the node the wide route applies)
    assert FilterWobsFunction.__name__ == "FilterWobsFunction"
    for wiring in (dict(use_bootstrap=True, use_2_q=True), dict(use_bootstrap=False, use_2_q=False)):
        smc = _objective(obj, Dy=Dy, **wiring)
        assert smc.wide_obs is wide
        assert not smc.uses_backward_simulation


@pytest.mark.parametrize("obj", ["PSVO", "PSVOwR"])
def test_backward_simulation_objectives_stay_narrow(obj):
    assert _objective(obj, Dy=2).wide_obs is False and _objective(obj, Dy=2).uses_backward_simulation
    with pytest.raises(ValueError, match=r"Dy = 3 with PSVO / PSVOwR.*Dy <= 2"):
        _objective(obj, Dy=3)


def test_refusal_messages_name_the_limit():
    with pytest.raises(ValueError, match=r"Dy = 3 with output_cov.*Dy <= 2"):
        _objective("AESMC", Dy=3, output_cov=True, diag_cov=True)
    with pytest.raises(ValueError, match=r"Dy = 3 with per-particle MLP layers \[\[32, 32\]\].*one hidden layer"):
        _objective("SVO", Dy=3, g_layers="32,32")
    with pytest.raises(ValueError, match=r"Dy = 33.*3 <= Dy <= 32"):
        _objective("IWAE", Dy=33)
    with pytest.raises(ValueError, match=r"Dy = 33"):          # (the width is refused first, whatever else is asked for)
        _objective("PSVO", Dy=33)
    # the narrow path keeps what it had
    assert _objective("AESMC", Dy=2, output_cov=True, diag_cov=True).wide_obs is False
    assert _objective("AESMC", Dy=2, q1_layers="32,32", g_layers="32,32").wide_obs is False


def test_fixtures():
    d = np.load(os.path.join(GOLDEN, "lorenz_slice.npz"))
    shapes = {k: d[k].shape for k in d.files}
    assert shapes == {"Ytrain": (8, 100, 10), "Yvalid": (4, 100, 10), "State_train": (8, 100, 3), "State_valid": (4, 100, 3)}
    v = np.load(os.path.join(GOLDEN, "vind_slice.npz"))
    shapes = {k: v[k].shape for k in v.files}
    assert shapes == {"Ytrain": (8, 30, 20), "Yvalid": (4, 30, 20), "Xtrain": (8, 30, 2), "Xvalid": (4, 30, 2)}
    for f in (d, v):
        for k in f.files:
            assert f[k].dtype == np.float32 and np.isfinite(f[k]).all(), k
    for name in ("lorenz_slice.npz", "vind_slice.npz"):
        assert os.path.getsize(os.path.join(GOLDEN, name)) <= 100 * 1024
