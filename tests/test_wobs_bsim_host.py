"""Host side of PSVO on wide observations (no GPU): the flag, the routing decision of PSVO with and without it, and the refusals
raised up front."""
import pytest

from tests.test_wobs_host import _objective


def test_flag():
    from psvo_amd.flags import parse_flags
    F = parse_flags(["--PSVO", "--BSim_wide_obs", "--Dy=10", "--Dx=3", "--datadir=data/lorenz/", "--datadict=lorenzdatadict_py3"])
    assert (F.Dy, F.Dx, F.PSVO, F.BSim_wide_obs) == (10, 3, True, True)
    assert parse_flags(["--PSVO", "--Dy=10"]).BSim_wide_obs is False          # off by default
    assert parse_flags(["--PSVO", "--noBSim_wide_obs"]).BSim_wide_obs is False


@pytest.mark.parametrize("Dy,wide", [(1, False), (2, False), (3, True), (10, True), (17, True), (32, True)])
def test_routing_with_the_flag(Dy, wide):
    from psvo_amd.autograd import BsimWobsFunction, FilterWobsFunction      # (the nodes the wide route applies)
    assert BsimWobsFunction.__name__ == "BsimWobsFunction" and FilterWobsFunction.__name__ == "FilterWobsFunction"
    for wiring in (dict(use_bootstrap=True, use_2_q=True), dict(use_bootstrap=False, use_2_q=False)):
        smc = _objective("PSVO", Dy=Dy, BSim_wide_obs=True, **wiring)
        assert smc.wide_obs is wide and smc.uses_backward_simulation and smc.has_wide_backward_simulation


def test_without_the_flag_psvo_stays_refused():
    for obj in ("PSVO", "PSVOwR"):
        assert _objective(obj, Dy=2).wide_obs is False
        with pytest.raises(ValueError, match=r"Dy = 3 with PSVO / PSVOwR.*Dy <= 2") as e:
            _objective(obj, Dy=3)
        assert "--BSim_wide_obs" in str(e.value)                           # (the message names the way out)
        with pytest.raises(ValueError, match=r"Dy = 3 with PSVO / PSVOwR.*Dy <= 2"):
            _objective(obj, Dy=3, BSim_wide_obs=False)


def test_refusals_with_the_flag():
    wide = dict(BSim_wide_obs=True)
    with pytest.raises(ValueError, match=r"Dy = 3 with PSVOwR.*PSVO only"):
        _objective("PSVOwR", Dy=3, **wide)
    assert not _objective("PSVOwR", Dy=2, **wide).wide_obs
    with pytest.raises(ValueError, match=r"Dy = 3 with output_cov.*Dy <= 2"):
        _objective("PSVO", Dy=3, output_cov=True, diag_cov=True, **wide)
    with pytest.raises(ValueError, match=r"Dy = 3 with per-particle MLP layers \[\[32, 32\]\].*one hidden layer"):
        _objective("PSVO", Dy=3, g_layers="32,32", **wide)
    with pytest.raises(ValueError, match=r"Dy = 3 with per-particle MLP layers .*one hidden layer"):
        _objective("PSVO", Dy=3, q1_layers="32,32", **wide)                # (q1 and with it q1_inv)
    for extra in ({}, dict(output_cov=True, diag_cov=True), dict(g_layers="32,32")):
        with pytest.raises(ValueError, match=r"Dy = 33.*3 <= Dy <= 32"):     # the width is refused first
            _objective("PSVO", Dy=33, **wide, **extra)
    with pytest.raises(ValueError, match=r"Dy = 33"):
        _objective("PSVOwR", Dy=33, **wide)


def test_the_flag_changes_nothing_elsewhere():
    wide = dict(BSim_wide_obs=True)
    for obj in ("SVO", "AESMC", "IWAE"):
        for Dy in (2, 3, 10):
            assert _objective(obj, Dy=Dy, **wide).wide_obs is _objective(obj, Dy=Dy).wide_obs is (Dy > 2)
    assert _objective("PSVO", Dy=2, **wide).wide_obs is False
    assert _objective("PSVO", Dy=2, output_cov=True, diag_cov=True, **wide).wide_obs is False


def test_ffbs_flags_with_psvo_stay_refused():
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    for flag in ("--FFBS", "--FFBSi"):
        F = parse_flags(["--PSVO", "--BSim_wide_obs", flag, "--Dy=10", "--Dx=3"])
        with pytest.raises(ValueError, match=flag):
            runner.main(F)
