"""The device-resident 3-D step with the warm start of the Stokes solve on (Options3.stokes_warm_start = True) against the
host-staged step with the same option: both commit the solution with the step's tstep, so they keep the same history and must
agree BITWISE as they do with the option off (tests/test_hip_step3_resident.py, whose runs and comparison are reused here).  The
sphere at 33^3 with the refill firing, four steps: one cold, one linear, two quadratic starts.  Measured on MI355X: 50, 43, 43 and
37 Stokes iterations, the same in both paths."""
import pytest

import test_hip_step3_resident as R

pytestmark = pytest.mark.gpu

NSTEP = 4


@pytest.fixture(scope="module")
def runs():
    nx, L, x, f = R._sphere(33, True, thin=[(5, 5, 5), (10, 20, 7), (20, 8, 30)])
    kw = dict(tracdens=8, tracdens_min=4, stokes_warm_start=True)
    keep = R.NSTEP
    R.NSTEP = NSTEP
    try:
        return R._run(nx, L, x, f, kw, False), R._run(nx, L, x, f, kw, True)
    finally:
        R.NSTEP = keep


def test_warm_resident_equals_warm_staged(runs):
    staged, resident = runs
    assert len(staged) == len(resident) == NSTEP
    R._assert_steps_equal(staged, resident, list(R.SCATTERED), list(R.SOLVED))
    for s, r in zip(staged, resident):
        assert list(s["rep"])[-1] == "stokes_start" and s["rep"]["stokes_start"] == r["rep"]["stokes_start"]
    print("starts:", [s["rep"]["stokes_start"] for s in staged], "iterations:", [s["rep"]["stokes"]["iterations"] for s in staged])
    assert [s["rep"]["stokes_start"] for s in staged] == ["cold"] + ["warm"] * (NSTEP - 1)


def test_history_stays_on_the_device(runs):
    """33^3: no copy of a node field (287 KB) or more in any resident step -- the history is committed device to device."""
    for it, r in enumerate(runs[1]):
        print("step %d: resident %s" % (it + 1, r["xfer"]))
        assert r["xfer"]["large"] == 0 and r["xfer"]["large_bytes"] == 0
