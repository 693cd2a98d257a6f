"""Options3.stokes_warm_start without a GPU: the default, the mapping to (points, order) and the validation by name."""
import pytest


def test_default_is_off_and_true_is_the_2d_default():
    from pylamp_amd import pylamp3d as P3
    assert P3.Options3().stokes_warm_start is False
    assert P3.warm_start_setting(False) == (0, 0) and P3.warm_start_setting(None) == (0, 0)
    assert P3.warm_start_setting(True) == (3, 2) == P3.WARM_START_DEFAULT
    assert P3.warm_start_setting((2, 1)) == (2, 1) and P3.warm_start_setting([6, 3]) == (6, 3)
    assert P3.Options3(stokes_warm_start=(4, 3)).stokes_warm_start == (4, 3)


@pytest.mark.parametrize("value, word", [((1, 1), "points = 1 must be 2 .. 6"), ((7, 2), "points = 7 must be 2 .. 6"),
                                         ((3, 0), "order = 0 must be 1 .. 3"), ((5, 4), "order = 4 must be 1 .. 3"),
                                         ((2, 2), "order = 2 needs points >= 3, got points = 2"),
                                         ((3, 3), "order = 3 needs points >= 4, got points = 3"),
                                         (3, "a \\(points, order\\) pair"), ((3, 2, 1), "a \\(points, order\\) pair"),
                                         ((3.0, 2), "a \\(points, order\\) pair"), ("on", "a \\(points, order\\) pair")])
def test_bad_values_are_rejected_by_name(value, word):
    from pylamp_amd import pylamp3d as P3
    with pytest.raises(Exception, match="Options3.stokes_warm_start: .*" + word):
        P3.Options3(stokes_warm_start=value)


def test_the_library_declares_the_points_limit():
    """WARM_START_MAX_POINTS is X0_HIST + 1 of the header the library takes its weights from."""
    import os
    import re
    from pylamp_amd import pylamp3d as P3
    src = open(os.path.join(os.path.dirname(P3.__file__), "csrc", "pl_x0.h")).read()
    assert int(re.search(r"constexpr int X0_HIST = (\d+);", src).group(1)) + 1 == P3.WARM_START_MAX_POINTS
