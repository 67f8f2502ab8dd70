"""The window barriers of the 8-lane kernel's two-wavefront builds, asked on the CPU (csrc/tds_oct_windows.h through
tds_hip_oct_window_plan_host).  No GPU.

The main wavefront and the helper of a workgroup walk the row windows of a step's contact sweep in loops of their own and
meet at one barrier per window; the loops are written against one rule, and this test walks that rule on the host for every
contact count a wavefront can have (NA = 0 .. 17: 0 .. 51 constraint rows, up to seven windows) x 0 .. 3 Gauss-Seidel iterations
x option oct_long_window off / on.  Two wavefronts that disagree about the number of barriers never leave the last one."""
import pytest

from tds_amd import hip_backend

NAS = range(18)
ITERS = range(4)


def parent_formula(na, iters):
    """one barrier per window of eight rows and iteration, as the loops were before the long window"""
    return iters * ((3 * na + 7) // 8) if na > 0 else 0


@pytest.mark.parametrize("iters", ITERS)
def test_both_wavefronts_take_the_same_number_of_window_barriers(iters, built):
    for na in NAS:
        off = hip_backend.oct_window_plan_host(na, iters, 0)
        on = hip_backend.oct_window_plan_host(na, iters, 1)
        for p in (off, on):
            assert p["main_barriers"] == p["help_barriers"], (na, iters, p)
        assert on["main_barriers"] == off["main_barriers"] == parent_formula(na, iters), (na, iters, on, off)


def test_the_long_window_is_taken_exactly_for_nine_to_twelve_rows(built):
    for iters in ITERS:
        for na in NAS:
            assert not hip_backend.oct_window_plan_host(na, iters, 0)["long_window"]
            assert hip_backend.oct_window_plan_host(na, iters, 1)["long_window"] == (na in (3, 4) and iters >= 1), (na, iters)


def test_bad_arguments_are_refused(built):
    with pytest.raises(hip_backend.TdsHipError):
        hip_backend.oct_window_plan_host(-1, 1, 1)
    with pytest.raises(hip_backend.TdsHipError):
        hip_backend.oct_window_plan_host(3, -1, 1)
