"""The window barriers of the 8-lane kernel's two wavefronts with the first sweep specialised for the contact count
(csrc/tds_oct_windows.h: tds_oct_sweep_na, tds_oct_main_barriers_sweep_na; csrc/tds_oct.hip: main_sweep with NA as a template
constant).  Host side only: the walk the kernel's loops do, asked through tds_hip_oct_sweep_na_plan_host.

The specialised sweep takes the barrier at its window's top in the caller's loop and, for 3 NA > 8 (the long window), one more
inside, in position 7 — what the generic chain takes.  A workgroup whose wavefronts disagree about the number of barriers never
leaves the last one, so: for NA = 0 .. 17, no, one and two iterations, options oct_long_window and oct_sweep_na off and on, the
main wavefront's count equals the helper's and equals the generic walk's."""
import pytest

from tds_amd import hip_backend


@pytest.mark.parametrize("iters", [0, 1, 2])
@pytest.mark.parametrize("na", range(18))
def test_both_wavefronts_take_the_same_number_of_barriers_on_the_specialised_and_the_generic_path(na, iters, built):
    for lw in (0, 1):
        generic = hip_backend.oct_window_plan_host(na, iters, lw)
        assert generic["main_barriers"] == generic["help_barriers"]
        for opt in (0, 1):
            p = hip_backend.oct_sweep_na_plan_host(na, iters, lw, opt)
            assert p["main_barriers"] == p["help_barriers"] == generic["main_barriers"], (na, iters, lw, opt, p, generic)
            # specialised exactly where the first sweep holds every row of the iteration: NA 1, 2; NA 3, 4 as a long window
            want = bool(opt) and iters > 0 and (na in (1, 2) or (na in (3, 4) and bool(lw)))
            assert p["specialised"] == want, (na, iters, lw, opt, p)
