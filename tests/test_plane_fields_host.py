"""``simulation/plane_fields.gather`` with the flag settings of its four callers accepts and refuses what their private gathers
did: the plane moments demand a pressure always and ``w`` exactly with a 3-D velocity, the spectra and the correlations (host and
GPU classes alike) take a pressure only for channel ``p`` and ``w`` whenever the velocity has three components.  The expected
outcomes are written out here, not derived from the code under test."""
import numpy as np
import pytest

from fluidgym_amd.simulation.plane_fields import gather

V3, P3, T3 = np.zeros((2, 3, 2, 3, 4)), np.zeros((2, 1, 2, 3, 4)), np.zeros((2, 2, 2, 3, 4))
V2, P2, T2 = np.zeros((2, 2, 3, 4)), np.zeros((2, 1, 3, 4)), np.zeros((2, 1, 3, 4))
FLAT = np.zeros((2, 2, 24))                  # a multi-block domain's flat velocity
BAD_D = np.zeros((2, 2, 2, 3, 4))            # two components on a 3-D grid
P3_OTHER = np.zeros((2, 1, 2, 3, 5))
T3_OTHER_GRID, T3_OTHER_BATCH, T_4D = np.zeros((2, 1, 2, 3, 5)), np.zeros((1, 1, 2, 3, 4)), np.zeros((2, 1, 3, 4))

CALLERS = {"moments": dict(pressure_required=True, w_exact=True), "host_moments": dict(pressure_required=True, w_exact=True),
           "spectra": dict(), "timecorr": dict(pressure_required=False, w_exact=False)}
STRICT = ("moments", "host_moments")

# (case, channels, velocity, pressure, scalar, outcome of the moments, outcome of the spectra / correlations); an outcome is the
# (tensor, component) list's components, or the pattern of the ValueError.  scalar_batch: the moments' own gather let a scalar of
# another batch size through to np.stack (a ValueError about shapes) or to the kernel; the shared one refuses it for every caller.
CASES = [
    ("3d", ("u", "v", "w", "p"), V3, P3, None, [0, 1, 2, 0], [0, 1, 2, 0]),
    ("3d_scalar", ("u", "v", "w", "p", "T"), V3, P3, T3, [0, 1, 2, 0, 0], [0, 1, 2, 0, 0]),
    ("2d", ("u", "v", "p"), V2, P2, None, [0, 1, 0], [0, 1, 0]),
    ("2d_scalar", ("u", "v", "p", "T"), V2, P2, T2, [0, 1, 0, 0], [0, 1, 0, 0]),
    ("flat", ("u", "v", "p"), FLAT, P2, None, "multi-block", "multi-block"),
    ("components", ("u", "v", "p"), BAD_D, P3, None, "do not fit", "do not fit"),
    ("w_in_2d", ("u", "v", "w", "p"), V2, P2, None, "do not fit", "do not fit"),
    ("no_w_in_3d", ("u", "v", "p"), V3, P3, None, "do not fit", [0, 1, 0]),
    ("velocity_only", ("u", "v", "w"), V3, None, None, "pressure must be", [0, 1, 2]),
    ("one_component", ("v",), V3, None, None, "do not fit", [1]),
    ("pressure_missing", ("u", "v", "w", "p"), V3, None, None, "pressure must be", "pressure must be"),
    ("pressure_grid", ("u", "v", "w", "p"), V3, P3_OTHER, None, "pressure must be", "pressure must be"),
    ("pressure_unused_grid", ("u", "v", "w"), V3, P3_OTHER, None, "pressure must be", [0, 1, 2]),
    ("scalar_missing", ("u", "v", "w", "p", "T"), V3, P3, None, "channel T needs", "channel T needs"),
    ("scalar_grid", ("u", "v", "w", "p", "T"), V3, P3, T3_OTHER_GRID, "channel T needs", "channel T needs"),
    ("scalar_rank", ("u", "v", "w", "p", "T"), V3, P3, T_4D, "channel T needs", "channel T needs"),
    ("scalar_batch", ("u", "v", "w", "p", "T"), V3, P3, T3_OTHER_BATCH, "channel T needs", "channel T needs"),
    ("scalar_unused", ("u", "v", "w", "p"), V3, P3, T3_OTHER_GRID, [0, 1, 2, 0], [0, 1, 2, 0]),
]


@pytest.mark.parametrize("caller", sorted(CALLERS))
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gather_outcomes(caller, case):
    _, channels, velocity, pressure, scalar, strict, loose = case
    expected = strict if caller in STRICT else loose
    what = caller + ".update"
    if isinstance(expected, str):
        with pytest.raises(ValueError, match=expected) as err:
            gather(channels, velocity, pressure, scalar, what, **CALLERS[caller])
        assert str(err.value).startswith(what + ": ")
        return
    parts = gather(channels, velocity, pressure, scalar, what, **CALLERS[caller])
    assert [c for _, c in parts] == expected
    source = {"u": velocity, "v": velocity, "w": velocity, "p": pressure, "T": scalar}
    assert all(t is source[ch] for (t, _), ch in zip(parts, channels))
