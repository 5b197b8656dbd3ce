"""The solver's any-hit walk (csrc/anyhit.h) with one blocker on an edge of its decisions - t at 1e-5f and at max_dist, u == 0, a
vertex, the quad's diagonal, |a| at 1e-8f, the pair alone, a target that would block its own pair were it not skipped, a direction
component of -5e-9 and one of -0 beside zeros, and a node's box with tmin == tmax, tmin == max_dist and tmax == 1e-5f exactly
(tests/anyhit_edge_sets.py, proven on the CPU by tests/test_anyhit_edge_sets_host.py) - through the point-to-point form factors:
rows 0 and 1 of the matrix, bit for bit the oracle's, by the reference's walk (0) and by the certified walk (2, asked for by name
for these scenes of 3 to 40 primitives)."""
import functools

import numpy as np
import pytest

import anyhit_edge_sets as A
import ptmi
from oracle_binding import OracleScene

pytestmark = pytest.mark.gpu
F = np.float32
MODE = dict(use_monte_carlo=False, num_iterations=1)


@pytest.fixture(scope="module")
def R():
    r = ptmi.Renderer(0)
    yield r
    r.set_solver_walk(-1)
    r.close()


@functools.lru_cache(maxsize=None)
def oracle_rows(case):
    out = {}
    for member, arrs, blocked in A.cases()[case]:
        rows = OracleScene.from_arrays(*arrs).form_factor_rows([0, 1], **MODE)[0]
        rows.setflags(write=False)
        out[member] = rows
    return out


@pytest.mark.parametrize("walk", [0, 2])
@pytest.mark.parametrize("case", list(A.cases()))
def test_blocker_on_an_edge_turns_the_form_factor_as_in_the_oracle(R, case, walk):
    want = oracle_rows(case)
    try:
        for member, arrs, blocked in A.cases()[case]:
            R.load_scene_arrays(*arrs)
            R.set_solver_walk(walk, 1)
            st = R.run_radiosity_solver(**MODE)
            assert st.walk == walk, (case, member, st.walk)
            got = R.radiosity_solution()["form_factors"][:2]
            assert (got[0, 1] == 0) == blocked, (case, member, got[0, 1])
            assert (got.view(np.uint32) == want[member].view(np.uint32)).all(), (case, member, got[0, :3], want[member][0, :3])
    finally:
        R.set_solver_walk(-1)
