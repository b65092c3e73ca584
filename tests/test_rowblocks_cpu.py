"""pdb2reaction_amd/rowblocks.py without a GPU: the six NumPy statements are stated once and re-exported, the row dot is the diagonal of
the block Gram matrix bit for bit, and both solvers reproduce, through the host backend, the bits recorded in
tests/golden/solver_bits.npz (tools/make_solver_bits.py, run on the commit before the row-block algebra was drawn together)."""
import os
import sys

import numpy as np
import pytest

import modes_cases as MC
from pdb2reaction_amd import dimer as D
from pdb2reaction_amd import modes as M
from pdb2reaction_amd import rowblocks as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_statement_is_one_function_wherever_it_is_imported_from():
    for name in ("blk_gram", "blk_combine", "blk_scale"):
        assert getattr(M, name) is getattr(R, name), name
    for name in ("row_dot", "row_axpby", "row_absmax"):
        assert getattr(D, name) is getattr(R, name), name
    assert M.BLK_MAX is R.BLK_MAX and D.ROW_MAX == R.BLK_MAX == 64
    for mod in (M, D):
        assert issubclass(mod.HostBackend, R.HostRows) and issubclass(mod.DeviceBackend, R.DeviceRows)
    assert R.takes(lambda base, dirs, base_forces=None: None, "base_forces") and not R.takes(M.dense_hvp(np.eye(3)), "base_forces")
    assert R.takes(print, "base_forces") is False                            # (a callable without a signature is answered, not raised on)


@pytest.mark.parametrize("n", [3, 255, 256, 257, 771])
@pytest.mark.parametrize("k", [1, 3, 17, 64])
def test_the_row_dot_is_the_diagonal_of_the_gram_matrix(n, k):
    x, y = MC.kernel_data(k, n, 10 + k), MC.kernel_data(k, n, 100 + k)
    d = R.row_dot(x, y)
    assert d.shape == (k,) and MC.same_bits(d, np.diag(R.blk_gram(x, y)).copy())
    assert MC.same_bits(R.row_dot(x, x), np.diag(R.blk_gram(x, x)).copy())
    assert MC.same_bits(R.HostRows().dot(x, y), d) and MC.same_bits(R.HostRows().gram(x, y), R.blk_gram(x, y))


def test_the_host_projection_is_gram_and_combine_row_by_row():
    u, q = MC.kernel_data(3, 257, 5), MC.kernel_data(4, 257, 6)
    out = R.HostRows().project([q, None, q[:2]], u)
    assert MC.same_bits(out[1], u[1])
    for i, qi in ((0, q), (2, q[:2])):
        assert MC.same_bits(out[i:i + 1], R.blk_combine(qi, R.blk_gram(qi, u[i:i + 1]), u[i:i + 1], True))


@pytest.fixture(scope="module")
def bits():
    """(recorded, computed now): computed once and left unchanged."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_solver_bits as B

    with np.load(B.OUT) as z:
        recorded = {name: z[name] for name in z.files}
    return recorded, B.compute()


def test_both_solvers_reproduce_the_recorded_bits(bits):
    recorded, now = bits
    assert sorted(now) == sorted(recorded) and len(recorded) == 54
    for name in sorted(recorded):
        assert MC.same_bits(now[name], recorded[name]), name                 # dtype, shape and every bit: counts exactly, floats bit for bit


def test_the_record_holds_what_it_should(bits):
    recorded, _ = bits
    runs = {name.split("/")[0] for name in recorded}
    assert {r for r in runs if r.startswith("modes_")} >= {"modes_quadratic_k1", "modes_quadratic_k3", "modes_near_degenerate_k2_restarts",
                                                           "modes_quadratic_k2_frozen_tr"}
    assert {r for r in runs if r.startswith("dimer_")} >= {"dimer_a_k1", "dimer_a_k3", "dimer_a_k1_frozen", "dimer_a_k3_frozen_tr"}
    assert recorded["modes_near_degenerate_k2_restarts/counts"][3] >= 1      # restarts happened
    for run in ("dimer_a_k3", "dimer_a_k3_frozen_tr"):
        assert all(f"{run}/{i}/per_cycle" in recorded for i in range(3))
    c = recorded["dimer_a_k3/0/counts"]
    pc = recorded["dimer_a_k3/0/per_cycle"]
    assert pc.shape == (c[0], 4) and c[2] == 1 and pc[:, 2].sum() > 0        # converged, one record per cycle, rotations were made
    assert not recorded["dimer_a_k3_frozen_tr/1/x_mode"][1][[2, 7]].any()    # the mode's frozen rows are zero
