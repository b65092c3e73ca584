"""Cells and the brute-force minimum-image yardstick of the periodic-path tests (tests/test_periodic_paths_cpu.py,
tests/test_gpu_periodic_paths.py).  TEST INFRASTRUCTURE: nothing here uses ``pdb2reaction_amd.periodic``.

The yardstick takes the minimum over -6 .. +6 translations per periodic axis of the RAW difference -- no rounding step, no bound on the
range derived from the cell.  It is sufficient for atoms inside the cell: the rounded translation is then within one cell of the raw
one and the widest search any of these cells needs is 4 (the skew cell), so the nearest image lies within 5 translations of the raw
difference."""
import itertools

import numpy as np

BRUTE = 6
SHEARED = np.array([[7.0, 0.0, 0.0], [1.5, 6.5, 0.0], [1.0, -2.0, 7.5]])
CELLS = {
    # name: (cell, pbc)
    "ortho": (np.diag([9.0, 10.0, 11.0]), (True, True, True)),
    "sheared": (SHEARED, (True, True, True)),
    "skew": (np.array([[5.0, 0.0, 0.0], [4.5, 2.0, 0.0], [0.0, 0.0, 8.0]]), (True, True, True)),      # M = (4, 4, 1)
    "slab": (SHEARED, (True, True, False)),
    "wire": (SHEARED, (False, False, True)),
}


def translations(cell, pbc, m=BRUTE):
    """(n, 3) every integer combination within -m .. m of the periodic lattice vectors."""
    rng = [range(-m, m + 1) if f else (0,) for f in pbc]
    return np.array(list(itertools.product(*rng)), dtype=np.float64) @ np.asarray(cell, dtype=np.float64)


def brute_vectors(delta, cell, pbc):
    """The shortest of delta + t over :func:`translations`, for every row of delta (n, 3)."""
    cand = np.asarray(delta, dtype=np.float64)[:, None, :] + translations(cell, pbc)[None]
    return cand[np.arange(len(cand)), np.argmin((cand * cand).sum(-1), axis=1)]


def brute_distances(r, cell, pbc):
    """(n, n) minimum-image distances D_ij = min_t |r_j - r_i + t|, row block by row block."""
    r = np.asarray(r, dtype=np.float64)
    t = translations(cell, pbc)
    out = np.empty((len(r), len(r)))
    for i in range(len(r)):
        d = (r - r[i])[:, None, :] + t[None]
        out[i] = np.sqrt((d * d).sum(-1).min(axis=1))
    return out


def atoms_in_cell(n, cell, seed):
    """n points with fractional coordinates in [0, 1) (open axes too: the cell row only scales them)."""
    return np.random.default_rng(seed).random((n, 3)) @ np.asarray(cell, dtype=np.float64)


def classify(d1, d2, cov, bond_factor=1.20, margin_fraction=0.05, delta_fraction=0.05):
    """The masks of oracle/bond_changes_oracle.compare on GIVEN distance matrices: (code, T)."""
    n = len(cov)
    T = bond_factor * (cov[:, None] + cov[None, :])
    up = np.triu(np.ones((n, n), bool), 1)
    a1, a2 = (d1 <= T - margin_fraction * T) & up, (d2 <= T - margin_fraction * T) & up
    need = (np.abs(d2 - d1) >= delta_fraction * T) & up
    code = np.zeros((n, n), np.uint8)
    code[(~a1) & a2 & need] = 1
    code[a1 & (~a2) & need] = 2
    return code, T


def clear_of_thresholds(d1, d2, T, margin_fraction=0.05, delta_fraction=0.05, rel=1e-9):
    """The condition on the inputs: no pair within rel * T of the bonded threshold (either geometry) or of the change threshold."""
    up = np.triu(np.ones(T.shape, bool), 1)
    thr = T - margin_fraction * T
    gap = np.minimum(np.minimum(np.abs(d1 - thr), np.abs(d2 - thr)), np.abs(np.abs(d2 - d1) - delta_fraction * T))
    return bool((gap[up] > rel * T[up]).all())
