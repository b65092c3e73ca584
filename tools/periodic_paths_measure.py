"""The figures of profiles/periodic_paths.txt.

    python tools/periodic_paths_measure.py [N]

One call of the bond-change entries at N atoms (default 2000) on one GPU: ``umx_bond_changes`` (open), ``umx_bond_changes_cell`` in a
cubic cell (M = 2, 2, 2: 125 candidates) and in the skew cell ``[[5,0,0],[4.5,2,0],[0,0,8]]`` scaled by 4 (M = 4, 4, 1: 243 candidates),
random atoms inside the box and a second geometry up to 0.4 off the first.  The whole call is timed on the host (three allocations, the
uploads, the kernel, the results back: two N x N float64 matrices and the N x N code), median of 7 after 2 warm-up calls, and again
without the distance matrices (``distances=False``: the kernel still computes them, only the code comes back), which brings the kernel
out from under the 64 MB of copies."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    sys.path.insert(0, ROOT)
    from pdb2reaction_amd.engine import Engine

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    rng = np.random.default_rng(0)
    skew = np.array([[5.0, 0, 0], [4.5, 2.0, 0], [0, 0, 8.0]]) * 4.0
    cells = {"open": (None, None), "cubic, 30 edge": (np.eye(3) * 30.0, True), "skew x 4": (skew, True)}
    eng = Engine(0)
    for name, (cell, pbc) in cells.items():
        r1 = rng.random((n, 3)) @ (np.eye(3) * 30.0 if cell is None else cell)
        r2 = r1 + rng.uniform(-0.4, 0.4, r1.shape)
        cov = np.full(n, 0.7)
        med = []
        for distances in (True, False):
            ts = []
            for _ in range(9):
                t0 = time.perf_counter()
                eng.bond_changes(r1, r2, cov, cell=cell, pbc=pbc, distances=distances)
                ts.append(time.perf_counter() - t0)
            ts = sorted(ts[2:])
            med.append((1e3 * ts[3], 1e3 * ts[0], 1e3 * ts[-1]))
        print(f"{name:16s} n={n}  call {med[0][0]:7.2f} ms (min {med[0][1]:.2f}, max {med[0][2]:.2f})   code only {med[1][0]:6.2f} ms (min {med[1][1]:.2f}, max {med[1][2]:.2f})",
              flush=True)
    eng.close()


if __name__ == "__main__":
    main()
