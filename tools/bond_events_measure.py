"""Measure the bond-change event route (``compare_path`` -> ``umx_bond_events``) against the matrix route (one ``compare_structures``
call per pair of neighbouring images -> ``umx_bond_changes[_cell]``) on one GPU -- the figures of profiles/bond_events.txt.

Legs: the 15 consecutive comparisons of a 16-image, 2000-atom string in open space and in a 20 A cubic cell; one pair of 20 000-atom
geometries; and, event route only (the matrix entry refuses it), the two consecutive pairs of three 50 000-atom geometries of
tests/test_gpu_bond_events.py.  Host wall time of the whole route (allocations, uploads, kernels, results back, the Python sets) and
the count / scan / fill kernel times of the event route from the HIP events inside the entry (``umx_debug_fetch
"bond_events:kernel_ms"``, read after every timed run): median (min .. max) of ``--repeat`` runs after ``--warmup`` runs; bytes over
PCIe from the sizes.

    python tools/bond_events_measure.py [--repeat 7] [--warmup 2] [--skip-large]
"""
import argparse
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pdb2reaction_amd import bond_changes as B          # noqa: E402
from pdb2reaction_amd import synth                       # noqa: E402
from pdb2reaction_amd.engine import Engine               # noqa: E402
from pdb2reaction_amd.uma_pysis import ANG2BOHR          # noqa: E402


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.median(v)), float(v.min()), float(v.max())


def timed(fn, warmup, repeat, after=None):
    """(last result, (median, min, max) of the wall time in ms, what ``after()`` returned behind every timed run)"""
    for _ in range(warmup):
        out = fn()
    ts, extra = [], []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        if after is not None:
            extra.append(after())
    return out, spread(ts), extra


def kernel_lines(ms):
    """count / scan / fill, each median (min .. max) over the timed runs"""
    ms = np.asarray(ms, dtype=np.float64)
    return "   ".join("%s %.3f ms (%.3f .. %.3f)" % ((name,) + spread(ms[:, k])) for k, name in enumerate(("count", "scan", "fill")))


def string_of(n, k, seed=7):
    z, imgs, _ = synth.make_images(n, k, seed=seed)
    atoms = [synth.SYMBOLS[int(a)] for a in z]
    return [types.SimpleNamespace(atoms=atoms, coords3d=x * ANG2BOHR) for x in imgs]


def leg(eng, label, geoms, kw, warmup, repeat):
    k, n = len(geoms), len(geoms[0].atoms)
    pairs = k - 1

    def matrix():
        return [B.compare_structures(geoms[a], geoms[a + 1], engine=eng, **kw) for a in range(pairs)]

    def events():
        return B.compare_path(geoms, "consecutive", engine=eng, **kw)

    old, (m_old, lo_old, hi_old), _ = timed(matrix, warmup, repeat)
    new, (m_new, lo_new, hi_new), ms = timed(events, warmup, repeat, lambda: eng.debug_fetch("bond_events:kernel_ms"))
    same = all(a.formed_covalent == b.formed_covalent and a.broken_covalent == b.broken_covalent for a, b in zip(old, new))
    n_ev = sum(len(r.formed_covalent) + len(r.broken_covalent) for r in new)
    up_old, down_old = pairs * (2 * n * 24 + n * 8), pairs * (2 * n * n * 8 + n * n)
    up_new, down_new = k * n * 24 + n * 8 + pairs * 8, (pairs + 1) * 8 + n_ev * 32
    print(f"{label}: n = {n}, {pairs} pair(s) of geometries, {n_ev} events, same sets: {same}")
    print(f"  matrix route  {pairs} x compare_structures   {m_old:10.2f} ms ({lo_old:.2f} .. {hi_old:.2f})   PCIe up {up_old / 1e6:9.3f} MB  down {down_old / 1e6:10.3f} MB")
    print(f"  event route   1 x compare_path          {m_new:10.2f} ms ({lo_new:.2f} .. {hi_new:.2f})   PCIe up {up_new / 1e6:9.3f} MB  down {down_new / 1e6:10.3f} MB")
    print(f"  event kernels: {kernel_lines(ms)};  matrix / event wall time = {m_old / m_new:.1f}")
    return same and m_new <= m_old + (hi_old - lo_old)


def lattice_leg(eng, warmup, repeat, n=50000):
    """Beyond the matrix entry's n * n <= 2^31: the case of tests/test_gpu_bond_events.py -- a 3 A cubic lattice of hydrogen radii (no
    bonds), eight planted pairs drawn to 0.6 A in the second geometry, two of them apart again in the third; ``Engine.bond_events`` on the
    consecutive pairs.  Event route only."""
    g = np.arange(37, dtype=np.float64) * 3.0
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[:n]
    cov = B.element_radii(["H"] * n, 1.0)[1]
    planted = [(0, 49999), (1, 2), (63, 64), (65, 129), (777, 30000), (12345, 40000), (25000, 25001), (49997, 49998)]
    back = [(63, 64), (12345, 40000)]
    geoms = np.stack([lattice, lattice, lattice])
    for i, j in planted:
        geoms[1, j] = geoms[1, i] + np.array([0.36, 0.48, 0.0])
        if (i, j) not in back:
            geoms[2, j] = geoms[1, j]
    (ev, per), (m, lo, hi), ms = timed(lambda: eng.bond_events(geoms, cov, per_pair=True), warmup, repeat, lambda: eng.debug_fetch("bond_events:kernel_ms"))
    ok = per.tolist() == [len(planted), len(back)]
    print(f"lattice, open space: n = {n}, 2 pairs of geometries ({n * (n - 1):.3g} pairs of atoms), {len(ev)} events, the planted ones: {ok}")
    print(f"  matrix route  refused (n * n exceeds 2^31 pairs)")
    print(f"  event route   1 x Engine.bond_events    {m:10.2f} ms ({lo:.2f} .. {hi:.2f})   PCIe up {(geoms.nbytes + cov.nbytes) / 1e6:9.3f} MB  down {(3 * 8 + len(ev) * 32) / 1e6:10.3f} MB")
    print(f"  event kernels: {kernel_lines(ms)}")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    eng = Engine(0)
    ok = True
    s = string_of(2000, 16)
    ok &= leg(eng, "string, open space", s, {}, a.warmup, a.repeat)
    ok &= leg(eng, "string, 20 A cubic cell", s, {"cell": np.eye(3) * 20.0 * ANG2BOHR, "pbc": True}, a.warmup, a.repeat)
    if not a.skip_large:
        ok &= leg(eng, "one pair, 20 000 atoms", string_of(20000, 2), {}, 1, 3)
        ok &= lattice_leg(eng, a.warmup, a.repeat)
    eng.close()
    print("event route not slower than the matrix route (margin: the matrix route's own spread) on every leg:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
