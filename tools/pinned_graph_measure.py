"""The figures of profiles/pinned_graph.txt.

    python tools/pinned_graph_measure.py cpu                                     the float64 checker alone, no GPU
    python tools/pinned_graph_measure.py gpu ATOMS IMAGES [--pin] [--tree DIR] [--steps N] [--warmup W]

cpu: the two rank-swap cases of tests/pinned_cases.py (the 12-atom cluster and the triclinic cell, max_neigh = 4) through the float64
checker: what the graph held fixed and the graph rebuilt give at the moved geometry, the central difference of E across the swap
(h = 1e-3 A) on either graph against the analytic derivative on the fixed graph.  These are the bounds the GPU tests take from the
checker's own error.

gpu: the step time of ONE batch (synthetic images of ATOMS atoms, energies and forces through the host entry, default precision mode):
median, mean and minimum over the steps after a warm-up.  ``--pin`` pins the graph of the middle image first.  ``--tree DIR`` imports the
package (and its built library) from another checkout -- the parent commit's.  One process per leg; the profile's numbers are legs run
alternately (parent, this build, this build pinned; c1 = 50 atoms x 8 images, c3 = 2000 x 16), three times over.  Kernel by kernel, this
build's device code against the parent's: ``tools/double_positions_measure.py isa --tree DIR``.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cpu():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import pinned_cases as PC
    from pdb2reaction_amd import weights as W

    w = W.make_synthetic_weights(0)
    for name in ("cluster", "triclinic"):
        if name == "cluster":
            z, orc, x0, xm, xs, u, j = PC.cluster_swap(w)
        else:
            z, orc, _, _, x0, xm, xs, u, j = PC.triclinic_swap(w)
        g0, gm = PC.graph_of(orc, x0), PC.graph_of(orc, xm)
        (ef, ff), (er, fr) = PC.energy_forces_on(orc, z, xm, g0), PC.energy_forces_on(orc, z, xm, None)
        print(f"{name}: moved atom {j}, {len(g0[0])} edges, rebuilt graph equals the start graph: {PC.same_graph(g0, gm)}")
        print(f"  at the moved geometry: E fixed {ef:.6f} eV, rebuilt {er:.6f} eV (jump {er - ef:+.4f}), max|dF| between the two {np.abs(ff - fr).max():.4f} eV/A")
        h = PC.FD_H
        xp, xn = xs.copy(), xs.copy()
        xp[j] += h * u
        xn[j] -= h * u
        fd = (PC.energy_on(orc, z, xp, g0) - PC.energy_on(orc, z, xn, g0)) / (2 * h)
        analytic = -float(PC.energy_forces_on(orc, z, xs, g0)[1][j] @ u)
        fdr = (PC.energy_on(orc, z, xp) - PC.energy_on(orc, z, xn)) / (2 * h)
        print(f"  across the swap, h = {h} A: fixed graph fd {fd:.7f} analytic {analytic:.7f} (|diff| {abs(fd - analytic):.2e}) eV/A; rebuilt graph fd {fdr:.4f} eV/A")


def gpu(args):
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else ROOT)
    from pdb2reaction_amd import synth, weights as W
    from pdb2reaction_amd.engine import Engine

    z, imgs, _ = synth.make_images(args.atoms, args.images)
    p = imgs.astype(np.float32)
    eng = Engine(0)
    eng.load_weights(W.make_synthetic_weights(0))
    eng.set_system(z)
    eng.reserve_images(args.images)
    if args.pin:
        eng.pin_graph(p[args.images // 2])
    for _ in range(args.warmup):
        eng.energy_forces(p)
    ts = []
    for _ in range(args.steps):
        t = time.perf_counter()
        eng.energy_forces(p)
        ts.append((time.perf_counter() - t) * 1e3)
    ts = np.array(ts)
    print(f"{'parent' if args.tree else 'this build'}{' pinned' if args.pin else ''}: {args.atoms} atoms x {args.images} images, {eng.graph_stats()[0]} edges: "
          f"median {np.median(ts):.3f} ms  mean {ts.mean():.3f}  min {ts.min():.3f}  ({args.steps} steps)", flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["cpu", "gpu"])
    ap.add_argument("atoms", nargs="?", type=int, default=2000)
    ap.add_argument("images", nargs="?", type=int, default=16)
    ap.add_argument("--pin", action="store_true")
    ap.add_argument("--tree")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    cpu() if a.mode == "cpu" else gpu(a)
