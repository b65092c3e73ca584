"""The timings of profiles/pinned_graphs.txt.

    python tools/pinned_graphs_measure.py step ATOMS IMAGES [--pin-each] [--tree DIR] [--steps N] [--warmup W]
    python tools/pinned_graphs_measure.py pin ATOMS REFS [--steps N]

step: the step time of ONE batch (synthetic images of ATOMS atoms, energies and forces through the host entry, default precision mode):
median, mean and minimum over the steps after a warm-up, wall clock around the host entry (it ends in a stream synchronise; copies
included).  ``--pin-each`` pins every image of the batch at its own geometry first (``Engine.pin_graphs``).  ``--tree DIR`` imports the
package (and its built library) from another checkout -- the parent commit's.  One process per leg; the profile's numbers are legs run
alternately (parent, this build, this build pinned per image; c1 = 50 atoms x 8 images, c3 = 2000 x 16), three times over.

pin: the time of ``Engine.pin_graphs`` for REFS references of ATOMS atoms (wall clock around the call, which synchronises), the first
call and the median of the following ones, next to one unpinned evaluation of the same batch.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def engine_for(args, n_images):
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else ROOT)
    from pdb2reaction_amd import synth, weights as W
    from pdb2reaction_amd.engine import Engine

    z, imgs, _ = synth.make_images(args.atoms, n_images)
    eng = Engine(0)
    eng.load_weights(W.make_synthetic_weights(0))
    eng.set_system(z)
    eng.reserve_images(n_images)
    return eng, imgs.astype(np.float32)


def timed(fn, n):
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return np.array(ts)


def step(args):
    eng, p = engine_for(args, args.images)
    if args.pin_each:
        eng.pin_graphs(p)
    for _ in range(args.warmup):
        eng.energy_forces(p)
    ts = timed(lambda: eng.energy_forces(p), args.steps)
    print(f"{'parent' if args.tree else 'this build'}{' pinned per image' if args.pin_each else ''}: {args.atoms} atoms x {args.images} images, "
          f"{eng.graph_stats()[0]} edges: median {np.median(ts):.3f} ms  mean {ts.mean():.3f}  min {ts.min():.3f}  ({args.steps} steps)", flush=True)
    eng.close()


def pin(args):
    eng, p = engine_for(args, args.images)
    eng.energy_forces(p)                                                     # (the staging buffers and the degree buffers exist)
    first = timed(lambda: eng.pin_graphs(p), 1)[0]
    ts = timed(lambda: eng.pin_graphs(p), args.steps)
    counts, maxdeg = eng.pinned_graphs()
    eng.unpin_graph()
    ev = timed(lambda: eng.energy_forces(p), 3)
    print(f"pin_graphs: {args.images} references of {args.atoms} atoms, {sum(counts)} edges ({min(counts)} ... {max(counts)} per reference, largest in-degree "
          f"{maxdeg}): first call {first:.3f} ms, then median {np.median(ts):.3f} ms  min {ts.min():.3f}  ({args.steps} calls); "
          f"one unpinned evaluation of the batch: {np.median(ev):.3f} ms", flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["step", "pin"])
    ap.add_argument("atoms", nargs="?", type=int, default=2000)
    ap.add_argument("images", nargs="?", type=int, default=16)
    ap.add_argument("--pin-each", action="store_true")
    ap.add_argument("--tree")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    step(a) if a.mode == "step" else pin(a)
