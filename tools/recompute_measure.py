"""Recompute plans, measured (profiles/recompute.txt): (i) ms per evaluation and workspace bytes of one c5 image (20 000 atoms) and of the
c3 batch (16 images of 2000 atoms), recompute 2 against 0 in one process, with the results compared bit for bit; (ii) the largest
synthetic cluster one engine evaluates with recompute 1 under the default workspace cap, checked for finiteness and sum F ~ 0 only.

usage: python tools/recompute_measure.py [ab] [wall N1 N2 ...]"""
import os, sys, time
import numpy as np
sys.path.insert(0, ".")
from pdb2reaction_amd import synth, weights as W
from pdb2reaction_amd.engine import Engine, workspace_bytes

w = W.make_synthetic_weights(0)


def timed(eng, pos, reps):
    eng.energy_forces(pos)
    eng.energy_forces(pos)                       # the amortised workspace has reached its size by now or stays where it is
    t = time.perf_counter()
    for _ in range(reps):
        e, f = eng.energy_forces(pos)
    return (time.perf_counter() - t) / reps * 1e3, e, f


def ab(label, z, pos, reps):
    out = {}
    for mode in (0, 2):
        eng = Engine(0, recompute=mode); eng.load_weights(w); eng.set_system(z)
        ms, e, f = timed(eng, pos, reps)
        ne, _ = eng.graph_stats()
        out[mode] = (ms, e, f)
        print(f"{label} recompute={mode}: {ms:8.1f} ms / evaluation  workspace {eng.workspace_stats()[0] / 2**30:7.2f} GiB  edges {ne}  lanes {eng.last_lanes()} "
              f"partitions {eng.last_partitions()}  last_recompute {eng.last_recompute()}  "
              f"one-piece arithmetic {workspace_bytes(pos.shape[0] * pos.shape[1], ne, 0, mode, engine=eng) / 2**30:.2f} GiB", flush=True)
        eng.close()
    print(f"{label}: recompute / stored = {out[2][0] / out[0][0]:.3f}  bitwise equal: E {np.array_equal(out[0][1], out[2][1])}  F {np.array_equal(out[0][2], out[2][2])}", flush=True)


args = sys.argv[1:] or ["ab"]
if "ab" in args:
    g = np.load(os.path.join("tests", "golden", "c5_n20000.npz"))
    ab("c5 (1 x 20000 atoms)", g["z"], g["pos"][None].astype(np.float32), 3)
    z, imgs, _ = synth.make_images(2000, 16)
    ab("c3 (16 x 2000 atoms)", z, np.asarray(imgs, np.float32), 5)
if "wall" in args:
    for n in [int(a) for a in args[args.index("wall") + 1:]]:
        z, pos = synth.make_cluster(n)
        eng = Engine(0, recompute=1); eng.load_weights(w); eng.set_system(z)
        try:
            t = time.perf_counter(); e, f = eng.energy_forces(pos[None].astype(np.float32)); dt = time.perf_counter() - t
            ne, md = eng.graph_stats()
            print(f"N = {n}: edges {ne}  recompute {eng.last_recompute()}  partitions {eng.last_partitions()}  workspace {eng.workspace_stats()[0] / 2**30:.1f} GiB  "
                  f"E = {e[0]:.3f} eV  finite {bool(np.isfinite(e).all() and np.isfinite(f).all())}  |sum F| = {np.abs(f[0].astype(np.float64).sum(0)).max():.2e}  "
                  f"max|F| = {np.abs(f).max():.2f}  first evaluation (allocation included) {dt:.1f} s", flush=True)
        except Exception as exc:
            print(f"N = {n}: {type(exc).__name__}: {str(exc)[:400]}", flush=True)
        eng.close()
