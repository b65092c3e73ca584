"""The figures of profiles/dimer.txt.

    python tools/dimer_measure.py fixture [--out FILE]                     the 12-atom saddle fixture of tests/dimer_cases.py
    python tools/dimer_measure.py scale [--atoms 2000] [--images 5] [--max-cycles 200] [--host] [--out FILE]

fixture: ``Engine.refine_saddles`` from the five noisy starts as one K = 5 call without a start direction, and each start alone with the
noisy lowest mode: cycles, images, wall time, distance to the fixture, curvature.
scale: a short synthetic string (``synth.make_images(atoms, images)``), its highest-energy image (HEI) and the central-difference
tangent there; ``Engine.refine_saddles`` from the HEI with K = 1 and K = 4 (the HEI and three copies with 0.01 A noise), defaults but
for ``--max-cycles``: cycles, images and wall time to convergence or to the cycle limit; with ``--host`` the K = 1 run again through the
host backend over ``Engine.hvp``; and the time of ONE batched evaluation of 64 displaced images under a pin, from which the cost of the
6N images of a finite-difference Hessian is EXTRAPOLATED (6N / 64 such batches; ``hessian`` measures it).
hessian: one ``uma_pysis.get_hessian`` (``hessian.fd_hessian``, 6N displaced images) of the same system, timed, for scale.
bench: ``bench.py --gpus 1 --steps S --warmup W`` in this tree and in the tree at ``--parent`` (a checkout of the parent commit, built),
alternating, ``--runs`` each, one fresh process per run: the headline value of every run, and each side's median and spread.

    python tools/dimer_measure.py hessian [--atoms 2000] [--out FILE]
    python tools/dimer_measure.py bench --parent DIR [--runs 3] [--steps 20] [--warmup 5] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def new_engine():
    from pdb2reaction_amd import weights as W
    from pdb2reaction_amd.engine import Engine

    eng = Engine(0)
    eng.load_weights(W.make_synthetic_weights(0))
    return eng


def line(tag, res, dt):
    return (f"{tag}: " + "; ".join(f"{r.reason} in {r.cycles} cycles, {r.images} images, C {r.curvature:.4f}, max|F| {r.max_force:.3e}" for r in res)
            + f"; {dt:.2f} s wall, {sum(r.images for r in res)} images in all")


def fixture(out):
    import dimer_cases as DC

    eng = new_engine()
    eng.set_system(DC.Z, max_neigh=DC.MAX_NEIGH)
    x0 = np.stack([DC.start(s) for s in range(DC.N_STARTS)])
    eng.refine_saddles(x0[0], max_cycles=1)                                  # warm-up: workspace, first launches
    t0 = time.perf_counter()
    res = eng.refine_saddles(x0)
    out(line("[fixture] K = 5, modes0 = None (lowest_modes' images included)", res, time.perf_counter() - t0))
    out("[fixture] max|x - X| " + ", ".join(f"{np.abs(r.x - DC.X).max():.4f}" for r in res) + " A; rotations per cycle "
        + ", ".join(str([h["rotations"] for h in r.history]) for r in res))
    mode = eng.lowest_modes(DC.X, np.ones(12), 1).modes[0]
    for s in range(DC.N_STARTS):
        t0 = time.perf_counter()
        r = eng.refine_saddles(x0[s], DC.noisy_mode(mode, s))
        out(line(f"[fixture] start {s} alone, noisy exact mode", r, time.perf_counter() - t0) + f"; max|x - X| {np.abs(r[0].x - DC.X).max():.4f} A")
    t0 = time.perf_counter()
    r = eng.refine_saddles(x0[:3], np.stack([DC.noisy_mode(mode, s) for s in range(3)]), thresh=(2e-3, 1e-3))
    out(line("[fixture] K = 3, thresholds (2e-3, 1e-3) eV/A", r, time.perf_counter() - t0))
    eng.close()


def scale(out, atoms, n_images, max_cycles, host):
    from pdb2reaction_amd import dimer as D
    from pdb2reaction_amd import synth

    eng = new_engine()
    z, imgs, _ = synth.make_images(atoms, n_images)
    x = imgs.astype(np.float64)
    eng.set_system(z)
    e, _ = eng.energy_forces(x, double_positions=True)
    hei = int(np.argmax(e[1:-1])) + 1
    tangent = x[hei + 1] - x[hei - 1]
    out(f"[scale] {atoms} atoms, string of {n_images} images: energies {np.array2string(e - e[0], precision=3)} eV, HEI = image {hei}")
    dirs = np.random.default_rng(3).standard_normal((32, atoms, 3))
    with eng.pinned(x[hei], double_positions=True):
        eng.hvp(x[hei], dirs[:2], step=1e-3)                                 # warm-up: workspace, graph
        t0 = time.perf_counter()
        eng.hvp(x[hei], dirs, step=1e-3)
        t64 = time.perf_counter() - t0
    out(f"[scale] one batch of 64 displaced images under the pin {t64 * 1e3:.1f} ms -> the 6N = {6 * atoms} images of ONE finite-difference Hessian "
        f"{6 * atoms / 64 * t64:.1f} s at that rate")
    noise = 0.01 * np.random.default_rng(4).standard_normal((3, atoms, 3))
    x4 = np.concatenate([x[hei][None], x[hei][None] + noise])
    for k in (1, 4):
        t0 = time.perf_counter()
        res = eng.refine_saddles(x4[:k], np.stack([tangent] * k), max_cycles=max_cycles)
        dt = time.perf_counter() - t0
        out(line(f"[scale] device backend, K = {k}, max_cycles = {max_cycles}", res, dt) + f"; {dt / max(1, sum(r.images for r in res)) * 1e3:.1f} ms per image")
    if host:
        t0 = time.perf_counter()
        res = D.refine_saddles(D.HostBackend(eng.hvp, pinner=eng), x4[:1], tangent[None], max_cycles=max_cycles)
        out(line(f"[scale] host backend over Engine.hvp, K = 1, max_cycles = {max_cycles}", res, time.perf_counter() - t0))
    eng.close()


def hessian(out, atoms, n_images):
    import importlib

    from pdb2reaction_amd import synth
    from pdb2reaction_amd._calculator_base import ANG2BOHR

    U = importlib.import_module("pdb2reaction_amd.uma_pysis")
    z, imgs, _ = synth.make_images(atoms, n_images)
    elem = [synth.SYMBOLS[int(a)] for a in z]
    calc = U.uma_pysis(model="synthetic", out_hess_torch=False)
    try:
        x = (imgs[n_images // 2].astype(np.float64) * ANG2BOHR).reshape(-1)
        calc.get_forces(elem, x)                                             # warm-up: engine, workspace
        t0 = time.perf_counter()
        h = calc.get_hessian(elem, x)["hessian"]
        dt = time.perf_counter() - t0
    finally:
        calc.close()
    out(f"[hessian] {atoms} atoms: ONE finite-difference Hessian (uma_pysis.get_hessian, {6 * atoms} displaced images), shape {tuple(np.shape(h))}: {dt:.1f} s wall")


def bench(out, parent, runs, steps, warmup):
    import json
    import subprocess

    sides = {"this": ROOT, "parent": os.path.abspath(parent)}
    vals = {k: [] for k in sides}
    for i in range(runs):
        for side, d in sides.items():
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=d, capture_output=True,
                               text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"bench.py failed in {d} (exit {p.returncode}): {p.stderr[-400:]}")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            vals[side].append(float(res["value"]))
            out(f"[bench] run {i + 1} {side}: {res['metric']} = {res['value']:.4f} {res['unit']}")
    for side, v in vals.items():
        out(f"[bench] {side}: median {np.median(v):.4f}, min {min(v):.4f}, max {max(v):.4f} ({steps} steps after {warmup}, {runs} runs)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=["fixture", "scale", "hessian", "bench"])
    ap.add_argument("--atoms", type=int, default=2000)
    ap.add_argument("--images", type=int, default=5)
    ap.add_argument("--max-cycles", type=int, default=200)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--parent", default=None, help="bench: a built checkout of the parent commit")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    a = ap.parse_args()

    def emit(text):
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")

    if a.part == "fixture":
        fixture(emit)
    elif a.part == "scale":
        scale(emit, a.atoms, a.images, a.max_cycles, a.host)
    elif a.part == "hessian":
        hessian(emit, a.atoms, a.images)
    else:
        if not a.parent:
            ap.error("bench needs --parent DIR")
        bench(emit, a.parent, a.runs, a.steps, a.warmup)
