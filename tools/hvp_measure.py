"""The figures of profiles/hvp.txt.

    python tools/hvp_measure.py cpu [--atoms N]                  the float64 checker alone, no GPU
    python tools/hvp_measure.py gpu [cost] [checker] [cycle] [--steps N] [--warmup W] [--cycles C]
    kernel by kernel, this build's device code against the parent's:  python tools/double_positions_measure.py isa --tree DIR

cpu: what rounding a displaced geometry to float32 positions does to a collective probe.  A synthetic cluster x (default 500 atoms) at the
origin offsets t = 0, 64 and 1024 A along (1, 1, 1) / sqrt(3), a random unit vector v over all 3N coordinates, step = 5e-3 Bohr (the
Lanczos recursion's dx).  Realised direction: d32 = float32(x + t + step v) - float32(x + t) against step v -- |d32 - step v| / step, and
the angle between the two.  Product: the forward difference (F(float32(x + t + step v)) - F(float32(x + t))) / step of the float64 checker
(oracle/, graph rebuilt, as the reference's probe does) against the same difference at the unrounded geometries -- |dHv| / |Hv|.  The engine
is not involved: this is what the float32 probe path inherits before any arithmetic of its own.

gpu cost: one ``Engine.hvp`` call with M = 1 and M = 8 directions, central and forward, at c1 (50 atoms) and c3 (2000 atoms), against the
SAME displaced images through ``energy_forces(double_positions=True)`` under ``pin_graph(base, double_positions=True)`` plus the NumPy
difference -- the two legs interleaved step by step after a warm-up; wall clock around the host entries (copies included), medians.
gpu checker: max |Hv_engine - Hv_checker| on the bases of tests/hvp_cases.py (step 1e-3 A, three random directions, the checker's central
difference on the base's fixed graph) and the rank-swap case pinned / unpinned.
gpu cycle: climbing cycles of ``gsm.GrowingStringDriver`` on the fully grown c3 string (2000 atoms x 16 images, device resident through
``parallel.EngineStringEvaluator``; thresholds forced so that the Lanczos phase runs every cycle) with ``climb_lanczos_hvp`` None, "forward"
and "central": time per cycle, recursions, images per recursion, the lowest Ritz values.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOHR = 0.529177210903


def cpu(atoms):
    sys.path.insert(0, ROOT)
    import torch
    from oracle.escn_md_oracle import Oracle
    from pdb2reaction_amd import synth, weights as W

    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    orc = Oracle(W.make_synthetic_weights(0))
    z, x = synth.make_cluster(atoms, seed=4)
    v = np.random.default_rng(7).standard_normal(x.shape)
    v /= np.linalg.norm(v)
    step, u = 5e-3 * BOHR, np.ones(3) / np.sqrt(3.0)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)                  # noqa: E731
    print(f"[hvp_measure cpu] {atoms} atoms, step = 5e-3 Bohr = {step:.4e} A, unit v over {v.size} coordinates: rms component {np.sqrt((v * v).mean()):.4f}, "
          f"rms displacement {step * np.sqrt((v * v).mean()):.3e} A", flush=True)
    for t in (0.0, 64.0, 1024.0):
        t0 = time.perf_counter()
        p0, p1 = x + t * u, x + t * u + step * v
        d32 = r32(p1) - r32(p0)
        err = np.linalg.norm(d32 - step * v) / step
        cos = float((d32 * v).sum() / np.linalg.norm(d32))
        f0, f1 = orc.energy_forces(z, p0)[1], orc.energy_forces(z, p1)[1]
        g0, g1 = orc.energy_forces(z, r32(p0))[1], orc.energy_forces(z, r32(p1))[1]
        hv, hv32 = -(f1 - f0) / step, -(g1 - g0) / step
        print(f"[hvp_measure cpu]   t = {t:6.0f} A: float32 ulp there {float(np.spacing(np.float32(max(t / np.sqrt(3.0), 8.0)))):.2e} A;  realised direction "
              f"|d32 - step v| / step = {err:.4f} (angle {np.degrees(np.arccos(min(cos, 1.0))):.3f} deg);  product |Hv32 - Hv| / |Hv| = "
              f"{np.linalg.norm(hv32 - hv) / np.linalg.norm(hv):.4f}  max|Hv32 - Hv| = {float(np.abs(hv32 - hv).max()):.3e} eV/A^2  (|Hv| = {np.linalg.norm(hv):.3f}, "
              f"v.Hv = {float((v * hv).sum()):.4f} / {float((v * hv32).sum()):.4f} eV/A^2)  ({time.perf_counter() - t0:.0f} s)", flush=True)


def new_engine():
    from pdb2reaction_amd import weights as W
    from pdb2reaction_amd.engine import Engine

    eng = Engine(0)
    eng.load_weights(W.make_synthetic_weights(0))
    return eng


def cost(args):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import hvp_cases as HC
    from pdb2reaction_amd import synth

    eng = new_engine()
    dp = {"double_positions": True}
    for label, atoms in (("c1", 50), ("c3", 2000)):
        z, imgs, _ = synth.make_images(atoms, 1)
        base = imgs[0].astype(np.float64)
        eng.set_system(z)
        for m in (1, 8):
            dirs = np.random.default_rng(3).standard_normal((m, atoms, 3))
            dirs /= np.linalg.norm(dirs.reshape(m, -1), axis=1)[:, None, None]
            for scheme in HC.SCHEMES:
                xs = HC.images(base, dirs, 1e-3, scheme)

                def entry():
                    return eng.hvp(base, dirs, step=1e-3, scheme=scheme)

                def composed():
                    with eng.pinned(base, **dp):
                        return HC.combine(eng.energy_forces(xs, **dp)[1], 1e-3, scheme)

                for _ in range(args.warmup):
                    a, b = entry(), composed()
                ts = {"hvp": [], "composed": []}
                for _ in range(args.steps):
                    for name, fn in (("hvp", entry), ("composed", composed)):
                        t0 = time.perf_counter()
                        fn()
                        ts[name].append((time.perf_counter() - t0) * 1e3)
                pair = [p - q for p, q in zip(ts["hvp"], ts["composed"])]
                print(f"[hvp_measure cost] {label} {atoms} atoms, M = {m}, {scheme}: {len(xs)} images, {eng.graph_stats()[0]} edges: hvp median "
                      f"{statistics.median(ts['hvp']):.3f} ms (min {min(ts['hvp']):.3f}), pin + energy_forces + NumPy median {statistics.median(ts['composed']):.3f} ms "
                      f"(min {min(ts['composed']):.3f}); step by step hvp - composed median {statistics.median(pair):+.3f} ms;  max|hv - composed| = "
                      f"{float(np.abs(a - b).max()):.1e}", flush=True)
    eng.close()


def checker(args):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import hvp_cases as HC
    import pinned_cases as PC
    from pdb2reaction_amd import weights as W

    w = W.make_synthetic_weights(0)
    eng = new_engine()
    for name, c in HC.bases(w).items():
        dirs = HC.directions(len(c["z"]))
        orc = PC.checker(w, cell=c["cell"], pbc=c["pbc"], max_neigh=c["max_neigh"])
        want = HC.checker_hv(orc, c["z"], c["x"], dirs, 1e-3, PC.graph_of(orc, c["x"]))
        eng.set_system(c["z"], max_neigh=c["max_neigh"])
        eng.set_cell(c["cell"], c["pbc"])
        for scheme in HC.SCHEMES:
            hv = eng.hvp(c["x"], dirs, step=1e-3, scheme=scheme)
            print(f"[hvp_measure checker] {name} ({eng.graph_stats()[0] // (6 if scheme == 'central' else 4)} edges), {scheme}: max|Hv_engine - Hv_checker(central)| = "
                  f"{float(np.abs(hv - want).max()):.3e} eV/A^2  (max|Hv| = {float(np.abs(want).max()):.3f})", flush=True)
    z, orc, x0, xm, xs, u, j = PC.cluster_swap(w)
    v = np.zeros((1, len(z), 3))
    v[0, j] = u
    eng.set_system(z, max_neigh=PC.MAX_NEIGH)
    eng.set_cell(None, None)
    for step in (1e-3, 2 * PC.INSIDE):
        want = HC.checker_hv(orc, z, xm, v, step, PC.graph_of(orc, xm))
        pinned, free = eng.hvp(xm, v, step=step), eng.hvp(xm, v, step=step, pin=False)
        print(f"[hvp_measure checker] rank swap at x_moved along the swapping atom's line, step {step} A: pinned max|Hv - checker| = "
              f"{float(np.abs(pinned - want).max()):.3e}, pin=False {float(np.abs(free - want).max()):.3e} eV/A^2  (bound {1e-3 / step:.3f})", flush=True)
    eng.close()


def cycle(args):
    sys.path.insert(0, ROOT)
    import torch
    from pdb2reaction_amd import synth
    from pdb2reaction_amd._calculator_base import ANG2BOHR
    from pdb2reaction_amd.gsm import GrowingStringDriver
    from pdb2reaction_amd.parallel import EngineStringEvaluator

    n, k, dev = 2000, 16, torch.device("cuda", 0)
    z, imgs, _ = synth.make_images(n, k)
    x0 = (imgs.astype(np.float64) * ANG2BOHR).reshape(k, -1)
    elem = [synth.SYMBOLS[int(v)] for v in z]
    for mode in (None, "forward", "central"):
        eng = new_engine()
        eng.set_system(z)
        ev = EngineStringEvaluator(eng, n, dev, check="deferred", max_images=k)
        gs = {"max_nodes": k - 2, "fix_first": False, "fix_last": False, "climb": True, "climb_rms": 1e9, "climb_lanczos": True, "climb_lanczos_rms": 1e9}
        if mode is not None:
            gs["climb_lanczos_hvp"] = mode
        drv = GrowingStringDriver(elem, x0[0], x0[-1], evaluate_device=ev, device=dev, images=x0, gs_kw=gs,
                                  stopt_kw={"max_cycles": args.cycles + args.warmup, "thresh": "gau_vtight", "max_step": 0.1, "print_every": 10 ** 9})
        marks, orig = [], drv._raw_eval

        def timed_eval(xq, _orig=orig, _marks=marks):
            if xq.shape[0] == k:
                torch.cuda.synchronize()
                _marks.append(time.perf_counter())
            return _orig(xq)

        drv._raw_eval = timed_eval
        out = drv.run()
        torch.cuda.synchronize()
        span = (marks[-1] - marks[args.warmup]) / max(len(marks) - 1 - args.warmup, 1)
        calls = max(drv.lanczos_calls, 1)
        print(f"[hvp_measure cycle] climb_lanczos_hvp={mode!r}: {span * 1e3:.1f} ms per cycle over {len(marks) - 1 - args.warmup} cycles; {drv.lanczos_calls} recursions, "
              f"{drv.lanczos_evals} images in them ({drv.lanczos_evals / calls:.2f} per recursion), warm kept {drv.lanczos_warm_calls} rejected {drv.lanczos_warm_rejected}; "
              f"(lowest Ritz value, overlap with the tangent, images): {[(round(w_, 5), round(o_, 3), n_) for w_, o_, n_, _ in drv.lanczos_log[:8]]}; "
              f"E(HEI) = {float(out.energies[out.hei_index]):.8f} Hartree", flush=True)
        ev.flush()
        eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["cpu", "gpu"])
    ap.add_argument("parts", nargs="*", default=["cost", "checker", "cycle"])
    ap.add_argument("--atoms", type=int, default=500)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cycles", type=int, default=5)
    a = ap.parse_args()
    if a.mode == "cpu":
        cpu(a.atoms)
    else:
        for part in a.parts:
            {"cost": cost, "checker": checker, "cycle": cycle}[part](a)
