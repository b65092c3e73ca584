"""The figures of profiles/lowest_modes.txt.

    python tools/lowest_modes_measure.py cases [--out FILE]      the three 12-atom bases of tests/hvp_cases.py
    python tools/lowest_modes_measure.py scale [--atoms 50 2000] [--out FILE]

cases: for every base the dense finite-difference matrix B = W H_fd W (columns: ``Engine.hvp(base, e_k)`` under the solver's pin, step
1e-3 A, central), its asymmetry asym = ||(B - B^T) / 2||_2, the lowest eigenvalues of the projected symmetrised matrix and the gaps
between them; then ``Engine.lowest_modes`` with k = 2, block = 2, max_subspace = 8 -- once with tol = 0 for 60 iterations, whose smallest
and last residual norms are the residual FLOOR of the finite-difference operator, and once with tol = 4 asym: iterations, restarts,
images, eigenvalue error and subspace angle against the dense eigenpairs.
scale: ``Engine.lowest_modes`` (k = 2) on the synthetic clusters of ``synth.make_images``: the residual floor (block 8, tol = 0, 40
iterations), then block 4 and 8 with tol = four times that floor: iterations, images, wall time;
beside it the time of ONE batched evaluation of 64 displaced images under the same pin, from which the cost of the 6N images of
``hessian.fd_hessian`` follows (6N / 64 such batches).  Masses: the table of tests/modes_cases.py."""
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


def dense_b(eng, x, masses):
    """(H_fd (3N,3N) with column k = hvp(e_k), B = W H_fd W, asym)."""
    n = x.size
    with eng.pinned(x, double_positions=True):
        hv = eng.hvp(x, np.eye(n).reshape(n, -1, 3), step=1e-3)
    h = hv.reshape(n, n).T
    w = np.repeat(1.0 / np.sqrt(masses), 3)
    b = w[:, None] * h * w[None, :]
    return h, b, float(np.linalg.norm(0.5 * (b - b.T), 2))


def cases(out):
    import hvp_cases as HC
    import modes_cases as MC
    from pdb2reaction_amd import modes as M
    from pdb2reaction_amd import weights as W

    eng = new_engine()
    for name, c in HC.bases(W.make_synthetic_weights(0)).items():
        eng.set_system(c["z"], max_neigh=c["max_neigh"])
        eng.set_cell(c["cell"], c["pbc"])
        masses = MC.masses_of(c["z"])
        how = M.resolve_project("auto", c["cell"] is not None, False)
        h, b, asym = dense_b(eng, c["x"], masses)
        lam, vec, q, _ = MC.dense_reference(h, c["x"], masses, project=how)
        out(f"[cases] {name}: Z = {list(map(int, c['z']))}, project = {how} (rank {len(q)}), asym = {asym:.3e} eV/A^2/amu, ||B||_2 = {np.linalg.norm(b, 2):.3f}")
        out(f"[cases] {name}: lowest dense eigenvalues {np.array2string(lam[:5], precision=5)}; gaps l2-l1 = {lam[1] - lam[0]:.4f}, l3-l2 = {lam[2] - lam[1]:.4f}; "
            f"the yardstick bites for k = 2 when l3 - l2 > 4 (tol + 4 asym) = {32 * asym:.3e}, for k = 1 when l2 - l1 does")
        kw = dict(block=MC.BLOCK, max_subspace=MC.MAX_SUBSPACE, step=MC.STEP)
        floor = eng.lowest_modes(c["x"], masses, MC.K, tol=0.0, max_iter=60, **kw)
        hist = np.array(floor.history)
        out(f"[cases] {name}: tol = 0, 60 iterations: smallest max-residual {hist.min():.3e} (iteration {int(hist.argmin()) + 1}), median of the last 20 "
            f"{np.median(hist[-20:]):.3e}, last {hist[-1]:.3e}; floor / asym = {np.median(hist[-20:]) / asym:.2f}; restarts {floor.restarts}")
        t0 = time.perf_counter()
        res = eng.lowest_modes(c["x"], masses, MC.K, tol=4 * asym, max_iter=200, **kw)
        dt = time.perf_counter() - t0
        out(f"[cases] {name}: tol = 4 asym = {4 * asym:.3e}: converged {res.converged.tolist()} ({res.reason}) in {res.iterations} iterations, {res.restarts} restarts, "
            f"{res.products} products, {res.images} images, {dt:.2f} s; residuals {np.array2string(res.residuals, precision=3)}; |theta - lambda| = "
            f"{np.array2string(np.abs(res.eigenvalues - lam[:MC.K]), precision=3)}; sin(largest angle) = {MC.sin_largest_angle(res.modes_mw, vec[:MC.K]):.3e} "
            f"(Davis-Kahan bound {2 * 8 * asym / (lam[MC.K] - lam[MC.K - 1]):.3e}); freqs {np.array2string(res.freqs_cm, precision=1)} cm^-1")
    eng.close()


def scale(out, sizes):
    import modes_cases as MC
    from pdb2reaction_amd import synth

    eng = new_engine()
    for atoms in sizes:
        z, imgs, _ = synth.make_images(atoms, 1)
        x = imgs[0].astype(np.float64)
        masses = MC.masses_of(z)
        eng.set_system(z)
        eng.set_cell(None, None)
        dirs = np.random.default_rng(3).standard_normal((32, atoms, 3))
        with eng.pinned(x, double_positions=True):
            eng.hvp(x, dirs[:2], step=1e-3)                                 # warm-up: workspace, graph
            t0 = time.perf_counter()
            eng.hvp(x, dirs, step=1e-3)
            t64 = time.perf_counter() - t0
        out(f"[scale] {atoms} atoms: one batch of 64 displaced images under the pin {t64 * 1e3:.1f} ms -> the 6N = {6 * atoms} images of a finite-difference "
            f"Hessian {6 * atoms / 64 * t64:.1f} s at that rate")
        floor = eng.lowest_modes(x, masses, 2, block=8, tol=0.0, max_iter=40)
        hist = np.array(floor.history)
        fl = float(np.median(hist[-10:]))
        out(f"[scale] {atoms} atoms, k = 2, block = 8, tol = 0, 40 iterations: smallest max-residual {hist.min():.3e} (iteration {int(hist.argmin()) + 1}), median of "
            f"the last 10 {fl:.3e}, last {hist[-1]:.3e}; eigenvalues {np.array2string(floor.eigenvalues, precision=5)}; history "
            f"{np.array2string(hist, precision=2)}")
        for block in (4, 8):
            t0 = time.perf_counter()
            res = eng.lowest_modes(x, masses, 2, block=block, tol=4.0 * fl, max_iter=80)
            dt = time.perf_counter() - t0
            out(f"[scale] {atoms} atoms, k = 2, block = {block}, tol = 4 x floor = {4 * fl:.3e}: {res.reason} {res.converged.tolist()} in {res.iterations} iterations, "
                f"{res.restarts} restarts, {res.products} products, {res.images} images, {dt:.2f} s wall; eigenvalues {np.array2string(res.eigenvalues, precision=5)} "
                f"eV/A^2/amu, freqs {np.array2string(res.freqs_cm, precision=1)} cm^-1, residuals {np.array2string(res.residuals, precision=3)}")
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=["cases", "scale"])
    ap.add_argument("--atoms", type=int, nargs="*", default=[50, 2000])
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    a = ap.parse_args()

    def emit(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.part == "cases":
        cases(emit)
    else:
        scale(emit, a.atoms)
