"""The recorded bits of both Hessian-free solvers on analytic operators: tests/golden/solver_bits.npz.

    python tools/make_solver_bits.py            write the file (run on the commit whose behaviour is to be pinned)

``lowest_modes`` runs through ``modes.HostBackend`` over ``modes.dense_hvp`` of the 30-dimensional matrices of tests/modes_cases.py /
tests/hvp_cases.py; ``refine_saddles`` through ``dimer.HostBackend`` over the analytic saddle surfaces of tests/dimer_cases.py, K = 1 and
K = 3, with and without frozen atoms.  :func:`compute` returns every array the file holds; tests/test_rowblocks_cpu.py calls it and
compares bit for bit, so any change of an operation order in the NumPy statements or of a solver's use of them shows."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "tests", "golden", "solver_bits.npz")
PER_CYCLE = ("energy", "curvature", "rotations", "step_max")    # the columns of a candidate's per_cycle array (rotations: a small integer, exact)


def modes_runs():
    import hvp_cases as HC
    import modes_cases as MC

    quad, near = HC.quadratic()[0], MC.near_degenerate()
    heavy = 1.0 + 0.5 * np.arange(10)
    return {"modes_quadratic_k1": (quad, 1, {}),
            "modes_quadratic_k3": (quad, 3, {}),
            "modes_near_degenerate_k2_restarts": (near, 2, dict(block=2, max_subspace=8, max_iter=400)),
            "modes_quadratic_k2_forward": (quad, 2, dict(scheme="forward")),
            "modes_quadratic_k2_frozen_tr": (quad, 2, dict(frozen=[2, 7], project="tr", masses=heavy)),
            "modes_near_degenerate_k1_t": (near, 1, dict(project="t", masses=heavy))}


def dimer_runs():
    import dimer_cases as DC

    out = {}
    for name, (ef, saddle, _), noise in (("a", DC.surface_a(0.5), 0.18), ("b", DC.surface_b(), 0.1)):
        rng = np.random.default_rng(9)
        x0 = saddle[None] + noise * rng.standard_normal((3,) + saddle.shape)
        n0 = rng.standard_normal(x0.shape)
        out[f"dimer_{name}_k1"] = (ef, x0[0], n0[0], dict(project="none"))
        if name == "a":
            out["dimer_a_k3"] = (ef, x0, n0, dict(project="none"))
            out["dimer_a_k1_frozen"] = (ef, x0[1], n0[1], dict(project="none", frozen=[2, 7], max_cycles=8))
            out["dimer_a_k3_frozen_tr"] = (ef, x0, n0, dict(project="tr", frozen=[2, 7], max_cycles=6))
        else:
            out["dimer_b_k3_tr"] = (ef, x0, n0, dict(project="tr", max_cycles=6))
    return out


def compute() -> dict:
    """name -> array, every solver run above.  modes: eigenvalues, history, counts = (iterations, products, images, restarts); dimer, per
    candidate: per_cycle (cycles, 4) in the order of :data:`PER_CYCLE`, x_mode (2, N, 3), counts = (cycles, images, converged)."""
    import dimer_cases as DC
    from pdb2reaction_amd import dimer as D
    from pdb2reaction_amd import modes as M

    base = np.random.default_rng(1).standard_normal((10, 3))
    out = {}
    for name, (a, k, kw) in modes_runs().items():
        kw = dict(kw)
        kw.setdefault("project", "none")
        res = M.lowest_modes(M.HostBackend(M.dense_hvp(a)), base, kw.pop("masses", np.ones(10)), k, tol=1e-9, **kw)
        out[name + "/eigenvalues"], out[name + "/history"] = res.eigenvalues, np.array(res.history)
        out[name + "/counts"] = np.array([res.iterations, res.products, res.images, res.restarts], dtype=np.int64)
    for name, (ef, x0, n0, kw) in dimer_runs().items():
        for i, r in enumerate(D.refine_saddles(D.HostBackend(DC.fd_hvp(ef)), x0, n0, **kw)):
            out[f"{name}/{i}/per_cycle"] = np.array([[h[f] for f in PER_CYCLE] for h in r.history], dtype=np.float64)
            out[f"{name}/{i}/x_mode"] = np.stack([r.x, r.mode])
            out[f"{name}/{i}/counts"] = np.array([r.cycles, r.images, int(r.converged)], dtype=np.int64)
    return out


if __name__ == "__main__":
    arrays = compute()
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {len(arrays)} arrays, {os.path.getsize(OUT)} bytes")
