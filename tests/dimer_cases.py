"""Cases and yardsticks of the dimer tests (tests/test_dimer_cpu.py, tests/test_dimer_facades_cpu.py, tests/test_gpu_rows_kernels.py,
tests/test_gpu_dimer.py).

The saddle fixture.  ``Z`` is ``synth.make_cluster(12, seed=4)[0]``; ``X`` is a first-order saddle of the synthetic surface (weights seed
0, open boundaries, no neighbour cap binding), found by the algorithm of pdb2reaction_amd/dimer.py on the float64 checker
(``pinned_cases.checker(weights, max_neigh=None)``).  There the checker gives max|F| = 1.6e-3 eV/A and a symmetrised central-difference
Hessian (step 1e-3) with eigenvalues -0.585, six within +-1.1e-4 (translations and rotations), then +0.113, +0.251, ... up to 7.19
eV/A^2.  From the starts ``start(s)`` (0.02 A noise), with the exact lowest mode plus 5 % noise and the ``gau`` thresholds, the host
backend over the checker (tests/test_dimer_cpu.py, starts 0, 1, 2) converges in 3 / 4 / 4 cycles (11 / 14 / 14 images; a cycle is one
evaluation of the geometry, the last being the one that meets the thresholds), to within 0.036 A of ``X``, C between -0.69 and -0.60,
|mode . exact| >= 0.999.  The bounds of the tests -- 15 cycles, 0.1 A, C in [-0.9, -0.4] -- were set when the fixture was made, from runs
of five starts that ended within 0.037 A with C between -0.70 and -0.57; starts of 0.05 A noise left the basin in 1 of 5 at thresholds
(2e-3, 1e-3) eV/A, so the tests use 0.02.

The analytic surfaces are functions ``x (N,3) -> (E, F (N,3) float64)``; :func:`fd_hvp` turns one into an ``hvp`` callable that does what
``umx_hvp``'s forward scheme does -- forces rounded to float32, differenced in float64 at the given step."""
import numpy as np

import hvp_cases as HC

Z = [6, 8, 1, 1, 8, 1, 1, 1, 1, 1, 7, 1]
MAX_NEIGH = 11                                                               # 12 atoms: a cap of 11 cannot bind
X = np.array([[0.85450973, -1.13282989, 2.81499359], [0.975781, -2.75653882, 1.34796147], [0.71949827, 1.20598505, -3.06815369],
              [-0.21415408, 2.79396172, -0.16575045], [-2.68911922, -1.25190752, 1.563203], [-0.77870076, 0.86062161, 1.25496488],
              [2.41749183, 0.70254172, -0.06646697], [-1.7333507, 0.45093067, -3.12393688], [2.12138875, -0.5491041, -2.06032087],
              [-2.82099671, -0.58281763, -1.14598759], [0.64018458, -3.7980574, 2.59440387], [-1.06089748, -1.73544651, -2.30046409]])
NOISE = 0.02
N_STARTS = 5
GAU = (4.5e-4 / 0.01944690379830087, 3.0e-4 / 0.01944690379830087)           # gsm.THRESH["gau"] forces, Hartree/Bohr -> eV/A: 2.314e-2, 1.543e-2


def start(s):
    return X + NOISE * np.random.default_rng(400 + s).standard_normal((12, 3))


def noisy_mode(mode, s, level=0.05):
    """``mode`` (N,3) unit vector plus ``level`` of noise per unit norm, not normalised again."""
    m = np.asarray(mode, dtype=np.float64)
    r = np.random.default_rng(500 + s).standard_normal(m.shape)
    return m + level * r / np.linalg.norm(r)


def fd_hessian(energy_forces, x, step=1e-3):
    """Symmetrised central-difference Hessian (3N,3N) of a function ``x (N,3) -> (E, F)``."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    h = np.empty((n, n))
    for c in range(n):
        d = np.zeros(n)
        d[c] = step
        fp = energy_forces(x + d.reshape(x.shape))[1].reshape(n)
        fm = energy_forces(x - d.reshape(x.shape))[1].reshape(n)
        h[:, c] = -(fp - fm) / (2.0 * step)
    return 0.5 * (h + h.T)


def fd_hvp(energy_forces, log=None):
    """An ``hvp`` callable of ``Engine.hvp``'s shape over ``energy_forces``: forward scheme only, float32 forces, float64 difference."""

    def hvp(bases, dirs, base_of=None, step=1e-3, scheme="forward", return_base=False, base_forces=None):
        assert scheme == "forward"
        b = np.asarray(bases, dtype=np.float64)
        b = b[None] if b.ndim == 2 else b
        d = np.asarray(dirs, dtype=np.float64)
        d = d[None] if d.ndim == 2 else d
        bo = np.zeros(len(d), dtype=int) if base_of is None else np.asarray(base_of, dtype=int)
        if log is not None:
            log.append((len(b), len(d), base_forces is not None))
        if base_forces is None:
            ef = [energy_forces(r) for r in b]
            e0 = np.array([e for e, _ in ef], dtype=np.float64)
            f0 = np.stack([f for _, f in ef]).astype(np.float32)
        else:
            e0, f0 = None, np.asarray(base_forces, dtype=np.float32).reshape(b.shape)
        fp = np.stack([energy_forces(b[bo[m]] + step * d[m])[1] for m in range(len(d))]).astype(np.float32)
        hv = -(fp.astype(np.float64) - f0[bo].astype(np.float64)) / step
        return (hv, e0, f0) if return_base else hv

    return hvp


# ---- analytic surfaces ---------------------------------------------------------------------------------------------------------------------
def surface_a(q):
    """``E = d.A.d / 2 + q sum d^4``, d = x - base, with ``hvp_cases.quadratic(30, 5)``: a saddle at the base point, curvature -0.7.
    (energy_forces, saddle (10,3), Hessian at the saddle (30,30))."""
    a, base = HC.quadratic(30, 5)

    def ef(x):
        d = np.asarray(x, dtype=np.float64).reshape(-1) - base
        return 0.5 * d @ a @ d + q * (d ** 4).sum(), -(a @ d + 4.0 * q * d ** 3).reshape(-1, 3)

    return ef, base.reshape(10, 3).copy(), a


def surface_b(seed=7):
    """A 36-dimensional double well ``(x0^2 - 1)^2 + sum k_i x_i^2 / 2`` (i >= 1, k in [0.5, 4]) plus ``x.S.x / 2`` with S a random
    symmetric matrix of entries 0.05 N(0,1): a saddle at the origin.  (energy_forces, saddle (12,3), Hessian at the saddle)."""
    rng = np.random.default_rng(seed)
    k = np.concatenate([[0.0], rng.uniform(0.5, 4.0, size=35)])
    s = rng.standard_normal((36, 36))
    s = 0.05 * 0.5 * (s + s.T)

    def ef(x):
        v = np.asarray(x, dtype=np.float64).reshape(-1)
        e = (v[0] ** 2 - 1.0) ** 2 + 0.5 * (k * v * v).sum() + 0.5 * v @ s @ v
        g = k * v + s @ v
        g[0] += 4.0 * v[0] * (v[0] ** 2 - 1.0)
        return e, -g.reshape(-1, 3)

    hess = np.diag(k) + s
    hess[0, 0] += -4.0
    return ef, np.zeros((12, 3)), hess


def checker_surface(weights):
    """(energy_forces of the float64 checker on the fixture's system, the checker)."""
    import pinned_cases as PC

    orc = PC.checker(weights, max_neigh=None)
    return (lambda x: PC.energy_forces_on(orc, Z, x)), orc


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


SCALARS = ("energy", "curvature", "converged", "reason", "cycles", "images", "max_force", "rms_force")
RECORD_SCALARS = ("energy", "max_force", "curv_probe", "curvature", "rotations", "step_max")


def same_result(r1, r2):
    """Every field and every history record of two ``SaddleResult``, bit for bit.  Returns the name of the first difference, or None."""
    for f in ("x", "forces", "mode"):
        if not same_bits(getattr(r1, f), getattr(r2, f)):
            return f
    for f in SCALARS:
        a, b = getattr(r1, f), getattr(r2, f)
        if isinstance(a, float):
            if not same_bits(np.float64(a), np.float64(b)):
                return f
        elif a != b:
            return f
    if len(r1.history) != len(r2.history):
        return "history length"
    for t, (h1, h2) in enumerate(zip(r1.history, r2.history)):
        if sorted(h1) != sorted(h2):
            return f"history[{t}] keys"
        for f in ("x", "n"):
            if not same_bits(h1[f], h2[f]):
                return f"history[{t}].{f}"
        for f in RECORD_SCALARS:
            if not same_bits(np.float64(h1[f]), np.float64(h2[f])):
                return f"history[{t}].{f}"
    return None
