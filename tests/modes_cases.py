"""Cases and NumPy yardsticks of the lowest-modes tests (tests/test_modes_cpu.py, tests/test_modes_facades_cpu.py,
tests/test_gpu_modes_kernels.py, tests/test_gpu_modes.py).

The solver (pdb2reaction_amd/modes.py) asks for the k lowest eigenpairs of ``A = P W H W P`` through Hessian-vector products.  The
yardstick is the same matrix written out: :func:`dense_reference` projects a dense mass-weighted matrix in NumPy float64, symmetrises it
and returns its sorted eigenpairs on range(P) (the zero modes of the projector and of frozen rows are taken out by construction, not by
a threshold on the eigenvalues)."""
import numpy as np

from pdb2reaction_amd import modes as M

# standard atomic weights (amu), by atomic number -- a fixed table: the package has none
MASS_BY_Z = {1: 1.008, 2: 4.0026, 3: 6.94, 4: 9.0122, 5: 10.81, 6: 12.011, 7: 14.007, 8: 15.999, 9: 18.998, 10: 20.180, 11: 22.990,
             12: 24.305, 13: 26.982, 14: 28.085, 15: 30.974, 16: 32.06, 17: 35.45, 18: 39.948, 19: 39.098, 20: 40.078, 35: 79.904}

K, BLOCK, MAX_SUBSPACE = 2, 2, 8                                             # the engine cases: restarts must happen
STEP = 1e-3


def masses_of(z):
    return np.array([MASS_BY_Z[int(a)] for a in z], dtype=np.float64)


def near_degenerate(n=30, seed=9, split=1e-3):
    """A random symmetric n x n matrix whose two lowest eigenvalues are ``-0.5`` and ``-0.5 + split``; the others lie in [0.4, 4]."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    w = np.concatenate([[-0.5, -0.5 + split], rng.uniform(0.4, 4.0, size=n - 2)])
    a = (q * w) @ q.T
    return 0.5 * (a + a.T)


def weights_vector(masses, frozen=()):
    w = 1.0 / np.sqrt(np.asarray(masses, dtype=np.float64))
    w[list(frozen)] = 0.0
    return np.repeat(w, 3)


def dense_reference(h, base, masses, frozen=(), project="tr"):
    """(eigenvalues ascending, eigenvectors as rows, Q, the projected unsymmetrised matrix) of ``P W h W P`` restricted to range(P) and to the active
    coordinates: an orthonormal basis Z of that space is built from the null space of [Q; frozen unit vectors], the matrix is
    symmetrised there, ``eigh`` is applied to ``Z^T B Z`` and the vectors are mapped back."""
    base = np.asarray(base, dtype=np.float64).reshape(-1, 3)
    na = len(base)
    active = np.ones(na, dtype=bool)
    active[list(frozen)] = False
    q = M.tr_vectors(base, np.asarray(masses, dtype=np.float64), active, project)
    w = weights_vector(masses, frozen)
    b = w[:, None] * np.asarray(h, dtype=np.float64) * w[None, :]
    out = np.concatenate([q, np.eye(3 * na)[w == 0.0]])
    if len(out):
        _, s, vt = np.linalg.svd(out, full_matrices=True)
        z = vt[int((s > 1e-10).sum()):]
    else:
        z = np.eye(3 * na)
    pb = z @ b @ z.T
    lam, s = np.linalg.eigh(0.5 * (pb + pb.T))
    return lam, (z.T @ s).T, q, pb


def sin_largest_angle(u, v):
    """sin of the largest principal angle between the row spaces of ``u`` and ``v`` (both k x n)."""
    qu, _ = np.linalg.qr(np.asarray(u).T)
    qv, _ = np.linalg.qr(np.asarray(v).T)
    return float(np.linalg.svd(qu - qv @ (qv.T @ qu), compute_uv=False)[0])      # ||(I - Pv) Qu||_2: accurate for small angles too


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_result(r1, r2):
    """Every field of two ModesResult, bit for bit."""
    for f in ("eigenvalues", "freqs_cm", "modes_mw", "modes", "residuals", "converged"):
        if not same_bits(getattr(r1, f), getattr(r2, f)):
            return False
    return (r1.iterations, r1.products, r1.images, r1.restarts, r1.reason, r1.history) == (r2.iterations, r2.products, r2.images, r2.restarts, r2.reason, r2.history)


def kernel_data(p, n, seed):
    """(p, n) float64 random rows with negative zeros, and (p >= 3) a zero row."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((p, n))
    x[rng.random((p, n)) < 0.1] = -0.0
    if p >= 3:
        x[1] = 0.0
    return x
