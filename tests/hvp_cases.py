"""Cases and NumPy yardsticks of the Hessian-vector-product tests (tests/test_hvp_cpu.py, tests/test_gpu_hvp.py).

``umx_hvp`` forms the displaced images ``base +- step * dir`` in float64 on the device, evaluates them in one batch on the pinned
graphs of their bases and differences the float32 forces in float64.  The exact yardstick is the same thing done by hand: the NumPy
expressions below for the images, one ``energy_forces(x[None], double_positions=True)`` per image under
``pin_graph(base, double_positions=True)``, and :func:`combine` on those forces.  The float64 yardstick is the checker of
tests/pinned_cases.py on the base's fixed graph, differenced at the same step.

Bases (the smallest at which the entry can go wrong):
  ``swap``       the 12-atom rank-swap cluster at ``max_neigh = 4`` (48 edges): the cap binds, the truncating fill builds the pin;
  ``odd47``      the 47-edge reference of tests/pinned_graphs_cases.py: an ODD edge count, so that without the even-row rule +v and -v
                 would start on rows of different parity;
  ``triclinic``  the 12-atom triclinic cell of tests/stress_oracle.py: translations, self images.
``even48`` is ``swap``'s start geometry under another name where a test needs an even count and says so."""
import numpy as np

import pinned_cases as PC
import pinned_graphs_cases as GC
from stress_oracle import make_case

STEPS = (1e-3, 5e-3)
SCHEMES = ("central", "forward")
M_DIRS = 3


def bases(weights):
    """name -> dict(z, x (N,3) float64, cell, pbc, max_neigh)."""
    out = {}
    z, orc, x0, xm, xs, u, j = PC.cluster_swap(weights)
    out["swap"] = dict(z=z, x=x0, cell=None, pbc=None, max_neigh=PC.MAX_NEIGH)
    z47, refs, _, _, mn = GC.reference_set("open12_capped")
    out["odd47"] = dict(z=z47, x=refs[2].astype(np.float64), cell=None, pbc=None, max_neigh=mn)
    zt, imgs, cell, pbc = make_case("triclinic")
    out["triclinic"] = dict(z=zt, x=imgs[0].astype(np.float64), cell=cell, pbc=pbc, max_neigh=None)
    return out


def directions(n_atoms, m=M_DIRS, seed=11):
    """(m, n_atoms, 3) float64 random directions, NOT normalised (the engine does not normalise either)."""
    return np.random.default_rng(seed).standard_normal((m, n_atoms, 3))


def images(base, dirs, step, scheme, base_of=None):
    """The displaced images in the engine's order, formed as the engine forms them: product and sum rounded separately in float64.
    ``base`` (N,3) or (R,N,3); central: 2m is +, 2m + 1 is -; forward: the bases first."""
    b = np.asarray(base, dtype=np.float64)
    b = b[None] if b.ndim == 2 else b
    d = np.asarray(dirs, dtype=np.float64)
    bo = np.zeros(len(d), dtype=int) if base_of is None else np.asarray(base_of, dtype=int)
    if scheme == "central":
        out = np.empty((2 * len(d),) + d.shape[1:])
        out[0::2] = b[bo] + step * d
        out[1::2] = b[bo] - step * d
        return out
    return np.concatenate([b, b[bo] + step * d])


def combine(forces, step, scheme, n_bases=1, base_of=None):
    """hv (M,N,3) float64 from the float32 forces of :func:`images`, in the engine's operation order (central: hessian.fd_hessian's)."""
    f = np.asarray(forces)
    assert f.dtype == np.float32
    f = f.astype(np.float64)
    if scheme == "central":
        return -(f[0::2] - f[1::2]) / (2.0 * step)
    m = len(f) - n_bases
    bo = np.zeros(m, dtype=int) if base_of is None else np.asarray(base_of, dtype=int)
    return -(f[n_bases:] - f[bo]) / step


def curvature_exact(dirs, hv):
    """(curv (M,), bound (M,)): dir.hv / dir.dir in extended precision, and the issue's bound 3N 2^-52 sum|d hv| / sum d^2."""
    d = np.asarray(dirs, dtype=np.longdouble).reshape(len(dirs), -1)
    h = np.asarray(hv, dtype=np.longdouble).reshape(len(hv), -1)
    den = (d * d).sum(axis=1)
    curv = ((d * h).sum(axis=1) / den).astype(np.float64)
    bound = (d.shape[1] * 2.0 ** -52 * np.abs(d * h).sum(axis=1) / den).astype(np.float64)
    return curv, bound


def checker_hv(orc, z, base, dirs, step, graph):
    """The float64 checker's central difference of its forces at the same step, on ``graph`` held fixed: (M,N,3) eV/A^2."""
    out = []
    for d in np.asarray(dirs, dtype=np.float64):
        fp = PC.energy_forces_on(orc, z, base + step * d, graph)[1]
        fm = PC.energy_forces_on(orc, z, base - step * d, graph)[1]
        out.append(-(fp - fm) / (2.0 * step))
    return np.stack(out)


# ---- CPU stand-ins ---------------------------------------------------------------------------------------------------------------------
def quadratic(n=30, seed=5):
    """A random symmetric n x n matrix with exactly one negative eigenvalue, and a base point."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    w = np.concatenate([[-0.7], rng.uniform(0.3, 4.0, size=n - 1)])
    a = (q * w) @ q.T
    return 0.5 * (a + a.T), rng.standard_normal(n)
