"""Lowest vibrational modes without a Hessian: block Davidson on Hessian-vector products (``umx_hvp``).

The reference decides whether a stationary point is a transition state from the lowest eigenpairs of the mass-weighted,
translation/rotation-projected Hessian, and builds the whole Hessian first (``tsopt.py`` ``_mode_direction_by_root``, ``freq.py``): 6N
displaced images.  Here the same eigenpairs cost some tens of batched products.

Operator.  ``A u = P (w * H (w * P u))`` on row vectors of length n = 3N: ``H v`` is one ``hvp`` of the engine (central differences of
the forces on the pinned graph of the base, float64 images), ``w[c] = 1 / sqrt(m)`` of the coordinate's atom and 0 on frozen atoms,
``P = I - Q^T Q`` with Q the orthonormalised mass-weighted translations and rotations about the centre of mass of the active atoms.
The eigenvalues are in eV/A^2/amu; ``freqs_cm = sign(lambda) sqrt(|lambda|) * FREQ_CM`` (:data:`FREQ_CM`, 521.47...).

Algorithm.  Block Davidson without a preconditioner: Rayleigh-Ritz on a growing orthonormal basis V with AV kept beside it, expansion
by the projected residuals of the unconverged pairs, thick restart on the lowest Ritz vectors (no new products).  Per iteration ONE
``hvp`` call (the new block's directions) and a handful of reads of matrices of at most 64 x 64 doubles; nothing of length n leaves the
device before the result.

Backends: :class:`DeviceBackend` (an ``Engine``: ``hvp_dev`` on torch's current stream) and :class:`HostBackend` (any ``hvp(base, dirs,
step=, scheme=)`` callable: ``Engine.hvp``, ``LocalEnginePool.hvp``, a dense matrix) are the two row classes of rowblocks.py -- which
states the vector interface and its bit-for-bit contract -- plus this solver's products.

Not provided: a preconditioner; thermochemistry; products through the graph-parallel entries; use inside the GSM run loop
(``optimize_path_gsm(hei_modes=k)`` is one call after the run).  The transition-state optimiser on the same products is dimer.py."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import numpy as np

from .rowblocks import BLK_MAX, DeviceRows, HostRows, blk_combine, blk_gram, blk_scale, takes  # noqa: F401  (the statements: re-exported)

# ---- sqrt(eV/A^2/amu) in cm^-1, from CODATA-2018 values written out ---------------------------------------------------------------------
ELEMENTARY_CHARGE_C = 1.602176634e-19          # J per eV (exact)
ATOMIC_MASS_KG = 1.66053906660e-27             # kg per amu
SPEED_OF_LIGHT_CM_S = 2.99792458e10            # cm/s (exact)
ANGSTROM_M = 1.0e-10
# omega = sqrt(lambda [eV/A^2/amu] * e / (A^2 * amu)) rad/s; wavenumber = omega / (2 pi c)
FREQ_CM = math.sqrt(ELEMENTARY_CHARGE_C / (ANGSTROM_M * ANGSTROM_M * ATOMIC_MASS_KG)) / (2.0 * math.pi * SPEED_OF_LIGHT_CM_S)

Q_RANK_TOL = 1e-8                              # singular values of Q below this fraction of the largest are dropped (linear molecule: rank 5)
# The default convergence threshold on ||A x - theta x|| in eV/A^2/amu: four times the worst residual floor measured in
# profiles/lowest_modes.txt (4.5e-4, the 50-atom cluster; 2.6e-4 .. 4.4e-4 on the 12-atom cases and at 2000 atoms).  The floor is the
# finite-difference operator's own asymmetry -- float32 forces over 2 step -- and was 0.6 .. 0.7 of asym = ||(B - B^T) / 2||_2.
DEFAULT_TOL = 1.8e-3


# ---- backends: the rows of rowblocks.py plus the products ---------------------------------------------------------------------------------
class HostBackend(HostRows):
    """The products come from ``hvp(base (N,3), dirs (M,N,3), step=, scheme=) -> (M,N,3)``.
    ``pinner``: an object with ``pin_graph / unpin_graph / pinned_graph`` (an ``Engine``, a ``LocalEnginePool``) whose graph the solver
    pins around its products, or None (a dense matrix has no graph)."""

    def __init__(self, hvp: Callable, pinner=None):
        self._hvp, self.pinner = hvp, pinner
        self._reuse = takes(hvp, "base_forces") and takes(hvp, "return_base")
        self._f0 = None
        self._wide = None

    def hvp(self, base, d, step, scheme):
        """(hv block, images spent)."""
        m, n = d.shape
        dirs = d.reshape(m, n // 3, 3)
        if scheme == "forward" and self._reuse:
            wide = bool(getattr(self.pinner, "widened", False))
            if self._f0 is None or wide != self._wide:                        # forces of a narrower arithmetic are not re-used
                hv, _, self._f0 = self._hvp(base, dirs, step=step, scheme=scheme, return_base=True)
                self._wide = bool(getattr(self.pinner, "widened", False))
                return np.asarray(hv, dtype=np.float64).reshape(m, n), m + 1
            hv = self._hvp(base, dirs, step=step, scheme=scheme, base_forces=self._f0)
            return np.asarray(hv, dtype=np.float64).reshape(m, n), m
        hv = self._hvp(base, dirs, step=step, scheme=scheme)
        return np.asarray(hv, dtype=np.float64).reshape(m, n), (2 * m if scheme == "central" else m + 1)

    def check(self):
        pass


class DeviceBackend(DeviceRows):
    """The products are ``hvp_dev`` of the engine on torch's current stream; the base and its forces stay on the device."""

    def __init__(self, engine):
        super().__init__(engine)
        self.pinner = engine
        self._f0 = None
        self._base = None

    def hvp(self, base, d, step, scheme):
        m, n = d.shape
        if self._base is None:
            self._base = self.put(base, ndmin=0)                               # (N,3), C-contiguous: the solver's x0
        hv = self.empty(m, n)
        if scheme == "forward":
            given = self._f0 is not None
            if not given:
                self._f0 = self.empty(n // 3, 3, dtype=self.torch.float32)
            self.engine.hvp_dev(1, self._base.data_ptr(), m, d.data_ptr(), hv.data_ptr(), step=step, scheme=scheme, d_f0=self._f0.data_ptr(),
                                given_f0=given, stream=self._stream())
            return hv, (m if given else m + 1)
        self.engine.hvp_dev(1, self._base.data_ptr(), m, d.data_ptr(), hv.data_ptr(), step=step, scheme=scheme, stream=self._stream())
        return hv, 2 * m

    def check(self):
        """The device entry reports a range violation late: a non-finite Rayleigh-Ritz matrix lands here."""
        if self.engine.take_range_error():
            raise RuntimeError(f"lowest_modes: non-finite energy in a batch of displaced images (precision mode {self.engine.precision_mode()})")


# ---- the projector ------------------------------------------------------------------------------------------------------------------------
def tr_vectors(base: np.ndarray, masses: np.ndarray, active: np.ndarray, project: str) -> np.ndarray:
    """Q (r, 3N): the orthonormalised mass-weighted translations (``project="t"``) and rotations about the centre of mass of the active
    atoms (``"tr"``), zero on the other atoms; singular values below ``Q_RANK_TOL`` of the largest are dropped.  ``"none"``: (0, 3N)."""
    n = len(masses)
    if project == "none":
        return np.zeros((0, 3 * n))
    sm = np.where(active, np.sqrt(masses), 0.0)
    raw = np.zeros((6 if project == "tr" else 3, n, 3))
    for a in range(3):
        raw[a, :, a] = sm
    if project == "tr":
        m_act = np.where(active, masses, 0.0)
        r = base - (m_act[:, None] * base).sum(axis=0) / m_act.sum()
        for a in range(3):
            e = np.zeros(3)
            e[a] = 1.0
            raw[3 + a] = sm[:, None] * np.cross(e[None, :], r)
    _, s, vt = np.linalg.svd(raw.reshape(len(raw), -1), full_matrices=False)
    return np.ascontiguousarray(vt[s > Q_RANK_TOL * s[0]])


@dataclass
class ModesResult:
    """``eigenvalues`` (k,) eV/A^2/amu, ascending; ``freqs_cm`` (k,) signed wavenumbers (negative = imaginary); ``modes_mw`` (k,3N) unit
    eigenvectors of the mass-weighted operator; ``modes`` (k,N,3) the Cartesian displacements ``w * u`` normalised (the reference's
    convention; zero rows on frozen atoms); ``residuals`` (k,) ``||A u - theta u||``; ``converged`` (k,) bool; ``iterations`` = ``hvp``
    calls; ``products`` directions sent through them; ``images`` evaluations spent; ``restarts``; ``reason``: "converged", "max_iter" or
    "no expansion vector"; ``history``: the largest of the k residual norms after every iteration."""
    eigenvalues: np.ndarray
    freqs_cm: np.ndarray
    modes_mw: np.ndarray
    modes: np.ndarray
    residuals: np.ndarray
    converged: np.ndarray
    iterations: int
    products: int
    images: int
    restarts: int
    reason: str = "converged"
    history: tuple = ()

    @property
    def n_imaginary(self) -> int:
        return int((self.eigenvalues < 0.0).sum())


def resolve_project(project: str, periodic: bool, any_frozen: bool) -> str:
    if project not in ("tr", "t", "none", "auto"):
        raise ValueError(f"lowest_modes: project must be 'tr', 't', 'none' or 'auto', got {project!r}")
    if project != "auto":
        return project
    if not periodic:
        return "tr"                                    # the reference's behaviour, frozen atoms or not
    return "none" if any_frozen else "t"


def lowest_modes(backend, base, masses, k: int = 1, *, frozen: Sequence[int] = (), project: str = "auto", step: float = 1e-3,
                 scheme: str = "central", block: Optional[int] = None, max_subspace: Optional[int] = None, tol: Optional[float] = None,
                 max_iter: int = 200, v0=None, seed: int = 0, periodic: bool = False) -> ModesResult:
    """The ``k`` lowest eigenpairs of ``A = P W H W P`` at ``base`` (N,3) Angstrom, ``masses`` (N,) amu, through ``backend``.

    frozen: atom indices held fixed (``w = 0`` on their rows: the active block, the reference's PHVA).
    project: "tr" (translations and rotations), "t", "none", or "auto" -- "tr" for open boundaries, "t" in a cell (``periodic``)
    without frozen atoms, "none" in a cell with frozen atoms.  Every basis vector is kept in range(P): zero modes never appear.
    step, scheme: of every ``hvp``; ``step`` (default 1e-3 A) is per unit of the Cartesian direction ``w * u``, so a probe displaces
    the geometry by ``step * ||w * u|| <= step / sqrt(m_min)`` Angstrom.  "forward" evaluates the base once and hands its forces back
    to every later product (``base_forces``; flags bit 2).
    block: directions per iteration (default ``max(2 k, 4)``; the first block has ``max(block, k)``); max_subspace: the basis restarts
    on its ``max(k, max_subspace // 2)`` lowest Ritz vectors when the next block would exceed it (default ``min(64, 8 block)``; <= 64).
    tol: all k residual norms ``<= tol`` stop the iteration (default :data:`DEFAULT_TOL` = 1.8e-3 eV/A^2/amu, four times the worst
    residual floor of profiles/lowest_modes.txt -- the finite-difference operator is not symmetric below that).
    v0: (j,3N) or (j,N,3) start vectors in the mass-weighted space (a string tangent, a previous mode); the block is filled up
    from ``numpy.random.default_rng(seed).standard_normal``.
    The solver pins the graph of ``base`` once (``pin_graph(base, double_positions=True)``) and unpins on every way out; under a
    caller's pin it uses that pin and leaves it.  Ending conditions are reported (``converged``, ``reason``), not raised."""
    be = backend
    x0 = np.ascontiguousarray(base, dtype=np.float64).reshape(-1, 3)
    na = x0.shape[0]
    n = 3 * na
    m_amu = np.asarray(masses, dtype=np.float64).reshape(-1)
    if m_amu.shape[0] != na or not (np.isfinite(m_amu).all() and (m_amu > 0.0).all()):
        raise ValueError(f"lowest_modes: masses must be {na} finite positive numbers (amu)")
    if scheme not in ("central", "forward"):
        raise ValueError(f"lowest_modes: scheme must be 'central' or 'forward', got {scheme!r}")
    if not (np.isfinite(step) and step > 0.0):
        raise ValueError(f"lowest_modes: the step must be finite and positive, got {step!r}")
    fz = sorted(set(int(i) for i in frozen))
    if fz and (fz[0] < 0 or fz[-1] >= na):
        raise ValueError(f"lowest_modes: frozen atom outside [0, {na})")
    active = np.ones(na, dtype=bool)
    active[fz] = False
    how = resolve_project(project, periodic, bool(fz))
    q_host = tr_vectors(x0, m_amu, active, how)
    n_free = 3 * int(active.sum()) - len(q_host)
    k = int(k)
    if k < 1 or k > min(n_free, BLK_MAX // 2):
        raise ValueError(f"lowest_modes: k = {k} must lie in [1, {min(n_free, BLK_MAX // 2)}] ({n_free} free dimensions)")
    block = min(max(2 * k, 4) if block is None else int(block), n_free)
    if block < 1:
        raise ValueError("lowest_modes: block must be positive")
    first = max(block, k)
    max_subspace = min(BLK_MAX, 8 * first) if max_subspace is None else int(max_subspace)
    if max_subspace > BLK_MAX or max(k, max_subspace // 2) + block > max_subspace or first > max_subspace:
        raise ValueError(f"lowest_modes: max_subspace = {max_subspace} must be <= {BLK_MAX} and hold max(k, max_subspace // 2) + block rows "
                         f"(k = {k}, block = {block})")
    tol = DEFAULT_TOL if tol is None else float(tol)
    w_host = np.repeat(np.where(active, 1.0 / np.sqrt(m_amu), 0.0), 3)
    w = be.vector(w_host)
    mask = be.vector((w_host != 0.0).astype(np.float64)) if fz else None
    qd = be.put(q_host) if len(q_host) else None

    def proj(u):
        if mask is not None:
            u = be.scale(u, mask)
        if qd is not None:
            u = be.combine(qd, be.gram(qd, u), u, True)
        return u

    def orthonormal(u, basis):
        """``u`` projected, made orthogonal to ``basis`` (two passes of classical Gram-Schmidt) and orthonormal in itself (the eigenvectors of
        its small Gram matrix, on the host); negligible directions are dropped.  The whole is done twice.  None when nothing is left."""
        u = proj(u)
        for thresh in (1e-8, 1e-8):
            if basis is not None:
                for _ in range(2):
                    u = be.combine(basis, be.gram(basis, u), u, True)
            g = be.gram(u, u)
            dg = np.diag(g).copy()
            keep = np.flatnonzero(dg > 1e-60)
            if len(keep) == 0:
                return None
            d = 1.0 / np.sqrt(dg[keep])
            lam, s = np.linalg.eigh(0.5 * (g[np.ix_(keep, keep)] + g[np.ix_(keep, keep)].T) * d[:, None] * d[None, :])
            good = np.flatnonzero(lam > thresh * max(lam[-1], 1.0))[::-1]          # the best-conditioned direction first
            if len(good) == 0:
                return None
            c = np.zeros((be.rows(u), len(good)))
            c[keep] = d[:, None] * s[:, good] / np.sqrt(lam[good])[None, :]
            u = be.combine(u, c, None, False)
        return u

    def apply(u):
        hv, imgs = be.hvp(x0, be.scale(proj(u), w), float(step), scheme)
        return proj(be.scale(hv, w)), imgs

    rng = np.random.default_rng(seed)
    start = np.zeros((0, n))
    if v0 is not None:
        start = np.array(v0, dtype=np.float64)
        if start.size == 0 or start.size % n != 0:
            raise ValueError(f"lowest_modes: v0 must be (j,3N) or (j,N,3) with N = {na}, got {np.shape(v0)}")
        start = start.reshape(-1, n)[:first]
    if len(start) < first:
        start = np.concatenate([start, rng.standard_normal((first - len(start), n))])

    pinner = getattr(be, "pinner", None)
    own_pin = pinner is not None and pinner.pinned_graph() is None
    if own_pin:
        pinner.pin_graph(x0, double_positions=True)
    try:
        wblk = orthonormal(be.put(start), None)
        v = av = None
        iterations = products = images = restarts = 0
        reason = "max_iter"
        theta = rn = x = None
        history = []
        while wblk is not None and iterations < int(max_iter):
            aw, imgs = apply(wblk)
            iterations += 1
            products += be.rows(wblk)
            images += imgs
            v = wblk if v is None else be.cat([v, wblk])
            av = aw if av is None else be.cat([av, aw])
            g = be.gram(v, av)                                                 # the Rayleigh-Ritz matrix: the read-back of the iteration
            if not np.isfinite(g).all():
                be.check()
                raise RuntimeError("lowest_modes: non-finite Rayleigh-Ritz matrix (non-finite positions, masses or products)")
            evals, s = np.linalg.eigh(0.5 * (g + g.T))
            m = len(evals)
            kk = min(k, m)
            theta = evals[:kk].copy()
            c = np.ascontiguousarray(s[:, :kk])
            x, ax = be.combine(v, c, None, False), be.combine(av, c, None, False)
            r = be.combine(x, np.diag(theta), ax, True)                        # r_i = A x_i - theta_i x_i
            rn = np.sqrt(np.diag(be.gram(r, r)))
            history.append(float(rn.max()))
            if kk == k and (rn <= tol).all():
                reason = "converged"
                break
            if iterations >= int(max_iter):
                break
            todo = [int(i) for i in np.argsort(-rn, kind="stable") if rn[i] > tol][:block]
            wblk = orthonormal(be.take(r, todo), v) if todo else None
            if wblk is None and kk < k:                                        # fewer Ritz pairs than asked for and nothing to add from them
                wblk = orthonormal(be.put(rng.standard_normal((block, n))), v)
            if wblk is None:
                reason = "no expansion vector"
                break
            if m + be.rows(wblk) > max_subspace:
                keep = min(m, max(k, max_subspace // 2))
                ck = np.ascontiguousarray(s[:, :keep])
                v, av = be.combine(v, ck, None, False), be.combine(av, ck, None, False)
                restarts += 1
        if x is None:
            raise RuntimeError("lowest_modes: no admissible start vector (v0 and the random block vanish under the projection)")
        u = be.get(x)
    finally:
        if own_pin:
            pinner.unpin_graph()
    u = u / np.sqrt((u * u).sum(axis=1))[:, None]
    for row in u:                                                              # a fixed sign: the largest component is positive
        if row[np.argmax(np.abs(row))] < 0.0:
            row *= -1.0
    cart = w_host[None, :] * u
    cart = cart / np.sqrt((cart * cart).sum(axis=1))[:, None]
    conv = rn <= tol
    return ModesResult(eigenvalues=theta, freqs_cm=np.sign(theta) * np.sqrt(np.abs(theta)) * FREQ_CM, modes_mw=u, modes=cart.reshape(-1, na, 3),
                       residuals=rn, converged=conv, iterations=iterations, products=products, images=images, restarts=restarts,
                       reason=reason, history=tuple(history))


def dense_hvp(h: np.ndarray) -> Callable:
    """An ``hvp`` callable that applies a dense (3N,3N) matrix exactly -- for tests and for callers who do have a Hessian."""
    h = np.asarray(h, dtype=np.float64)

    def hvp(base, dirs, step=1e-3, scheme="central"):
        d = np.asarray(dirs, dtype=np.float64)
        return (d.reshape(len(d), -1) @ h.T).reshape(d.shape)

    return hvp
