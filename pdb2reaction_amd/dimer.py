"""Refine transition-state guesses to first-order saddles without a Hessian: a batched dimer on Hessian-vector products (``umx_hvp``).

The reference's ``tsopt.HessianDimer`` builds a full finite-difference Hessian for the dimer's first orientation, again every
``update_interval_hessian`` steps and at the end: 6N displaced images each.  A dimer needs per cycle only what ONE forward ``hvp`` call
returns: the energy and forces of the geometry (``e0``, ``f0``: bit for bit its unpinned evaluation) and ``H n`` on its own pinned graph.
``hvp`` takes R bases, so K guesses -- the highest-energy images of a multi-step path, several candidate starts -- advance together, one
batch per product round, as ``lbfgs.BatchedLBFGS`` advances K relaxations.

Algorithm, per candidate (Angstrom, eV, Cartesian, no mass weighting -- the reference's ``Dimer`` is Cartesian too).  ``w`` is the 0/1 mask
of the atoms that are not frozen, ``P = I - Q^T Q`` with ``Q = modes.tr_vectors(x, unit masses, active, how)`` re-formed on the host every
cycle from the current geometry, ``how = modes.resolve_project(project, periodic, any_frozen)``; ``proj(v) = P (w * v)``::

    n <- proj(n0) / ||.||
    cycle t (at most max_cycles):
      one forward product at x along n, step h:  E, F (float32 -> float64), hn = -(F+ - F) / h
      F <- proj(F);  hn <- proj(hn)
      rotation, r = 0 ... max_rot - 1:
         C = n.hn;  g = hn - C n;  rho = ||g||
         if rho <= rot_tol max(|C|, c_floor): break
         theta = g / rho;  ht = proj(H theta)                 # forward product with the forces of x handed back in: ONE image
         a = C, b = (theta.hn + n.ht) / 2, d = theta.ht;  (c, s) = eigenvector of the lowest eigenvalue of [[a, b], [b, d]], c >= 0
         n <- c n + s theta;  hn <- c hn + s ht;  both divided by ||n||      # H is linear: no product for the new n
      C = n.hn
      converged  <=>  C < 0  and  max|F| <= max_force  and  rms(F) <= rms_force       # rms over all 3N entries, frozen rows are zeros
      Feff = F - 2 (F.n) n  if C < 0  else  -(F.n) n
      L-BFGS on -Feff (the last 7 pairs s = dx, y = d(-Feff); the two-loop of lbfgs._two_loop, H0 = s.y / y.y of the newest pair,
         1 / max(|C|, 1) with no pair); the history is dropped when sign(C) changed since the last cycle or s.y <= 0, and is not built
         while C >= 0
      step = two-loop result if C < 0,  else  Feff (max_step / max|Feff|)
      if max|step| > max_step: step <- step (max_step / max|step|);   x <- x + step

A cycle costs 1 + (1 ... 1 + max_rot) images per candidate.  The step criteria of the threshold sets are not applied.

Every dot, norm and maximum is ``row_dot`` / ``row_absmax`` of rowblocks.py, every vector update ``row_axpby`` (``blk_scale`` for the mask,
``blk_gram`` + ``blk_combine`` per candidate for the Q projection); the small scalars -- K numbers per operation -- are combined on the host.  A row's
result never depends on the rows beside it and every image of ``umx_hvp`` is its evaluation alone, so a candidate of a batch is bit for bit
its own K = 1 run.

Backends: the two row classes of rowblocks.py -- which states the vector interface and its bit-for-bit contract -- plus this solver's
products.  :class:`DeviceBackend`: ``hvp_dev`` of the evaluator (the engine by default; any object with a method of that shape) on torch's
current stream; read back per cycle are the K-vectors of scalars and, once, the K geometries and directions (for Q and the trajectory);
the L-BFGS pairs stay on the device.  :class:`HostBackend`: any ``hvp(bases, dirs, base_of=, step=, scheme="forward", return_base=/
base_forces=)`` callable (``Engine.hvp``, a pool's dealing wrapper, an analytic surface).

Graphs: nothing is pinned across cycles -- the geometry moves; each ``hvp`` call pins its own bases and unpins.  Under a caller's pin
:func:`refine_saddles` raises ``ValueError``.  An fp16 range violation widens the engine as ``Engine.hvp`` does; the cycle is repeated and
the L-BFGS histories (forces of the narrower arithmetic) are dropped.

Not provided: the reference's flatten loop for further imaginary modes, Bofill updates, internal coordinates; products through the
graph-parallel entries or ``parallel.py``'s sharded evaluators; per-image cells; a transition-state search from a minimum."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import hessian as H
from . import modes
from .engine import UMX_ERR_RANGE, UmxError
from .gsm import THRESH
from .rowblocks import BLK_MAX, DeviceRows, HostRows, row_absmax, row_axpby, row_dot, takes  # noqa: F401  (the statements: re-exported)

ROW_MAX = BLK_MAX                              # candidates of one call (the row entries take at most BLK_MAX rows)
KEEP_LAST = 7                                  # L-BFGS pairs kept per candidate (lbfgs.BatchedLBFGS's default)
C_FLOOR = 1e-2                                 # eV/A^2: the rotation residual is not chased below rot_tol times this


# ---- backends: the rows of rowblocks.py plus the products ---------------------------------------------------------------------------------
class HostBackend(HostRows):
    """``hvp(bases (k,N,3), dirs (k,N,3), base_of=, step=, scheme="forward", return_base=True) -> (hv, e0, f0)``; with a ``base_forces``
    parameter the rotation products hand ``f0`` back in and cost one image each.
    ``pinner``: the object whose ``pinned_graph()`` / ``widened`` the solver consults (an ``Engine``, a ``LocalEnginePool``), or None."""

    def __init__(self, hvp: Callable, pinner=None, lowest_modes: Optional[Callable] = None):
        self._hvp, self.pinner, self._modes = hvp, pinner, lowest_modes
        self._reuse = takes(hvp, "base_forces")

    def _wide(self) -> bool:
        engines = getattr(self.pinner, "engines", None) or [self.pinner]     # a pool: any of its engines
        return any(bool(getattr(e, "widened", False)) for e in engines)

    def hvp(self, x, d, step, f0=None):
        """``(hv (k,n), e0 (k,) | None, f64 (k,n) | None, f0, widened, failed)``: one forward product per row of ``d`` at the row of
        ``x``; with ``f0`` (an earlier call's) the bases are not evaluated again."""
        k, n = d.shape
        bases, dirs, bo = x.reshape(k, n // 3, 3), d.reshape(k, n // 3, 3), np.arange(k, dtype=np.int32)
        was = self._wide()
        try:
            if f0 is not None and self._reuse:
                hv, e0 = self._hvp(bases, dirs, base_of=bo, step=step, scheme="forward", base_forces=f0), None
            else:
                hv, e0, got = self._hvp(bases, dirs, base_of=bo, step=step, scheme="forward", return_base=True)
                if f0 is None:
                    f0 = np.ascontiguousarray(got, dtype=np.float32).reshape(k, n // 3, 3)
                else:
                    e0 = None
        except UmxError as err:
            if getattr(err, "status", 0) != UMX_ERR_RANGE:
                raise
            return None, None, None, None, False, True
        f64 = None if e0 is None else f0.astype(np.float64).reshape(k, n)
        return np.asarray(hv, dtype=np.float64).reshape(k, n), (None if e0 is None else np.array(e0, dtype=np.float64)), f64, f0, self._wide() != was, False

    def cost(self, given: bool) -> int:
        """Images per direction of a product: the displaced one, and the base unless its forces were handed in."""
        return 1 if given and self._reuse else 2

    def forces(self, f0):
        return np.array(f0, dtype=np.float32)

    def lowest_modes(self, x, masses, k, **kw):
        if self._modes is not None:
            return self._modes(x, masses, k, **kw)
        return modes.lowest_modes(modes.HostBackend(self._hvp, pinner=self.pinner), x, masses, k, **kw)


class DeviceBackend(DeviceRows):
    """``evaluator``: the object whose ``hvp_dev`` gives the products (default: the engine); the row and block entries always come from
    the engine."""

    def __init__(self, engine, evaluator=None):
        super().__init__(engine)
        self.evaluator = engine if evaluator is None else evaluator
        self.pinner = self.evaluator if hasattr(self.evaluator, "pinned_graph") else None

    def hvp(self, x, d, step, f0=None):
        k, n = d.shape
        hv = self.empty(k, n)
        given = f0 is not None
        e0 = None
        if not given:
            f0, e0 = self.empty(k, n // 3, 3, dtype=self.torch.float32), self.empty(k)
        self.evaluator.hvp_dev(k, x.data_ptr(), k, d.data_ptr(), hv.data_ptr(), base_of=np.arange(k, dtype=np.int32), step=step, scheme="forward",
                               d_e0=0 if given else e0.data_ptr(), d_f0=f0.data_ptr(), stream=self._stream(), given_f0=given)
        check = getattr(self.evaluator, "take_range_error", None)
        if check is not None and check():                                      # the device entry reports a range violation late
            widen = getattr(self.evaluator, "_widen", None)
            if widen is not None and widen("non-finite energy in a batch of displaced images"):
                return None, None, None, None, True, False
            return None, None, None, None, False, True
        if given:
            return hv, None, None, f0, False, False
        return hv, e0.cpu().numpy(), f0.to(self.torch.float64).reshape(k, n), f0, False, False

    def cost(self, given: bool) -> int:
        return 1 if given else 2

    def forces(self, f0):
        return f0.cpu().numpy()

    def lowest_modes(self, x, masses, k, **kw):
        if self.evaluator is not self.engine:
            raise ValueError("refine_saddles: modes0 is needed with an evaluator that is not the engine (lowest_modes runs on the engine's own surface)")
        return self.engine.lowest_modes(x, masses, k, **kw)


# ---- the result ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class SaddleResult:
    """One candidate.  ``x`` (N,3) Angstrom: the last geometry evaluated; ``energy`` eV and ``forces`` (N,3) float32 eV/A there, as
    evaluated (not projected); ``mode`` (N,3) the dimer direction, a unit vector; ``curvature`` = mode.H.mode in eV/A^2; ``converged``,
    ``reason`` ("converged", "max_cycles" or "non_finite"); ``cycles`` evaluated; ``images`` spent (those of ``lowest_modes`` for a start
    direction included); ``max_force``, ``rms_force`` of the projected forces, eV/A; ``history``: one dict per cycle -- ``x``, ``n`` at its
    start, ``energy``, ``max_force``, ``curv_probe`` (n.hn before any rotation), ``curvature`` (after), ``rotations``, ``step_max`` (the
    largest component of the step taken; 0.0 when none was).  ``verify=True`` adds ``freqs_cm`` (2,) and ``n_imaginary``."""
    x: np.ndarray
    energy: float
    forces: np.ndarray
    mode: np.ndarray
    curvature: float
    converged: bool
    reason: str
    cycles: int
    images: int
    max_force: float
    rms_force: float
    history: List[dict] = field(default_factory=list)
    freqs_cm: Optional[np.ndarray] = None
    n_imaginary: Optional[int] = None


def force_thresholds(thresh) -> tuple:
    """(max_force, rms_force) in eV/A: the force entries of ``gsm.THRESH[thresh]`` converted from Hartree/Bohr, or a tuple's first two."""
    if isinstance(thresh, str):
        if thresh not in THRESH:
            raise ValueError(f"refine_saddles: thresh must be one of {sorted(THRESH)} or (max_force, rms_force) in eV/A, got {thresh!r}")
        return THRESH[thresh][0] / H.EV_PER_ANG_TO_AU, THRESH[thresh][1] / H.EV_PER_ANG_TO_AU
    t = tuple(float(v) for v in thresh)
    if len(t) < 2 or not (t[0] > 0.0 and t[1] > 0.0):
        raise ValueError(f"refine_saddles: thresh must be a name or (max_force, rms_force) > 0 in eV/A, got {thresh!r}")
    return t[0], t[1]


def _lowest_pair(a: float, b: float, d: float) -> tuple:
    """(c, s), c >= 0: the eigenvector of the lowest eigenvalue of [[a, b], [b, d]]."""
    _, v = np.linalg.eigh(np.array([[a, b], [b, d]]))
    c, s = float(v[0, 0]), float(v[1, 0])
    return (-c, -s) if (c < 0.0 or (c == 0.0 and s < 0.0)) else (c, s)


def refine_saddles(backend, x0, modes0=None, *, frozen: Sequence[int] = (), project: str = "auto", thresh="gau", step: float = 1e-3,
                   max_cycles: int = 200, max_rot: int = 2, rot_tol: float = 0.1, max_step: float = 0.1, masses=None, verify: bool = False,
                   periodic: bool = False, c_floor: float = C_FLOOR, keep_last: int = KEEP_LAST) -> List[SaddleResult]:
    """Refine the guesses ``x0`` (N,3) or (K,N,3) Angstrom, K <= 64, through ``backend``; one :class:`SaddleResult` per candidate.

    modes0: (K,N,3) (or (N,3), (K,3N)) start directions -- a string tangent, a previous mode --, not normalised; None: the lowest mode of
    ``lowest_modes(x0[i], unit masses, k=1)`` per candidate (its images are counted).
    frozen: atom indices held fixed (their rows of every vector are zero, they never move).  project: "tr", "t", "none" or "auto" as in
    ``modes.lowest_modes`` (``periodic`` says whether a cell is bound).  thresh: a name of ``gsm.THRESH`` (its force entries, converted to
    eV/A: "gau" is 2.314e-2 and 1.543e-2) or ``(max_force, rms_force)`` in eV/A.  step: the finite-difference step of every product, A.
    max_rot: rotations per cycle at most; rot_tol: a rotation is made while ``||hn - C n|| > rot_tol max(|C|, c_floor)``.
    max_step: the largest component of a step, A.  verify (needs ``masses`` (N,) amu): one ``lowest_modes(x, masses, k=2)`` per converged
    candidate after the run fills ``freqs_cm`` and ``n_imaginary``.
    Ending conditions are reported per candidate (``reason``), never raised; a converged or failed candidate leaves the batch."""
    be = backend
    xs = np.array(x0, dtype=np.float64)
    if xs.ndim == 2:
        xs = xs[None]
    if xs.ndim != 3 or xs.shape[2] != 3 or xs.shape[0] < 1 or xs.shape[1] < 1:
        raise ValueError(f"refine_saddles: x0 must be (N,3) or (K,N,3), got {np.shape(x0)}")
    kk, na = xs.shape[0], xs.shape[1]
    n = 3 * na
    if kk > ROW_MAX:
        raise ValueError(f"refine_saddles: {kk} candidates, at most {ROW_MAX} advance in one call")
    for i in range(kk):
        if not np.isfinite(xs[i]).all():
            raise ValueError(f"refine_saddles: non-finite position (candidate {i})")
    pinner = getattr(be, "pinner", None)
    if pinner is not None and pinner.pinned_graph() is not None:
        raise ValueError("refine_saddles: a graph is pinned -- the geometries move and every product pins its own bases: call unpin_graph first")
    max_f, rms_f = force_thresholds(thresh)
    if not (np.isfinite(step) and step > 0.0):
        raise ValueError(f"refine_saddles: the step must be finite and positive, got {step!r}")
    if not (np.isfinite(max_step) and max_step > 0.0) or int(max_cycles) < 1 or int(max_rot) < 0 or not rot_tol >= 0.0:
        raise ValueError("refine_saddles: max_step > 0, max_cycles >= 1, max_rot >= 0 and rot_tol >= 0 are needed")
    fz = sorted(set(int(i) for i in frozen))
    if fz and (fz[0] < 0 or fz[-1] >= na):
        raise ValueError(f"refine_saddles: frozen atom outside [0, {na})")
    active = np.ones(na, dtype=bool)
    active[fz] = False
    if not active.any():
        raise ValueError("refine_saddles: every atom is frozen")
    how = modes.resolve_project(project, periodic, bool(fz))
    m_amu = None
    if verify:
        if masses is None:
            raise ValueError("refine_saddles: verify=True needs masses (N values in amu)")
        m_amu = np.asarray(masses, dtype=np.float64).reshape(-1)
        if m_amu.shape[0] != na:
            raise ValueError(f"refine_saddles: {na} atoms, but masses has {m_amu.shape[0]} entries")
    unit = np.ones(na)
    images = np.zeros(kk, dtype=int)
    if modes0 is None:
        start = np.empty((kk, n))
        for i in range(kk):
            res = be.lowest_modes(xs[i], unit, 1, frozen=tuple(fz), project=project, step=float(step))
            start[i] = np.asarray(res.modes[0], dtype=np.float64).reshape(n)
            images[i] += int(res.images)
    else:
        start = np.array(modes0, dtype=np.float64)
        if start.size != kk * n:
            raise ValueError(f"refine_saddles: modes0 must hold one (N,3) direction per candidate ({kk} x {na} x 3), got {np.shape(modes0)}")
        start = start.reshape(kk, n)
        for i in range(kk):
            if not np.isfinite(start[i]).all():
                raise ValueError(f"refine_saddles: non-finite component in modes0 (candidate {i})")
    run = _Batch(be, xs, start, images, active, how, bool(fz), float(step), max_f, rms_f, int(max_cycles), int(max_rot), float(rot_tol),
                 float(c_floor), float(max_step), int(keep_last))
    results = run.run()
    if verify:
        for r in results:
            if r.converged:
                vm = be.lowest_modes(r.x, m_amu, 2, frozen=tuple(fz), project=project, step=float(step))
                r.freqs_cm, r.n_imaginary = np.array(vm.freqs_cm), int(vm.n_imaginary)
    return results


class _Batch:
    """The state of one ``refine_saddles`` call.  ``act`` lists the candidates still in the batch: row j of every block belongs to
    candidate ``act[j]``; per-candidate records (cycles, images, history, L-BFGS pairs, results) are indexed by the candidate."""

    def __init__(self, be, xs, start, images, active, how, any_frozen, step, max_f, rms_f, max_cycles, max_rot, rot_tol, c_floor, max_step,
                 keep_last):
        self.be, self.active, self.how = be, active, how
        self.kk, self.na = xs.shape[0], xs.shape[1]
        self.n = 3 * self.na
        self.step, self.max_f, self.rms_f, self.max_cycles, self.max_rot = step, max_f, rms_f, max_cycles, max_rot
        self.rot_tol, self.c_floor, self.max_step, self.keep_last = rot_tol, c_floor, max_step, keep_last
        self.unit = np.ones(self.na)
        self.w_dev = be.vector(np.repeat(active.astype(np.float64), 3)) if any_frozen else None
        self.images = images
        self.cycles = np.zeros(self.kk, dtype=int)
        self.history = [[] for _ in range(self.kk)]
        self.pairs = [[] for _ in range(self.kk)]      # per candidate, oldest first: (s row, y row, s.y, y.y)
        self.prev = [None] * self.kk                   # (Feff row, step row) of the last cycle when it had C < 0
        self.results: List[Optional[SaddleResult]] = [None] * self.kk
        self.act = list(range(self.kk))
        self.x = be.put(xs.reshape(self.kk, self.n))
        nvec = self.proj(be.put(start), self.q_blocks(xs.reshape(self.kk, self.n)))
        nn = self.norm(nvec)
        for i in range(self.kk):
            if not (np.isfinite(nn[i]) and nn[i] > 0.0):
                raise ValueError(f"refine_saddles: the start direction vanishes under the projection (candidate {i})")
        self.nvec = be.axpby(1.0 / nn, nvec)

    # ---- small pieces ----------------------------------------------------------------------------------------------------------------
    def q_blocks(self, x_host):
        out = []
        for row in x_host:
            q = modes.tr_vectors(row.reshape(self.na, 3), self.unit, self.active, self.how)
            out.append(self.be.put(q) if len(q) else None)
        return out

    def proj(self, u, qs):
        if self.w_dev is not None:
            u = self.be.scale(u, self.w_dev)
        if any(q is not None for q in qs):
            u = self.be.project(qs, u)
        return u

    def norm(self, u):
        return np.sqrt(self.be.dot(u, u))

    def forget(self, idx):
        for i in idx:
            self.pairs[i].clear()
            self.prev[i] = None

    def finish(self, i, reason, x, mode, energy=float("nan"), forces=None, curvature=float("nan"), max_force=float("nan"), rms_force=float("nan")):
        """The one place a candidate's result is written: it has left the batch."""
        na = self.na
        forces = np.full((na, 3), np.nan, dtype=np.float32) if forces is None else forces.reshape(na, 3)
        self.results[i] = SaddleResult(x=np.array(x, dtype=np.float64).reshape(na, 3), energy=float(energy), forces=forces,
                                       mode=np.array(mode, dtype=np.float64).reshape(na, 3), curvature=float(curvature), converged=reason == "converged",
                                       reason=reason, cycles=int(self.cycles[i]), images=int(self.images[i]), max_force=float(max_force),
                                       rms_force=float(rms_force), history=self.history[i])

    def fail_all(self, x_host, n_host):
        """A non-finite energy that wider forward planes do not cure: the batch's evaluation is void, every candidate still in it ends."""
        for j, i in enumerate(self.act):
            self.finish(i, "non_finite", x_host[j], n_host[j])

    def keep(self, rows, *blocks):
        """The rows ``rows`` of every block, and ``act`` cut down with them."""
        self.act = [self.act[j] for j in rows]
        return [self.be.take(b, rows) for b in blocks]

    # ---- rotation ----------------------------------------------------------------------------------------------------------------------
    def rotate(self, hn, f0, qs, c_probe):
        """Up to ``max_rot`` rotations of the candidates whose residual asks for one.  Returns ``(hn, rotations, status)``, status None,
        "widened" or "failed" (a range violation in a product: the caller repeats or ends the cycle); ``self.nvec`` is updated."""
        be, act = self.be, self.act
        rotations = np.zeros(len(act), dtype=int)
        rot = list(range(len(act)))
        for r in range(self.max_rot):
            ns, hs = be.take(self.nvec, rot), be.take(hn, rot)
            c_rot = c_probe[rot] if r == 0 else be.dot(ns, hs)
            g = be.axpby(np.ones(len(rot)), hs, -c_rot, ns)
            rho = self.norm(g)
            go = [j for j in range(len(rot)) if np.isfinite(rho[j]) and rho[j] > self.rot_tol * max(abs(c_rot[j]), self.c_floor)]
            if not go:
                break
            if len(go) < len(rot):
                ns, hs, g = be.take(ns, go), be.take(hs, go), be.take(g, go)
                rot, c_rot, rho = [rot[j] for j in go], c_rot[go], rho[go]
            theta = be.axpby(1.0 / rho, g)
            ht, _, _, _, widened, failed = be.hvp(be.take(self.x, rot), theta, self.step, f0=be.take(f0, rot))
            self.images[[act[j] for j in rot]] += be.cost(True)
            if widened or failed:
                return hn, rotations, "failed" if failed else "widened"
            ht = self.proj(ht, [qs[j] for j in rot])
            b_rot = 0.5 * (be.dot(theta, hs) + be.dot(ns, ht))
            d_rot = be.dot(theta, ht)
            cs = np.array([_lowest_pair(c_rot[j], b_rot[j], d_rot[j]) if np.isfinite([c_rot[j], b_rot[j], d_rot[j]]).all() else (1.0, 0.0)
                           for j in range(len(rot))])
            ns, hs = be.axpby(cs[:, 0], ns, cs[:, 1], theta), be.axpby(cs[:, 0], hs, cs[:, 1], ht)
            inv = 1.0 / self.norm(ns)
            self.nvec, hn = be.scatter(self.nvec, rot, be.axpby(inv, ns)), be.scatter(hn, rot, be.axpby(inv, hs))
            rotations[rot] += 1
        return hn, rotations, None

    # ---- translation -------------------------------------------------------------------------------------------------------------------
    def new_pairs(self, feff, down):
        """For the rows ``down`` (C < 0) that took an L-BFGS-eligible step last cycle: the pair s = that step, y = (-Feff) - (-Feff then);
        a pair with s.y <= 0 drops the candidate's history instead."""
        be, act = self.be, self.act
        have = [j for j in down if self.prev[act[j]] is not None]
        if not have:
            return
        one = np.ones(len(have))
        s_new = be.cat([self.prev[act[j]][1] for j in have])
        y_new = be.axpby(one, be.cat([self.prev[act[j]][0] for j in have]), -one, be.take(feff, have))
        sy, yy = be.dot(s_new, y_new), be.dot(y_new, y_new)
        for t, j in enumerate(have):
            hist = self.pairs[act[j]]
            if not (np.isfinite(sy[t]) and sy[t] > 0.0 and yy[t] > 0.0):
                hist.clear()
                continue
            hist.append((be.take(s_new, [t]), be.take(y_new, [t]), float(sy[t]), float(yy[t])))
            if len(hist) > self.keep_last:
                hist.pop(0)

    def two_loop(self, feff, down, curv):
        """``lbfgs._two_loop`` on the rows ``down`` of Feff (H is linear, so this is -H (-Feff)), level by level: every level is one batch
        over the candidates that have a pair there, so a cycle reads back a fixed number of K-vectors whatever K."""
        be = self.be
        hists = [self.pairs[self.act[j]] for j in down]
        depth = [len(h) for h in hists]
        q = be.take(feff, down)

        def level(lv):
            """The candidates that have an lv-th newest pair, and that pair's rows: (sub, S, Y, 1 / s.y)."""
            sub = [t for t in range(len(down)) if depth[t] > lv]
            at = [hists[t][-1 - lv] for t in sub]
            return sub, be.cat([p[0] for p in at]), be.cat([p[1] for p in at]), 1.0 / np.array([p[2] for p in at])

        alphas = {}
        for lv in range(max(depth)):                                           # newest pair first
            sub, s_l, y_l, rho_l = level(lv)
            q_l = be.take(q, sub)
            alphas[lv] = rho_l * be.dot(s_l, q_l)
            q = be.scatter(q, sub, be.axpby(np.ones(len(sub)), q_l, -alphas[lv], y_l))
        gamma = np.array([hists[t][-1][2] / hists[t][-1][3] if depth[t] else 1.0 / max(abs(curv[down[t]]), 1.0) for t in range(len(down))])
        q = be.axpby(gamma, q)
        for lv in reversed(range(max(depth))):                                 # oldest pair first
            sub, s_l, y_l, rho_l = level(lv)
            q_l = be.take(q, sub)
            b_l = rho_l * be.dot(y_l, q_l)
            q = be.scatter(q, sub, be.axpby(np.ones(len(sub)), q_l, alphas[lv] - b_l, s_l))
        return q

    def translate(self, force, f0, curv, f_n):
        """The step of every row: L-BFGS on the reflected force while C < 0, a capped step along -(F.n) n otherwise; no component beyond
        ``max_step``.  A candidate whose step is not a number ends here.  ``self.x`` moves; returns nothing."""
        be, act = self.be, self.act
        k = len(act)
        neg = curv < 0.0
        feff = be.axpby(np.where(neg, 1.0, 0.0), force, np.where(neg, -2.0 * f_n, -f_n), self.nvec)
        f_eff_max = be.absmax(feff)
        with np.errstate(divide="ignore", invalid="ignore"):
            up = np.where(f_eff_max > 0.0, self.max_step / f_eff_max, 0.0)
        stp = be.axpby(up, feff)                                               # the step of the rows with C >= 0; the others are replaced below
        down = [j for j in range(k) if neg[j]]
        self.forget([act[j] for j in range(k) if not neg[j]])                  # sign(C) changed, or no history is built
        if down:
            self.new_pairs(feff, down)
            stp = be.scatter(stp, down, self.two_loop(feff, down, curv))
        s_max = be.absmax(stp)
        bad = [j for j in range(k) if not np.isfinite(s_max[j])]
        with np.errstate(divide="ignore", invalid="ignore"):
            cap = np.where(s_max > self.max_step, self.max_step / s_max, 1.0)
        cap[bad] = 0.0
        stp = be.axpby(cap, stp)
        if bad:
            f_host, m_host = be.forces(f0), be.get(self.nvec)
            for j in bad:
                h = self.history[act[j]][-1]
                self.finish(act[j], "non_finite", h["x"], m_host[j], h["energy"], f_host[j], h["curvature"], h["max_force"])
        self.x = be.axpby(np.ones(k), self.x, np.ones(k), stp)
        for j in range(k):
            i = act[j]
            self.history[i][-1]["step_max"] = 0.0 if j in bad else float(min(s_max[j], self.max_step))
            self.prev[i] = (be.take(feff, [j]), be.take(stp, [j])) if neg[j] else None
        if bad:
            self.x, self.nvec = self.keep([j for j in range(k) if j not in bad], self.x, self.nvec)

    # ---- the cycles --------------------------------------------------------------------------------------------------------------------
    def run(self) -> List[SaddleResult]:
        be, na = self.be, self.na
        while self.act:
            act = self.act
            x_host, n_host = be.get(self.x), be.get(self.nvec)
            qs = self.q_blocks(x_host)
            hn, e0, force, f0, widened, failed = be.hvp(self.x, self.nvec, self.step)
            self.images[act] += be.cost(False)
            status = "failed" if failed else "widened" if widened else None
            if status is None:
                force, hn = self.proj(force, qs), self.proj(hn, qs)
                c_probe = be.dot(self.nvec, hn)
                hn, rotations, status = self.rotate(hn, f0, qs, c_probe)
            if status == "failed":
                self.fail_all(x_host, n_host)
                break
            if status == "widened":
                # The engine now runs in the wider arithmetic: the cycle is repeated and the histories (forces of the narrower one) are
                # dropped.  ``images`` counts the products this solver asked for; on the host backend ``Engine.hvp`` has by then repeated
                # the violating call by itself, which is not counted -- after a widening ``images`` is a lower bound of what was spent.
                self.nvec = be.put(n_host)                                     # (a rotation may have turned some rows already)
                self.forget(act)
                continue
            curv = be.dot(self.nvec, hn)
            f_n = be.dot(force, self.nvec)
            f_max = be.absmax(force)
            f_rms = np.sqrt(be.dot(force, force) / self.n)
            finite = np.isfinite(e0) & np.isfinite(curv) & np.isfinite(f_n) & np.isfinite(f_max) & np.isfinite(f_rms)
            with np.errstate(invalid="ignore"):
                conv = finite & (curv < 0.0) & (f_max <= self.max_f) & (f_rms <= self.rms_f)
            stay, leave = [], []
            for j, i in enumerate(act):
                self.cycles[i] += 1
                self.history[i].append(dict(x=x_host[j].reshape(na, 3).copy(), n=n_host[j].reshape(na, 3).copy(), energy=float(e0[j]),
                                            max_force=float(f_max[j]), curv_probe=float(c_probe[j]), curvature=float(curv[j]),
                                            rotations=int(rotations[j]), step_max=0.0))
                reason = "non_finite" if not finite[j] else "converged" if conv[j] else "max_cycles" if self.cycles[i] >= self.max_cycles else None
                (stay if reason is None else leave).append((j, reason))
            if leave:
                rows = [j for j, _ in leave]
                f_host, m_host = be.forces(be.take(f0, rows)), be.get(be.take(self.nvec, rows))
                for t, (j, reason) in enumerate(leave):
                    self.finish(act[j], reason, x_host[j], m_host[t], e0[j], f_host[t], curv[j], f_max[j], f_rms[j])
                if not stay:
                    break
                rows = [j for j, _ in stay]
                self.x, self.nvec, force, f0 = self.keep(rows, self.x, self.nvec, force, f0)
                curv, f_n = curv[rows], f_n[rows]
            self.translate(force, f0, curv, f_n)
        return self.results
