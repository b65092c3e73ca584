"""ASE-style calculator facade -- the reference's secondary boundary for the DMF path.

The reference builds ``FAIRChemCalculator(predictor, task_name=...)`` and assigns it to ``atoms.calc`` of every DMF
image, with ``atoms.info["charge"]`` / ``atoms.info["spin"]`` set per image (reference ``path_opt.py:351-363,418-423``);
torch_dmf then calls ``get_potential_energy()`` / ``get_forces()`` (eV, eV/Angstrom) image by image.  This class offers
the same protocol on the HIP engine, plus ``calculate_images`` which evaluates a whole list of images in one launch.

ASE is not installed here: the class subclasses ``ase.calculators.calculator.Calculator`` when importable and otherwise
is a duck-typed stand-in that works with any object exposing ``get_positions()``, ``get_atomic_numbers()`` (or
``numbers``) and an ``info`` dict.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Sequence

import numpy as np

try:  # pragma: no cover - only where ASE exists
    from ase.calculators.calculator import Calculator as _AseBase, all_changes  # type: ignore

    HAVE_ASE = True
except Exception:
    HAVE_ASE = False
    all_changes = ["positions", "numbers", "cell", "pbc", "initial_charges", "initial_magmoms"]

    class _AseBase:  # minimal protocol
        def __init__(self, **kwargs):
            self.results: Dict[str, Any] = {}
            self.atoms = None

        def get_potential_energy(self, atoms=None, force_consistent=False):
            self.calculate(atoms, ["energy"], all_changes)
            return self.results["energy"]

        def get_forces(self, atoms=None):
            self.calculate(atoms, ["forces"], all_changes)
            return self.results["forces"]

        def get_stress(self, atoms=None):
            self.calculate(atoms, ["stress"], all_changes)
            return self.results["stress"]


try:  # pragma: no cover - only where ASE exists
    from ase.calculators.calculator import PropertyNotImplementedError  # type: ignore
except Exception:
    PropertyNotImplementedError = NotImplementedError


def _numbers(atoms) -> np.ndarray:
    if hasattr(atoms, "get_atomic_numbers"):
        return np.asarray(atoms.get_atomic_numbers(), dtype=np.int32)
    return np.asarray(atoms.numbers, dtype=np.int32)


def _cell_pbc(atoms):
    """(cell bytes, pbc flags) of an image, or None for open boundaries: ``get_cell()`` / ``get_pbc()`` of an ASE ``Atoms``, the
    ``cell`` / ``pbc`` attributes of a duck-typed stand-in; absent attributes, or no periodic axis, mean open boundaries."""
    pbc = atoms.get_pbc() if hasattr(atoms, "get_pbc") else getattr(atoms, "pbc", None)
    cell = atoms.get_cell() if hasattr(atoms, "get_cell") else getattr(atoms, "cell", None)
    if pbc is None or cell is None:
        return None
    flags = np.broadcast_to(np.asarray(pbc, dtype=bool), (3,))
    if not flags.any():
        return None
    c = np.ascontiguousarray(np.asarray(cell, dtype=np.float64).reshape(3, 3))
    return c.tobytes(), tuple(bool(f) for f in flags)


class UMXCalculator(_AseBase):
    """ASE calculator protocol on the MI355X engine (energies eV, forces eV/Angstrom).

    Periodic images: the cell and the pbc flags of the ``Atoms`` reach the engine (``Engine.set_cell``), one cell for all images of a
    ``calculate_images`` call -- or, with ``calculate_images(..., per_image_cells=True)``, every image's own cell
    (``Engine.set_cells``: a variable-cell string, a scan over strained cells), the pbc flags still shared.

    Stress is opt-in: ``UMXCalculator(stress=True)`` adds ``"stress"`` to the INSTANCE's ``implemented_properties`` (the class attribute
    stays energy and forces).  Every evaluation of an image whose three axes are periodic then goes through
    ``Engine.energy_forces_stress`` and caches energy, forces and stress (eV/A^3, Voigt xx, yy, zz, yz, xz, xy, ASE's sign: tensile
    positive), so ``get_potential_energy()``, ``get_forces()`` and ``get_stress()`` on an unchanged image are one evaluation, and ASE's
    cell filters and variable-cell optimisers can drive the calculator.  The stress is the analytic strain derivative with the graph of
    the unstrained geometry held fixed.  An image that is not fully periodic has no volume: energy and forces as before, a request
    for ``"stress"`` raises ``PropertyNotImplementedError`` (``NotImplementedError`` where ASE is absent) -- as does any request for
    it with ``stress=False``.  A single image on a pool of
    engines (``workers > 1``) is evaluated on engine 0 alone when the stress is on, unless ``gp_stress=True``: then it goes graph-parallel
    over the whole pool (``LocalEnginePool.energy_forces_stress(graph_parallel=True)``), every engine adding its share of the strain
    derivative -- for a cell too large for one GPU.

    ``UMXCalculator(double_positions=True)`` hands the float64 positions of the ``Atoms`` to the engine as they are
    (``Engine.energy_forces(..., double_positions=True)``: edge vectors from float64 differences, results independent of where the
    frame sits) in ``calculate`` and ``calculate_images``, with and without stress and per-image cells.  Off by default: positions are
    then rounded to float32 first, as the reference's model input is.  Not together with ``gp_stress`` (``ValueError`` from the pool)."""

    implemented_properties = ["energy", "forces"]

    def __init__(self, model: str = "uma-s-1p1", task_name: str = "omol", device: str = "auto", charge: int = 0, spin: int = 1,
                 radius: Optional[float] = None, max_neigh: Optional[int] = None, workers: int = 1, stress: bool = False, gp_stress: bool = False,
                 double_positions: bool = False, **kwargs):
        """workers > 1 (outside a torch.distributed process group): that many engines in this process when there are that many
        devices (``UMX_LOCAL_DEVICES`` names them), as in ``uma_pysis.UMAcore`` -- ``calculate_images`` deals its images over them,
        a single image is evaluated graph-parallel (``parallel.LocalEnginePool``); ``local_devices`` lists the ordinals in use.
        gp_stress: with ``stress=True`` and such a pool, single-image evaluations take the pool's graph-parallel virial instead of
        engine 0 alone (default off: engine 0, the single-engine stress bit for bit); without a pool it changes nothing."""
        # not an ASE keyword: recompute plans (0 | 1 | 2; None = UMX_RECOMPUTE), as in ``uma_pysis`` (Engine.set_recompute)
        self.recompute = kwargs.pop("recompute", None)
        if self.recompute not in (None, 0, 1, 2):
            raise ValueError(f"recompute must be 0, 1 or 2, got {self.recompute!r}")
        super().__init__(**kwargs)
        self.stress = bool(stress)
        self.gp_stress = bool(gp_stress)
        self.double_positions = bool(double_positions)
        if self.stress:
            self.implemented_properties = ["energy", "forces", "stress"]      # on the instance: the class attribute stays as it is
        self.workers = max(int(workers or 1), 1)
        self.local_devices = None
        self.model, self.task_name, self.device = model, task_name, device
        self.default_charge, self.default_spin = int(charge), int(spin)
        self.radius, self.max_neigh = radius, max_neigh
        self._engine = None
        self._bound = None          # (numbers bytes, charge, spin, (cell bytes, pbc flags) | ("cells", bytes of all cells, pbc flags) | None)
        self._last = None           # (bound key, positions, results) of the most recent single-image evaluation
        if not hasattr(self, "results"):
            self.results = {}

    # ---- engine / system binding ------------------------------------------------------------------
    def _ensure(self, atoms, bind_cell: bool = True):
        """The engine, with the system of ``atoms`` bound and (``bind_cell``) its cell; without, the cell entry of ``_bound`` is the
        caller's to bring up to date."""
        from .engine import Engine
        from . import weights as W
        from .uma_pysis import _device_index, resolve_weights

        z = _numbers(atoms)
        info = getattr(atoms, "info", {}) or {}
        charge, spin = int(info.get("charge", self.default_charge)), int(info.get("spin", self.default_spin))
        if self._engine is None:
            self._weights = resolve_weights(self.model)
            pool_devices = None
            if self.workers > 1:
                from . import parallel as P

                if not P.process_group_active():
                    pool_devices = P.local_devices_for(self.workers)
            if pool_devices is not None:
                self._engine = P.LocalEnginePool.create(pool_devices, self._weights, engine_factory=Engine, recompute=self.recompute)     # same methods as one engine
            else:
                self._engine = Engine(_device_index(self.device))
                self._engine.load_weights(self._weights)
                if self.recompute is not None:
                    self._engine.set_recompute(self.recompute)
            self.local_devices = list(pool_devices) if pool_devices is not None else [_device_index(self.device)]
            from ._host import cap_pools_to_usable_cores

            cap_pools_to_usable_cores()          # the DMF driver's dense linear algebra between two calls must not starve the GPU feeder
        cell = _cell_pbc(atoms)
        key = (z.tobytes(), charge, spin, cell)
        if self._bound is None or key[:3] != self._bound[:3]:
            # merged-MoLE weights depend on (composition, charge, spin, task): refuse to re-bind them to another system
            W.check_merged_for(self._weights, z, charge, spin, self.task_name)
            self._engine.set_system(z, charge=charge, spin=spin, task=self.task_name, radius=self.radius, max_neigh=self.max_neigh)
            self._bound = key[:3] + (None,) if self._bound is None else key[:3] + (self._bound[3],)
        if bind_cell and cell != self._bound[3]:
            # (after set_system: the engine checks the cell against the cutoff that is bound)
            if cell is None:
                self._engine.set_cell(None, None)
            else:
                self._engine.set_cell(np.frombuffer(cell[0], dtype=np.float64).reshape(3, 3), cell[1])
            self._bound = key
        return self._engine

    def close(self) -> None:
        """Release the engine (HBM workspace, weights) now; it is rebuilt lazily on the next calculation."""
        if self._engine is not None:
            self._engine.close()
            self._engine, self._bound, self._last = None, None, None

    # ---- ASE protocol -------------------------------------------------------------------------------
    def calculate(self, atoms=None, properties: Sequence[str] = ("energy", "forces"), system_changes=all_changes):
        if atoms is None:
            atoms = self.atoms
        if atoms is None:
            raise ValueError("no atoms to calculate")
        self.atoms = atoms
        eng = self._ensure(atoms)
        pos = np.array(atoms.get_positions(), dtype=np.float64)
        # get_potential_energy() followed by get_forces() on an unchanged image is ONE evaluation (ASE's own base class caches by atoms
        # state; the stand-in base used where ASE is absent does not, and the engine always computes both)
        with_stress = self.stress and self._fully_periodic()
        if "stress" in properties and not with_stress:
            raise PropertyNotImplementedError(
                "stress: " + ("this calculator was built with stress=False (UMXCalculator(stress=True) turns it on)" if not self.stress
                              else "the image is not periodic along all three axes, so there is no volume to refer a stress to"))
        if self._last is not None and self._last[0] == self._bound and np.array_equal(self._last[1], pos):
            self.results = dict(self._last[2])
            return
        if with_stress:
            e, f, sv = eng.energy_forces_stress(pos[None], **self._stress_kw(), **self._dp_kw())
            self.results = {"energy": float(e[0]), "forces": np.asarray(f[0], dtype=np.float64), "stress": np.asarray(sv[0], dtype=np.float64)}
        else:
            e, f = eng.energy_forces(pos[None], forces=True, **self._dp_kw())
            self.results = {"energy": float(e[0]), "forces": np.asarray(f[0], dtype=np.float64)}
        self._last = (self._bound, pos, dict(self.results))

    def pinned(self, atoms):
        """``with calc.pinned(atoms): ...`` -- the neighbour graph of ``atoms`` (its positions, cell and pbc flags; ``Engine.pin_graph``)
        is pinned for the block and unpinned on the way out, also on an exception: every ``calculate`` / ``calculate_images`` inside --
        the displaced or strained copies of ``atoms`` -- is evaluated on that one edge set.  Images with other pbc flags, or of another
        system, end the pin early (the engine's rules)."""
        from .engine import _Pinned

        eng = self._ensure(atoms)
        self._last = None                # a result cached without the pin is not the pinned one
        return _Pinned(eng, np.array(atoms.get_positions(), dtype=np.float64), self._dp_kw())

    def pinned_each(self, images, per_image_cells: bool = False):
        """``with calc.pinned_each(images): e, f = calc.calculate_images(images)`` -- every image pinned at its own geometry
        (``Engine.pin_graphs``: image k of the calls inside replays the graph of ``images[k]``), all in the cell and pbc flags of the
        first image, and unpinned on the way out, also on an exception.  The references are built in ONE cell: images that differ in
        their cell or flags, and ``per_image_cells=True``, raise ``ValueError`` here, before anything is pinned."""
        from .engine import _Pinned

        if not images:
            raise ValueError("empty image list")
        if per_image_cells:
            raise ValueError("pinned_each: references are built open or in one cell, not under per-image cells (per_image_cells=True)")
        z0, cell0 = _numbers(images[0]), _cell_pbc(images[0])
        for im in images[1:]:
            if not np.array_equal(_numbers(im), z0):
                raise ValueError("all images must share atom order and elements")
            if _cell_pbc(im) != cell0:
                raise ValueError("pinned_each: all images must share the cell and the pbc flags of the first image (the references are built in one cell)")
        eng = self._ensure(images[0])
        self._last = None                # a result cached without the pin is not the pinned one
        refs = np.stack([np.asarray(im.get_positions(), dtype=np.float64) for im in images])
        return _Pinned(eng, refs, self._dp_kw(), "pin_graphs")

    def hvp(self, atoms, vectors, step: float = 1e-3, scheme: str = "central", pin: bool = True, return_curvature: bool = False):
        """Hessian-vector products at ``atoms`` in eV/A^2: ``vectors`` (N,3) or (M,N,3), not normalised -> ``hv`` (M,N,3) float64 per unit
        of ``vectors`` (and ``curv`` (M,), ``v.Hv / v.v``, with ``return_curvature``).  One engine call (``Engine.hvp``): the displaced
        images ``positions +- step * vectors`` (``step`` in A) are formed in float64 on the device and evaluated on the pinned graph of
        ``atoms`` -- its positions, cell and pbc flags -- whatever ``double_positions`` this calculator was built with.  Inside
        ``with calc.pinned(ref)`` the pinned graph of ``ref`` is used instead.  ``scheme``: "central" or "forward"; ``pin=False``: every
        image builds its own graph (for comparison; refused inside ``pinned``)."""
        eng = self._ensure(atoms)
        return eng.hvp(np.array(atoms.get_positions(), dtype=np.float64), np.asarray(vectors, dtype=np.float64), step=float(step), scheme=scheme,
                       pin=pin, return_curvature=return_curvature)

    def lowest_modes(self, atoms, k: int = 1, frozen=(), **kw):
        """The ``k`` lowest vibrational modes at ``atoms`` without a Hessian (``Engine.lowest_modes`` / ``LocalEnginePool.lowest_modes``;
        ``modes.lowest_modes`` documents the keywords and the :class:`modes.ModesResult` returned, eV/A^2/amu and cm^-1): masses from
        ``atoms.get_masses()``, the graph, cell and pbc flags of ``atoms``; ``frozen``: atom indices held fixed.  Inside
        ``with calc.pinned(ref)`` the pinned graph of ``ref`` is used and left in place."""
        eng = self._ensure(atoms)
        return eng.lowest_modes(np.array(atoms.get_positions(), dtype=np.float64), np.asarray(atoms.get_masses(), dtype=np.float64), int(k),
                                frozen=frozen, **kw)

    def refine_saddle(self, atoms, mode=None, frozen=(), **kw):
        """Refine the transition-state guess ``atoms`` to a first-order saddle without a Hessian (``Engine.refine_saddles`` /
        ``LocalEnginePool.refine_saddles``; ``dimer.refine_saddles`` documents the keywords): ``mode`` (N,3) the start direction (None: the
        lowest mode), ``frozen`` atom indices held fixed, the cell and pbc flags of ``atoms``; ``verify=True`` takes its masses from
        ``atoms.get_masses()``.  Returns ``(new atoms, dimer.SaddleResult)``: a copy of ``atoms`` at the refined positions (eV, A)."""
        eng = self._ensure(atoms)
        if kw.get("verify") and kw.get("masses") is None:
            kw["masses"] = np.asarray(atoms.get_masses(), dtype=np.float64)
        res = eng.refine_saddles(np.array(atoms.get_positions(), dtype=np.float64), mode, frozen=frozen, **kw)[0]
        new = atoms.copy()
        new.set_positions(res.x)
        return new, res

    def _stress_kw(self) -> dict:
        """What ``energy_forces_stress`` is called with: the graph-parallel opt-in when this calculator runs a pool of engines."""
        return {"graph_parallel": True} if self.gp_stress and len(self.local_devices or []) > 1 else {}

    def _dp_kw(self) -> dict:
        """``double_positions=True`` for the engine when this calculator was built with it; nothing otherwise (the calls as they were)."""
        return {"double_positions": True} if self.double_positions else {}

    def _fully_periodic(self) -> bool:
        """The image bound last has a cell and all three pbc flags set."""
        return self._bound is not None and self._bound[3] is not None and all(self._bound[3][-1])

    def _bind_image_cells(self, eng, images) -> None:
        """Every image's own cell to ``Engine.set_cells``.  ``_bound`` then names the set of cells, which no single image's cell equals:
        the next ``calculate()`` binds its cell again, and the single-image cache is dropped."""
        cps = [_cell_pbc(im) for im in images]
        if any(cp is None for cp in cps):
            raise ValueError("per_image_cells: every image needs a cell and at least one periodic axis")
        if any(cp[1] != cps[0][1] for cp in cps):
            raise ValueError("per_image_cells: all images must share the pbc flags of the first image (one set of flags per call)")
        mark = ("cells", b"".join(cp[0] for cp in cps), cps[0][1])
        if mark != self._bound[3]:
            eng.set_cells(np.frombuffer(mark[1], dtype=np.float64).reshape(len(images), 3, 3), mark[2])
            self._bound = self._bound[:3] + (mark,)
        self._last = None

    def calculate_images(self, images: Sequence[Any], stress: bool = False, per_image_cells: bool = False):
        """One batched evaluation for a list of images of the SAME system; returns (E [K] eV, F [K,N,3] eV/A), and with ``stress=True``
        (E, F, stress [K,6] eV/A^3 in Voigt order) -- for images that are periodic along all three axes, whatever the constructor's
        ``stress`` says; ``PropertyNotImplementedError`` otherwise.  All images share the cell of the first one (``ValueError``
        otherwise) unless ``per_image_cells=True``: then image k is evaluated in its own cell, and its stress refers to its own volume;
        the images must all have a cell and agree in their pbc flags (``ValueError``)."""
        if not images:
            raise ValueError("empty image list")
        eng = self._ensure(images[0], bind_cell=not per_image_cells)
        z0 = _numbers(images[0])
        for im in images[1:]:
            if not np.array_equal(_numbers(im), z0):
                raise ValueError("all images must share atom order and elements")
            if not per_image_cells and _cell_pbc(im) != self._bound[3]:
                raise ValueError("all images must share the cell and the pbc flags of the first image (one cell per call)")
        if per_image_cells:
            self._bind_image_cells(eng, images)
        pos = np.stack([np.asarray(im.get_positions(), dtype=np.float64) for im in images])
        if stress:
            if not self._fully_periodic():
                raise PropertyNotImplementedError("stress: the images are not periodic along all three axes, so there is no volume to refer a stress to")
            e, f, sv = eng.energy_forces_stress(pos, **self._stress_kw(), **self._dp_kw())
            return e, np.asarray(f, dtype=np.float64), np.asarray(sv, dtype=np.float64)
        e, f = eng.energy_forces(pos, forces=True, **self._dp_kw())
        return e, np.asarray(f, dtype=np.float64)
