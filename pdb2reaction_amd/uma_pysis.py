"""UMA calculator for pysisyphus -- MI355X-native drop-in for ``pdb2reaction.uma_pysis``.

Mirrors the reference interface (reference ``pdb2reaction/uma_pysis.py``):

* ``CALC_KW`` / ``GEOM_KW_DEFAULT`` (``:132-165``), unit constants (``:127-129``);
* ``UMAcore`` (``:170-419``): ``compute(coord_ang, forces=, hessian=)`` -> eV, eV/A;
* ``uma_pysis(Calculator)`` (``:425-780``): ``get_energy / get_forces / get_hessian(elem, coords)``
  with coordinates in Bohr, results in Hartree, Hartree/Bohr, Hartree/Bohr^2, frozen-atom force
  zeroing (``:561-567``), finite-difference Hessian (``:595-686``), Hessian symmetrisation / unit
  conversion / dtype (``:515-551``), mode dispatch (``:708-780``);
* ``run_pysis`` (``:784-789``).

What differs underneath: ``predict_unit.predict(batch)`` (fairchem, ``:373,385``) is replaced by the
HIP engine (``libumx.so``), and two batched entry points are added so a string driver can evaluate
all images at once: ``UMAcore.compute_batch`` and ``uma_pysis.get_forces_batch``.  The FD Hessian
uses the batched path (the 2*3N_active displaced geometries are images of one batch) but keeps the
reference's arithmetic: float32 forces, central difference with h = 1e-3 A, columns assembled in
float64 when ``hessian_double``.

Own keywords, taken out of ``**kwargs`` so that the reference's signature stays: ``precision``, ``recompute``,
``double_positions``, ``hessian_pin_graph``, and ``cell`` (3,3, Angstrom) / ``pbc`` -- ONE fixed periodic cell, bound on
the engine after the system (``Engine.set_cell``), in which every energy, force and Hessian is then evaluated
(``uma_pysis.set_cell`` re-binds it).  The reference never sets a cell (``:292-327``).

There is no CPU fallback: importing works anywhere, evaluating requires a gfx950 GPU and the built
library, and fails loudly otherwise.
"""
from __future__ import annotations

import os
from typing import Any, Dict, List, Mapping, Optional, Sequence

import numpy as np

from ._calculator_base import ANG2BOHR, AU2EV, BOHR2ANG, Calculator  # noqa: F401
from . import hessian as H
from ._host import cap_pools_to_usable_cores
from . import synth
from . import weights as W

# ------------ unit conversion constants (reference uma_pysis.py:127-129) ----------------------
EV2AU = H.EV_TO_HARTREE                   # eV -> Hartree
F_EVAA_2_AU = H.EV_PER_ANG_TO_AU          # eV/A -> Hartree/Bohr
H_EVAA_2_AU = H.EV_PER_ANG2_TO_AU         # eV/A^2 -> Hartree/Bohr^2

# reference uma_pysis.py:132-135
GEOM_KW_DEFAULT: Dict[str, Any] = {
    "coord_type": "cart",
    "freeze_atoms": [],
}

# reference uma_pysis.py:138-165
CALC_KW: Dict[str, Any] = {
    "charge": 0,
    "spin": 1,
    "model": "uma-s-1p1",
    "task_name": "omol",
    "device": "auto",
    "workers": 1,
    "workers_per_node": 1,
    "max_neigh": None,
    "radius": None,
    "r_edges": False,
    "out_hess_torch": True,
    "freeze_atoms": None,
    "hessian_calc_mode": "FiniteDifference",
    "return_partial_hessian": False,
    "hessian_double": True,
}

PIN_NOT_GP = ("hessian_pin_graph=True cannot be combined with the graph-parallel mode (workers == world size / enable_graph_parallel): its "
              "entries (umx_gp_begin) build their own graph and refuse a pinned engine")
HVP_NOT_GP = ("get_hvp cannot be combined with the graph-parallel mode (workers == world size / enable_graph_parallel): Hessian-vector "
              "products need the pinned graph, and the graph-parallel entries (umx_gp_begin) build their own")
MODES_NOT_GP = ("get_lowest_modes cannot be combined with the graph-parallel mode (workers == world size / enable_graph_parallel): its "
                "Hessian-vector products need the pinned graph, and the graph-parallel entries (umx_gp_begin) build their own")
TS_NOT_GP = ("get_ts cannot be combined with the graph-parallel mode (workers == world size / enable_graph_parallel): its "
             "Hessian-vector products need the pinned graph, and the graph-parallel entries (umx_gp_begin) build their own")

# number of displaced geometries evaluated per engine call while building an FD Hessian
FD_BATCH = int(os.environ.get("UMX_FD_BATCH", "64"))


def resolve_weights(model: str) -> "W.WeightSet":
    """Map the reference's ``model`` keyword to a UMA-S parameter set.

    * a path to a ``.umxw`` blob -> loaded as is, merged for one system or in EXPERT FORM (``checkpoint.convert_experts``: one file
      for every system, the engine merges the experts on the GPU when a system is bound);
    * a path to a checkpoint file (anything else that exists) -> ``torch.load(map_location="cpu", weights_only=True)`` and
      ``checkpoint.convert_checkpoint_experts``: model config, state dict, normaliser and element references are taken from the
      mapping as ``checkpoint.convert`` demands them; a file that does not unpickle under ``weights_only=True`` raises with that
      reason (key names [3P-UNVERIFIED], like the rest of the loader);
    * a model name -> ``$UMX_WEIGHTS_DIR/<name>.umxw``, else ``$UMX_WEIGHTS_DIR/<name>.pt`` (a checkpoint file, as above);
    * ``"synthetic"`` / ``"synthetic:<seed>"`` -> the deterministic stand-in of ``weights.make_synthetic_weights``
      (what tests and bench.py use: the real checkpoint is a gated download that does not exist here);
    * anything else raises ``FileNotFoundError`` -- like the reference, which raises when the checkpoint cannot be
      obtained (``uma_pysis.py:246-250``).  A calculator must never hand out energies of random weights unasked;
      ``UMX_ALLOW_SYNTHETIC=1`` turns the miss into the synthetic stand-in (with a warning) for plumbing runs.
    """
    m = str(model)
    if m == "synthetic" or m.startswith("synthetic:"):
        return W.make_synthetic_weights(int(m.split(":", 1)[1]) if ":" in m else int(os.environ.get("UMX_SYNTHETIC_SEED", "0")))
    if os.path.isfile(m):
        return _load_weight_file(m)
    wdir = os.environ.get("UMX_WEIGHTS_DIR")
    cand = os.path.join(wdir, f"{m}.umxw") if wdir else None
    if cand and os.path.isfile(cand):
        return W.load_weights(cand)
    if wdir and os.path.isfile(os.path.join(wdir, f"{m}.pt")):
        return _load_weight_file(os.path.join(wdir, f"{m}.pt"))
    if os.environ.get("UMX_ALLOW_SYNTHETIC", "0") == "1":
        import warnings

        warnings.warn(f"model {m!r}: no weight blob found, UMX_ALLOW_SYNTHETIC=1 -> RANDOM synthetic weights; energies and "
                      "forces are physically meaningless", RuntimeWarning, stacklevel=2)
        return W.make_synthetic_weights(int(os.environ.get("UMX_SYNTHETIC_SEED", "0")))
    where = cand if cand else f"$UMX_WEIGHTS_DIR/{m}.umxw (UMX_WEIGHTS_DIR is not set)"
    raise FileNotFoundError(
        f"UMA weights for model {m!r} not found: expected {where}, or pass model=<path to a .umxw blob> "
        "(convert a fairchem checkpoint with pdb2reaction_amd.checkpoint.convert). "
        "Use model='synthetic' or UMX_ALLOW_SYNTHETIC=1 only for tests and benchmarks.")


def _load_weight_file(path: str) -> "W.WeightSet":
    """A ``.umxw`` blob (by its magic) as it is; any other file as a checkpoint -> expert-form weight set."""
    with open(path, "rb") as f:
        magic = f.read(len(W.MAGIC))
    if magic == W.MAGIC:
        return W.load_weights(path)
    import torch

    from . import checkpoint as CK

    try:
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as exc:
        raise CK.UnsupportedCheckpoint(f"{path}: not a .umxw blob, and torch.load(weights_only=True) does not read it as a checkpoint: {exc}") from exc
    if not isinstance(ckpt, Mapping):
        raise CK.UnsupportedCheckpoint(f"{path}: the checkpoint is a {type(ckpt).__name__}, not a mapping with a model config and a state dict")
    return W.unpack_blob(CK.convert_checkpoint_experts(ckpt))


def _device_index(device: str) -> int:
    """'auto' | 'cuda' | 'cuda:N' -> HIP ordinal; 'cpu' is refused (no CPU path exists)."""
    d = str(device).lower()
    if d == "cpu":
        raise RuntimeError("device='cpu' requested, but this calculator has no CPU path; it requires an MI355X (gfx950) GPU.")
    if d in ("auto", "cuda", "hip", "gpu"):
        return int(os.environ.get("LOCAL_RANK", "0")) if d == "auto" and "LOCAL_RANK" in os.environ else 0
    if ":" in d:
        return int(d.split(":", 1)[1])
    raise ValueError(f"unrecognised device {device!r}")


# ===================================================================
#                         UMA core wrapper
# ===================================================================
class UMAcore:
    """Thin wrapper around the HIP engine (counterpart of reference ``UMAcore``, ``:170-419``)."""

    def __init__(
        self,
        elem: Sequence[str],
        *,
        charge: int = 0,
        spin: int = 1,
        model: str = "uma-s-1p1",
        task_name: str = "omol",
        device: str = "auto",
        workers: int = 1,
        workers_per_node: int = 1,
        max_neigh: Optional[int] = None,
        radius: Optional[float] = None,
        r_edges: bool = False,
        precision: Optional[str] = None,
        recompute: Optional[int] = None,
        double_positions: bool = False,
        cell=None,
        pbc=None,
    ):
        from .engine import Engine  # raises ImportError loudly when libumx.so is missing

        self.device_str = device
        self.workers = max(int(workers) if workers is not None else 1, 1)
        self.workers_per_node = max(int(workers_per_node) if workers_per_node is not None else 1, 1)
        # The reference's workers>1 is graph-parallel inference of ONE image (ParallelMLIPPredictUnit,
        # :220-242).  Here images are the parallel unit (one engine per GPU, see parallel.py).  Outside a process
        # group `workers=G` builds G engines in THIS process when there are G devices to put them on
        # (parallel.LocalEnginePool; UMX_LOCAL_DEVICES names them); otherwise it only keeps the reference's side
        # effect: no analytical Hessian.
        self.parallel_predict = self.workers > 1
        self.has_torch_model = False       # no nn.Module is exposed -> analytical Hessian unavailable
        self.elem = [e.capitalize() for e in elem]
        self.charge = charge
        self.spin = spin
        self.task_name = task_name
        self._max_neigh_user = max_neigh
        self._radius_user = radius
        self._r_edges_user = r_edges
        # False: positions are rounded to float32 before the engine sees them (the reference's AtomicData.pos, :312-322).  True: the float64
        # geometry goes through (Engine.energy_forces(double_positions=True)): edge vectors from float64 differences
        self.double_positions = bool(double_positions)

        weights = resolve_weights(model)                    # raises FileNotFoundError before any GPU work
        # graph defaults come from the MODEL, as in the reference (backbone.cutoff / backbone.max_neighbors, fallback 6.0 A;
        # uma_pysis.py:301-309): a converted checkpoint records them in the blob trailer (checkpoint.validate_model_config)
        model_rec = (getattr(weights, "meta", None) or {}).get("model") or {}
        if radius is None and model_rec.get("cutoff") is not None:
            radius = float(model_rec["cutoff"])
        if max_neigh is None and model_rec.get("max_neighbors") is not None:
            max_neigh = int(model_rec["max_neighbors"])
        self.model_record = dict(model_rec)
        if r_edges:
            import warnings
            warnings.warn("uma_pysis: r_edges=True has no effect here: the radius graph is always built on the device for every call "
                          "(the reference collates with otf_graph=True as well, uma_pysis.py:322, so pre-computed edges are not what its model uses)",
                          RuntimeWarning, stacklevel=3)
        if self.workers_per_node != 1:
            import warnings
            warnings.warn(f"uma_pysis: workers_per_node={self.workers_per_node} has no effect here: there are no Ray actors to place "
                          "(uma_pysis.py:228-242); under torch.distributed the launcher decides which rank runs on which node",
                          RuntimeWarning, stacklevel=3)
        self.z = synth.symbols_to_z(self.elem)
        W.check_merged_for(weights, self.z, charge, spin, task_name)   # a MoLE merge is valid for one system only
        self._pool = None
        pool_devices = None
        if self.workers > 1:
            from . import parallel as P

            if not P.process_group_active():
                pool_devices = P.local_devices_for(self.workers)          # ValueError: UMX_LOCAL_DEVICES and workers disagree
        if pool_devices is not None:
            # `workers` engines in this process (ordinals may repeat: "0,0" rehearses the path on one GPU); engine 0 is `self.engine`
            self._pool = P.LocalEnginePool.create(pool_devices, weights, precision=precision, engine_factory=Engine, recompute=recompute)
            self.engine = self._pool.engines[0]
            cap_pools_to_usable_cores()
            self._pool.set_system(self.z, charge=charge, spin=spin, task=task_name, radius=radius, max_neigh=max_neigh)
        else:
            dev_index = _device_index(device)
            self.engine = Engine(dev_index, precision=precision)     # None: UMX_PRECISION (default "auto")
            if recompute is not None:                                 # None: UMX_RECOMPUTE (default 0)
                self.engine.set_recompute(recompute)
            cap_pools_to_usable_cores()                       # BLAS pools sized for the machine inside a CPU-quota container starve the GPU feeder
            self.engine.load_weights(weights)
            self.engine.set_system(self.z, charge=charge, spin=spin, task=task_name, radius=radius, max_neigh=max_neigh)
        self.local_devices = list(pool_devices) if pool_devices is not None else [dev_index]   # ordinals in use by this core
        if cell is not None:                              # one periodic cell (A) for every geometry of this core, bound after the system
            self.set_cell(cell, pbc)
        self._gp = None
        if self.workers > 1 and os.environ.get("UMX_WORKERS_GP", "1") != "0":
            # the reference's workers > 1 IS graph-parallel inference of one structure over `workers` processes
            # (ParallelMLIPPredictUnit, :220-242).  Under torch.distributed with one rank per GPU and a world of exactly that
            # many ranks the same thing happens here: the graph of every geometry is partitioned over the ranks -- which is also
            # the route for a single structure too large for one GPU's workspace (UMX_ERR_CAPACITY).  Every rank must then call
            # the calculator with the same coordinates (SPMD), as every rank of such a job runs the same driver.
            import torch.distributed as dist

            if dist.is_available() and dist.is_initialized() and dist.get_world_size() == self.workers:
                self.enable_graph_parallel(True)

    @property
    def device(self):
        import torch
        return torch.device("cuda", self.engine.device)

    def close(self) -> None:
        """Release every engine of this core (the pool's, or the one)."""
        if getattr(self, "_pool", None) is not None:
            self._pool.close()
        else:
            self.engine.close()

    def reserve_images(self, n_images: int) -> None:
        (self._pool if self._pool is not None else self.engine).reserve_images(int(n_images))

    def set_cell(self, cell=None, pbc=None) -> None:
        """``Engine.set_cell`` (cell (3,3) in A, pbc a bool or three flags; None: open boundaries) on the engine, or on every engine of
        an in-process pool.  It persists: every later ``compute`` / ``compute_batch`` / ``compute_batch_dev``, the graph-parallel mode
        included (``umx_gp_begin`` honours the bound cell), evaluates in that cell."""
        (self._pool if getattr(self, "_pool", None) is not None else self.engine).set_cell(cell, pbc)

    def enable_graph_parallel(self, on: bool = True, group=None) -> None:
        """Evaluate every geometry with its GRAPH partitioned over the ranks of `group` (default: the world) -- the reference's
        ``workers > 1`` mode (``ParallelMLIPPredictUnit``, ``:220-242``), for single large structures when there are fewer images
        than GPUs.  From then on ``compute`` / ``compute_batch`` are COLLECTIVES: every rank must call them with the same
        coordinates.  Images stay the preferred unit of parallelism (``parallel.ShardedImageEvaluator``): this mode moves
        9 x N x 4.6 KB through all-reduces per evaluation."""
        if not on:
            self._gp = None
            return
        if getattr(self, "double_positions", False):
            raise ValueError("enable_graph_parallel: double_positions=True cannot be combined with the graph-parallel mode -- its entry "
                             "(umx_gp_begin) takes float32 positions only")
        if self._pool is not None:
            raise RuntimeError("enable_graph_parallel: this core evaluates on an in-process pool of engines (workers > 1 without a process "
                               "group); the rank-level graph-parallel mode needs one engine per rank")
        from .parallel import GraphParallelEvaluator

        self._gp = GraphParallelEvaluator(self.engine, len(self.z), self.device, group)

    def _gp_eval(self, coords_ang: np.ndarray):
        import torch

        c = np.asarray(coords_ang, dtype=np.float64).reshape(-1, len(self.z), 3)
        es, fs = [], []
        for k in range(c.shape[0]):                       # images one after another, each spread over all ranks
            if not np.isfinite(c[k]).all():
                raise ValueError(f"non-finite position in image {k}")
            e, f = self._gp(torch.as_tensor(c[k], dtype=torch.float32, device=self.device))
            es.append(float(e[0]))
            if not np.isfinite(es[-1]):
                # the device-pointer entries are asynchronous and cannot refuse the result themselves (include/umx.h, UMX_ERR_RANGE);
                # every rank sees the same energy, so every rank raises here
                raise RuntimeError(f"image {k}: non-finite energy in graph-parallel mode (an activation beyond the fp16 operand range of "
                                   "UMX_PRECISION=split? create the calculators with UMX_PRECISION=split-bf16)")
            fs.append(f.cpu().numpy())
        return np.asarray(es, dtype=np.float64), np.stack(fs)

    # ----------------------------------------------------------------
    def compute_batch(self, coords_ang: np.ndarray, *, forces: bool = True) -> Dict[str, Any]:
        """Batched evaluation: (K,N,3) A -> {"energy": (K,) float64 eV, "forces": (K,N,3) float32 eV/A}."""
        if getattr(self, "_gp", None) is not None:
            e, f = self._gp_eval(coords_ang)
            return {"energy": e, "forces": f if forces else None}
        e, f = (getattr(self, "_pool", None) or self.engine).energy_forces(np.asarray(coords_ang), forces=forces, **self._dp_kw())
        return {"energy": e, "forces": f}

    def _dp_kw(self) -> dict:
        """``double_positions=True`` for the engine (or pool) when this core was built with it; nothing otherwise (the calls as they were)."""
        return {"double_positions": True} if getattr(self, "double_positions", False) else {}

    def compute_batch_dev(self, pos32):
        """Device form of :meth:`compute_batch` for loops that stay on the GPU (the batched FD Hessian): ``pos32`` torch float32 [K,N,3] on
        the engine's device -> forces torch float32 [K,N,3] on the same device, through the engine's device-pointer entry on torch's
        current stream.  That entry is asynchronous and cannot refuse a non-finite energy itself, so the energies are looked at here (one
        scalar read per call); a range violation of the fast split-f16 mode widens the engine and repeats the call, as the host entry does.
        A core built with ``double_positions=True`` takes a torch float64 tensor instead (``umx_energy_forces_f64_dev``).  The pointer
        entry cannot see the type behind its pointer, so the tensor's dtype is held to the flag here: ``TypeError`` otherwise."""
        import torch

        dp = self._dp_kw()
        want = torch.float64 if dp else torch.float32
        if pos32.dtype != want:
            raise TypeError(f"compute_batch_dev: positions are {pos32.dtype}, this core takes {want} "
                            f"(double_positions={bool(dp)})")
        k = int(pos32.shape[0])
        pos32 = pos32.contiguous()
        e = torch.empty(k, dtype=torch.float64, device=pos32.device)
        f = torch.empty(k, pos32.shape[1], 3, dtype=torch.float32, device=pos32.device)
        for attempt in range(2):
            self.engine.energy_forces_dev(k, pos32.data_ptr(), e.data_ptr(), f.data_ptr(), stream=torch.cuda.current_stream(pos32.device).cuda_stream, **dp)
            if bool(torch.isfinite(e).all()):
                return f
            self.engine.take_range_error()
            if attempt == 0 and self.engine.widen("non-finite energy in a device-resident batch"):
                continue
            raise RuntimeError(f"non-finite energy in a device-resident batch (precision mode {self.engine.precision_mode()}): non-finite "
                               "coordinates, or an overflow that wider forward planes cannot cure")
        return f

    def hvp(self, coord_ang: np.ndarray, vectors: np.ndarray, *, step: float = 1e-3, scheme: str = "central", base_of=None) -> np.ndarray:
        """Hessian-vector products of the FULL Hessian: ``coord_ang`` (N,3) or (R,N,3) A, ``vectors`` (M,N,3) -> (M,N,3) float64 eV/A^2
        per unit of ``vectors``, through ``Engine.hvp`` (or the pool's): displaced images formed in float64 on the device, evaluated on
        the pinned graph of their base in one batched call.  The graph-parallel mode has no such entry: ``ValueError``."""
        if getattr(self, "_gp", None) is not None:
            raise ValueError(HVP_NOT_GP)
        n = len(self.z)
        return (getattr(self, "_pool", None) or self.engine).hvp(np.asarray(coord_ang, dtype=np.float64).reshape(-1, n, 3),
                                                                 np.asarray(vectors, dtype=np.float64).reshape(-1, n, 3), base_of,
                                                                 step=float(step), scheme=scheme)

    def lowest_modes(self, coord_ang: np.ndarray, masses_amu, k: int = 1, **kw):
        """The ``k`` lowest eigenpairs of the mass-weighted, projected Hessian at ``coord_ang`` (N,3) A without a Hessian
        (``modes.lowest_modes``: keywords and the ``ModesResult`` returned, in eV/A^2/amu): on the engine with every vector on the
        device, or over the in-process pool.  The graph-parallel mode has no such entry: ``ValueError``."""
        if getattr(self, "_gp", None) is not None:
            raise ValueError(MODES_NOT_GP)
        return (getattr(self, "_pool", None) or self.engine).lowest_modes(np.asarray(coord_ang, dtype=np.float64).reshape(len(self.z), 3),
                                                                          masses_amu, int(k), **kw)

    def refine_saddles(self, coord_ang: np.ndarray, modes0=None, **kw):
        """Refine transition-state guesses ``coord_ang`` (N,3) or (K,N,3) A to first-order saddles without a Hessian
        (``dimer.refine_saddles``: keywords and the ``SaddleResult`` list returned, in eV and A): on the engine with every vector on the
        device, or over the in-process pool.  The graph-parallel mode has no such entry: ``ValueError``."""
        if getattr(self, "_gp", None) is not None:
            raise ValueError(TS_NOT_GP)
        return (getattr(self, "_pool", None) or self.engine).refine_saddles(np.asarray(coord_ang, dtype=np.float64).reshape(-1, len(self.z), 3),
                                                                            modes0, **kw)

    def compute(self, coord_ang: np.ndarray, *, forces: bool = False, hessian: bool = False) -> Dict[str, Any]:
        """Energy (eV) and optionally forces (eV/A) of one geometry; same contract as reference ``:330-419``."""
        if hessian:
            raise RuntimeError(
                "Analytical Hessian is not available when predictor workers > 1 "
                "or when predictor.model is not exposed. Use FiniteDifference Hessian."
            )
        if getattr(self, "_gp", None) is not None:
            e, f = self._gp_eval(coord_ang)
        else:
            e, f = (getattr(self, "_pool", None) or self.engine).energy_forces(np.asarray(coord_ang, dtype=np.float64).reshape(1, -1, 3), forces=forces,
                                                                               **self._dp_kw())
        return {"energy": float(e[0]), "forces": (f[0] if forces else None), "hessian": None}


# ===================================================================
#                    PySisyphus calculator class
# ===================================================================
class uma_pysis(Calculator):
    """PySisyphus-compatible UMA calculator (counterpart of reference ``:425-780``)."""

    implemented_properties = ["energy", "forces", "hessian"]

    def __init__(
        self,
        *,
        charge: int = CALC_KW["charge"],
        spin: int = CALC_KW["spin"],
        model: str = CALC_KW["model"],
        task_name: str = CALC_KW["task_name"],
        device: str = CALC_KW["device"],
        workers: int = CALC_KW["workers"],
        workers_per_node: int = CALC_KW["workers_per_node"],
        out_hess_torch: bool = CALC_KW["out_hess_torch"],
        max_neigh: Optional[int] = CALC_KW["max_neigh"],
        radius: Optional[float] = CALC_KW["radius"],
        r_edges: bool = CALC_KW["r_edges"],
        freeze_atoms: Optional[Sequence[int]] = CALC_KW["freeze_atoms"],
        hessian_calc_mode: str = CALC_KW["hessian_calc_mode"],
        return_partial_hessian: bool = CALC_KW["return_partial_hessian"],
        hessian_double: bool = CALC_KW["hessian_double"],
        **kwargs,
    ):
        # not a reference keyword: the arithmetic of the large GEMMs ("auto" | "split" | "split-bf16" | "bf16x3" | "fp32"; None = UMX_PRECISION).
        # Taken out of **kwargs so that the reference's signature stays as it is.
        precision = kwargs.pop("precision", None)
        if precision not in (None, "auto", "split", "split-f16", "split-bf16", "bf16x3", "split-exact", "fp32"):
            raise ValueError(f"precision must be auto, split, split-bf16, bf16x3 or fp32, got {precision!r}")
        # likewise: recompute plans (0 off | 1 when the stored plans do not fit the workspace | 2 always; None = UMX_RECOMPUTE) -- one
        # image of any size on one GPU, at the price of one more forward edge pipeline (Engine.set_recompute)
        recompute = kwargs.pop("recompute", None)
        if recompute not in (None, 0, 1, 2):
            raise ValueError(f"recompute must be 0, 1 or 2, got {recompute!r}")
        # likewise: False (default) keeps the reference's float32 positions (AtomicData.pos, :312-322); True passes the float64 geometry
        # through get_energy / get_forces / get_forces_batch / get_hessian to the engine (edge vectors from float64 differences, FD
        # displacements realised in float64).  Not with the graph-parallel mode.
        self.double_positions = bool(kwargs.pop("double_positions", False))
        # likewise: True makes get_hessian pin the neighbour graph of the geometry it was given (Engine.pin_graph) for the displaced images
        # of the finite-difference Hessian, so that no column differences across a change of the edge set (an edge entering or leaving
        # through max_neigh) -- the graph held fixed is what the reference's "Analytical" mode differentiates (:394-417).  Not with the
        # graph-parallel mode, whose entries build their own graph.
        self.hessian_pin_graph = bool(kwargs.pop("hessian_pin_graph", False))
        # likewise: one periodic cell for every geometry this calculator sees -- cell (3,3) lattice vectors as rows in ANGSTROM (the unit of
        # Engine.set_cell and of ASE, not the Bohr of the coordinates), pbc a bool or three flags.  Bound on the engine right after the
        # system; everything behind it (energies, forces, batches, the FD Hessian with or without hessian_pin_graph / double_positions) is
        # the engine with that cell.  The reference never sets a cell (:292-327).
        self.cell, self.pbc = _cell_and_flags(kwargs.pop("cell", None), kwargs.pop("pbc", None))
        super().__init__(charge=charge, mult=spin, **kwargs)
        self._core: Optional[UMAcore] = None
        self._core_kw = dict(
            charge=charge, spin=spin, model=model, task_name=task_name, device=device, workers=workers,
            workers_per_node=workers_per_node, max_neigh=max_neigh, radius=radius, r_edges=r_edges, precision=precision,
            recompute=recompute,
        )
        if self.double_positions:                 # (only then: a stand-in core keeps the reference's signature)
            self._core_kw["double_positions"] = True
        if self.cell is not None:                 # (likewise)
            self._core_kw.update(cell=self.cell, pbc=self.pbc)
        self._reserve_images = 0
        self.out_hess_torch = out_hess_torch
        self.hessian_calc_mode = hessian_calc_mode
        self.freeze_atoms: List[int] = sorted(set(int(i) for i in (freeze_atoms or [])))
        self.return_partial_hessian = bool(return_partial_hessian)
        self.hessian_double = bool(hessian_double)
        # multi-GPU FD Hessian is opt-in (enable_hessian_sharding): a collective must never start implicitly
        self._hess_shard = False
        self._hess_group = None

    # ---------- internals -------------------------------------------
    def _ensure_core(self, elem: Sequence[str]):
        # the first `elem` binds the instance for its lifetime, as in the reference (:502-504)
        if self._core is None:
            self._core = UMAcore(elem, **self._core_kw)
            if self._reserve_images and hasattr(self._core, "engine"):
                self._core.reserve_images(self._reserve_images)
        return self._core

    def reserve_images(self, n_images: int) -> None:
        """Tell the engine that batches of up to ``n_images`` images are coming (a string that will grow to that size): its workspace is
        then allocated once instead of being re-allocated at every growth -- seconds each (``umx_reserve_images``).  A hint only."""
        self._reserve_images = max(0, int(n_images))
        if getattr(self._core, "engine", None) is not None:
            (self._core if hasattr(self._core, "reserve_images") else self._core.engine).reserve_images(self._reserve_images)

    def set_cell(self, cell=None, pbc=None) -> None:
        """Bind another cell (A; ``None`` or no flag set: open boundaries) without rebuilding the core: weights, system and workspace
        stay, the next call evaluates in the new cell.  Before the first call it only changes what the core will be built with."""
        self.cell, self.pbc = _cell_and_flags(cell, pbc)
        for key in ("cell", "pbc"):
            self._core_kw.pop(key, None)
        if self.cell is not None:
            self._core_kw.update(cell=self.cell, pbc=self.pbc)
        if self._core is not None:
            self._core.set_cell(self.cell, self.pbc)

    def close(self) -> None:
        """Release the engine (HBM workspace, weights) now instead of at garbage collection; the calculator can be used
        again afterwards (the core is rebuilt lazily on the next call)."""
        if self._core is not None:
            eng = getattr(self._core, "engine", None)
            if hasattr(self._core, "close"):
                self._core.close()                        # every engine of an in-process pool
            elif eng is not None:
                eng.close()
            self._core = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def enable_graph_parallel(self, elem: Sequence[str], on: bool = True, group=None) -> None:
        """Reference ``workers > 1`` semantics on the engine: partition the graph of each geometry over the ranks of `group`
        (see ``UMAcore.enable_graph_parallel``).  Every later ``get_energy / get_forces / get_hessian`` call is then a collective."""
        if on and self._hess_shard:
            raise RuntimeError("enable_graph_parallel: FD-Hessian column sharding is on (enable_hessian_sharding); the two cannot be combined")
        if on and getattr(self, "hessian_pin_graph", False):
            raise ValueError(PIN_NOT_GP)
        self._ensure_core(elem).enable_graph_parallel(on, group)

    def enable_hessian_sharding(self, on: bool = True, group=None) -> None:
        """Deal the FD-Hessian columns over the ranks of `group` (default: the world) -- c4's "freq Hessian (3N force
        batches) on 8 GPUs".  From then on ``get_hessian`` is a COLLECTIVE: every rank of the group must call it with the
        same geometry (checked).  Off by default, so a Hessian requested by one rank only stays a local computation."""
        if on and self._core is not None and getattr(self._core, "_gp", None) is not None:
            raise RuntimeError("enable_hessian_sharding: this calculator evaluates in graph-parallel mode (workers == world size, or "
                               "enable_graph_parallel) -- every force call is already a collective over all ranks on the SAME geometry, "
                               "so the columns cannot be dealt to different ranks.  Use one or the other (UMX_WORKERS_GP=0 keeps "
                               "workers>1 from switching the graph-parallel mode on)")
        self._hess_shard, self._hess_group = bool(on), group

    def _fd_hessian_ev(self, elem: Sequence[str], coord_ang: np.ndarray) -> Dict[str, Any]:
        """Base-point E/F plus the finite-difference Hessian (eV/A^2, torch on the core's device); hessian.fd_hessian."""
        core = self._ensure_core(elem)
        if self._hess_shard and getattr(core, "_gp", None) is not None:
            # with both on, every rank would displace DIFFERENT columns and enter a different number of graph-parallel
            # collectives -- a hang, or partial sums mixed across geometries.  The graph-parallel mode wins (it may be the only way the
            # structure fits); the columns are computed by all ranks together, un-sharded.
            raise RuntimeError("FD Hessian: column sharding (enable_hessian_sharding) and the graph-parallel mode (workers == world size / "
                               "enable_graph_parallel) cannot be combined: in graph-parallel mode every force call is a collective on one geometry")
        pin = getattr(self, "hessian_pin_graph", False)
        if pin and getattr(core, "_gp", None) is not None:
            raise ValueError(PIN_NOT_GP)
        base = core.compute(coord_ang, forces=True, hessian=False)
        # the displaced geometries and their forces stay on the GPU when the core runs on the HIP engine (round 6); the graph-parallel mode and
        # stand-in cores keep the host form
        # stand-in cores keep the host form; so does an in-process pool (its blocks go to the engines from the host: the same columns, bit for bit)
        dev_fn = core.compute_batch_dev if (getattr(core, "_gp", None) is None and getattr(core, "_pool", None) is None and hasattr(core, "compute_batch_dev")
                                            and hasattr(getattr(core, "engine", None), "energy_forces_dev")
                                            and getattr(core.device, "type", "cpu") == "cuda") else None
        # hessian_pin_graph: the displaced images on the edge set of the geometry at hand -- pinned on the engine (every engine of a pool)
        # around fd_hessian, which runs exactly as without it, and unpinned whatever happens in there
        pinner = (getattr(core, "_pool", None) or core.engine) if pin else None
        if pinner is not None:
            pinner.pin_graph(coord_ang, **({"double_positions": True} if self.double_positions else {}))
        try:
            hess = H.fd_hessian(lambda c: core.compute_batch(c, forces=True)["forces"], coord_ang, self.freeze_atoms, device=core.device,
                                double=self.hessian_double, partial=self.return_partial_hessian, batch=FD_BATCH,
                                shard=self._hess_shard, group=self._hess_group, engine=getattr(core, "engine", None), batch_forces_dev=dev_fn,
                                **({"double_positions": True} if self.double_positions else {}))
        finally:
            if pinner is not None:
                pinner.unpin_graph()
        # (a pool that widens in the middle of this Hessian widens ALL its engines, engine 0 -- `engine` above -- included, so fd_hessian's
        # "compute every column again" rule sees it)
        return {"energy": base["energy"], "forces": base["forces"], "hessian": hess}

    # ---------- PySisyphus API --------------------------------------
    def get_energy(self, elem, coords):
        core = self._ensure_core(elem)
        res = core.compute(_bohr_to_ang(coords), forces=False, hessian=False)
        return {"energy": res["energy"] * EV2AU}

    def get_forces(self, elem, coords):
        core = self._ensure_core(elem)
        res = core.compute(_bohr_to_ang(coords), forces=True, hessian=False)
        f_ev = H.mask_frozen(res["forces"], self.freeze_atoms)            # zeroed in eV/A before conversion (:701)
        return {"energy": res["energy"] * EV2AU, "forces": (np.asarray(f_ev, dtype=np.float64) * F_EVAA_2_AU).reshape(-1)}

    def get_forces_batch(self, elem, coords_batch):
        """All images of a string in ONE engine call.

        ``coords_batch``: (K, 3N) or (K, N, 3) Bohr.  Returns ``{"energy": (K,) Hartree,
        "forces": (K, 3N) Hartree/Bohr float64}`` -- per image exactly what ``get_forces`` returns.
        """
        core = self._ensure_core(elem)
        c = np.asarray(coords_batch, dtype=np.float64)
        k = c.shape[0]
        res = core.compute_batch(c.reshape(k, -1, 3) * BOHR2ANG, forces=True)
        f_ev = H.mask_frozen(res["forces"], self.freeze_atoms)
        return {"energy": np.asarray(res["energy"], dtype=np.float64) * EV2AU,
                "forces": (np.asarray(f_ev, dtype=np.float64) * F_EVAA_2_AU).reshape(k, -1)}

    def get_energy_batch(self, elem, coords_batch):
        core = self._ensure_core(elem)
        c = np.asarray(coords_batch, dtype=np.float64)
        res = core.compute_batch(c.reshape(c.shape[0], -1, 3) * BOHR2ANG, forces=False)
        return {"energy": np.asarray(res["energy"], dtype=np.float64) * EV2AU}

    def get_hvp(self, elem, coords_bohr, vectors, step_bohr: Optional[float] = None, scheme: str = "central"):
        """Hessian-vector products without a Hessian: ``coords_bohr`` (3N,) or (N,3) Bohr, ``vectors`` (3N,), (M,3N) or (M,N,3) --
        directions in the coordinates' space, not normalised -- -> ``{"hvp": (M,3N) float64 Hartree/Bohr^2}`` per unit of ``vectors``.
        ``step_bohr``: the displacement per unit of ``vectors`` (None: 1e-3 A, the FD Hessian's step); ``scheme``: "central" (two images
        per vector) or "forward" (one, plus the base once per call).  One engine call (``Engine.hvp``): displaced images in float64,
        on the pinned graph of the geometry at hand; the cell of ``uma_pysis(cell=...)`` applies.

        ``freeze_atoms``: the rows of frozen atoms are zeroed in the vectors BEFORE the displacement and in the result -- this is the
        product of the ACTIVE BLOCK of the Hessian (what ``return_partial_hessian`` cuts out, embedded in 3N with zeros), not rows of
        the full Hessian times an arbitrary vector.  A graph-parallel core (``workers`` == world size / ``enable_graph_parallel``)
        raises ``ValueError``, as ``hessian_pin_graph`` does; so do a bad shape, a bad scheme and a step that is not positive."""
        core = self._ensure_core(elem)
        if getattr(core, "_gp", None) is not None:
            raise ValueError(HVP_NOT_GP)
        if scheme not in ("central", "forward"):
            raise ValueError(f"get_hvp: scheme must be 'central' or 'forward', got {scheme!r}")
        x = _bohr_to_ang(coords_bohr)
        n = x.shape[0]
        v = np.array(vectors, dtype=np.float64)
        if v.size == 0 or v.size % (3 * n) != 0 or (v.ndim > 1 and v.shape[0] != v.size // (3 * n)):
            raise ValueError(f"get_hvp: vectors must be (3N,), (M,3N) or (M,N,3) with N = {n}, got {v.shape}")
        v = v.reshape(-1, n, 3)
        step_ang = H.FD_STEP_ANG if step_bohr is None else float(step_bohr) * BOHR2ANG
        if not (np.isfinite(step_ang) and step_ang > 0.0):
            raise ValueError(f"get_hvp: the step must be finite and positive, got {step_bohr!r}")
        if self.freeze_atoms:
            v[:, np.asarray(self.freeze_atoms, dtype=int), :] = 0.0
        hv = np.array(core.hvp(x, v, step=step_ang, scheme=scheme), dtype=np.float64).reshape(-1, n, 3)
        if self.freeze_atoms:
            hv[:, np.asarray(self.freeze_atoms, dtype=int), :] = 0.0
        return {"hvp": (hv * H.EV_PER_ANG2_TO_AU).reshape(-1, 3 * n)}

    def get_lowest_modes(self, elem, coords_bohr, k: int = 1, masses_amu=None, *, project: str = "auto", step_bohr: Optional[float] = None,
                         scheme: str = "central", block=None, max_subspace=None, tol=None, max_iter: int = 200, v0=None, seed: int = 0):
        """The ``k`` lowest vibrational modes without a Hessian (block Davidson on Hessian-vector products, ``modes.lowest_modes``):
        ``coords_bohr`` (3N,) or (N,3) Bohr -> ``{"freqs_cm": (k,) signed wavenumbers (negative = imaginary), "eigenvalues": (k,)
        Hartree/Bohr^2/amu, "modes": (k,3N) Cartesian displacements, each normalised (the reference's convention), "converged": (k,)
        bool, "residuals": (k,) Hartree/Bohr^2/amu, "images": evaluations spent}``.

        masses_amu: (N,) amu; None takes pysisyphus' table for ``elem`` when pysisyphus can be imported and raises ``ValueError``
        otherwise (the package has no table of its own).  ``freeze_atoms`` are held fixed (their rows of ``modes`` are zero) and the
        cell of ``uma_pysis(cell=...)`` applies; ``project="auto"``: translations and rotations for open boundaries, translations in a
        cell without frozen atoms, nothing in a cell with frozen atoms.  ``step_bohr``: per unit of the Cartesian direction (None:
        1e-3 A); ``tol``: on the residual norms, in Hartree/Bohr^2/amu (None: ``modes.DEFAULT_TOL``, 1.8e-3 eV/A^2/amu).  ``v0``: start
        vectors in the mass-weighted space, (j,3N).  A graph-parallel core raises ``ValueError``, as ``get_hvp`` does."""
        core = self._ensure_core(elem)
        if getattr(core, "_gp", None) is not None:
            raise ValueError(MODES_NOT_GP)
        x = _bohr_to_ang(coords_bohr)
        if masses_amu is None:
            try:
                from pysisyphus.elem_data import MASS_DICT
            except ImportError as exc:
                raise ValueError("get_lowest_modes: masses_amu is needed (N values in amu): pysisyphus, whose table would be used, "
                                 "cannot be imported and this package has no table of its own") from exc
            masses_amu = [MASS_DICT[str(e).lower()] for e in elem]
        m = np.asarray(masses_amu, dtype=np.float64).reshape(-1)
        if m.shape[0] != x.shape[0]:
            raise ValueError(f"get_lowest_modes: {x.shape[0]} atoms, but masses_amu has {m.shape[0]} entries")
        step_ang = H.FD_STEP_ANG if step_bohr is None else float(step_bohr) * BOHR2ANG
        res = core.lowest_modes(x, m, int(k), frozen=tuple(self.freeze_atoms or ()), project=project, step=step_ang, scheme=scheme, block=block,
                                max_subspace=max_subspace, tol=None if tol is None else float(tol) / H.EV_PER_ANG2_TO_AU, max_iter=max_iter,
                                v0=v0, seed=seed)
        return {"freqs_cm": np.array(res.freqs_cm), "eigenvalues": np.asarray(res.eigenvalues) * H.EV_PER_ANG2_TO_AU,
                "modes": np.asarray(res.modes, dtype=np.float64).reshape(len(res.eigenvalues), -1), "converged": np.array(res.converged),
                "residuals": np.asarray(res.residuals) * H.EV_PER_ANG2_TO_AU, "images": int(res.images)}

    def get_ts(self, elem, coords_bohr, mode=None, **kw):
        """Refine a transition-state guess to a first-order saddle without a Hessian (a dimer on Hessian-vector products,
        ``dimer.refine_saddles``): ``coords_bohr`` (3N,) or (N,3) Bohr, ``mode`` (3N,) or (N,3) the start direction (None: the lowest
        mode of ``lowest_modes`` with unit masses) -> ``{"coords": (3N,) Bohr, "energy": Hartree, "forces": (3N,) Hartree/Bohr (frozen
        rows zeroed), "mode": (3N,) unit vector, "curvature": Hartree/Bohr^2, "converged", "cycles", "images"}``.

        Keywords: ``thresh`` a name of ``gsm.THRESH`` or ``(max_force, rms_force)`` in Hartree/Bohr; ``step_bohr`` and ``max_step_bohr``
        (None: 1e-3 A and 0.1 A); ``max_cycles``, ``max_rot``, ``rot_tol``, ``project`` as ``dimer.refine_saddles`` takes them.
        ``freeze_atoms`` are held fixed and the cell of ``uma_pysis(cell=...)`` applies.  A graph-parallel core raises ``ValueError``, as
        ``get_hvp`` does."""
        core = self._ensure_core(elem)
        if getattr(core, "_gp", None) is not None:
            raise ValueError(TS_NOT_GP)
        x = _bohr_to_ang(coords_bohr)
        n = x.shape[0]
        kw = dict(kw)
        thresh = kw.pop("thresh", "gau")
        if not isinstance(thresh, str):
            thresh = tuple(float(t) / F_EVAA_2_AU for t in thresh)
        step_bohr, max_step_bohr = kw.pop("step_bohr", None), kw.pop("max_step_bohr", None)
        if step_bohr is not None:
            kw["step"] = float(step_bohr) * BOHR2ANG
        if max_step_bohr is not None:
            kw["max_step"] = float(max_step_bohr) * BOHR2ANG
        m0 = None if mode is None else np.asarray(mode, dtype=np.float64).reshape(1, n, 3)
        res = core.refine_saddles(x, m0, frozen=tuple(self.freeze_atoms or ()), thresh=thresh, **kw)[0]
        f_ev = H.mask_frozen(np.asarray(res.forces, dtype=np.float64), self.freeze_atoms)
        return {"coords": (np.asarray(res.x, dtype=np.float64) * ANG2BOHR).reshape(-1), "energy": float(res.energy) * EV2AU,
                "forces": (f_ev * F_EVAA_2_AU).reshape(-1), "mode": np.asarray(res.mode, dtype=np.float64).reshape(-1),
                "curvature": float(res.curvature) * H_EVAA_2_AU, "converged": bool(res.converged), "cycles": int(res.cycles),
                "images": int(res.images)}

    def get_hessian(self, elem, coords):
        """Hessian per ``hessian_calc_mode`` with the reference's dispatch (``:708-780``): "Analytical" only when the core
        exposes a differentiable model and is not a parallel predictor, anything else (falsy, unknown, FiniteDifference) is
        the central-difference route.  The HIP engine exposes no such model (``UMAcore.has_torch_model`` is False), so on
        the engine every mode resolves to FiniteDifference -- exactly like the reference with ``workers > 1`` (``:736-737``)."""
        core = self._ensure_core(elem)
        coord_ang = _bohr_to_ang(coords)
        force_fd = core.parallel_predict or (not core.has_torch_model)
        mode = (self.hessian_calc_mode or "FiniteDifference").strip().lower()
        if (not force_fd) and mode in ("analytical", "analytic"):
            res = core.compute(coord_ang, forces=True, hessian=True)
            hess = H.active_trim(res["hessian"], self.freeze_atoms, partial=self.return_partial_hessian)
        else:
            res = self._fd_hessian_ev(elem, coord_ang)
            hess = res["hessian"]
        f_ev = H.mask_frozen(res["forces"], self.freeze_atoms)
        return {"energy": res["energy"] * EV2AU, "forces": (np.asarray(f_ev, dtype=np.float64) * F_EVAA_2_AU).reshape(-1),
                "hessian": H.hessian_to_au(hess, double=self.hessian_double, as_torch=self.out_hess_torch)}


def _cell_and_flags(cell, pbc):
    """(cell (3,3) float64 copy, three bools), or (None, None) for open boundaries: no cell, or no flag set.  A cell without flags is
    refused rather than read as open or as fully periodic."""
    if cell is None:
        return None, None
    if pbc is None:
        raise ValueError("uma_pysis: a cell needs pbc (a bool or three flags)")
    flags = tuple(bool(x) for x in np.broadcast_to(np.asarray(pbc, dtype=bool), (3,)))
    if not any(flags):
        return None, None
    c = np.array(cell, dtype=np.float64).reshape(3, 3)
    if not np.isfinite(c).all():
        raise ValueError("uma_pysis: non-finite cell entry")
    return c, flags


def _bohr_to_ang(coords) -> np.ndarray:
    return np.asarray(coords, dtype=np.float64).reshape(-1, 3) * BOHR2ANG


# ---------- CLI ----------------------------------------
def run_pysis():
    """Enable ``uma_pysis input.yaml`` (reference ``:784-789``); needs pysisyphus installed."""
    try:
        from pysisyphus import run
    except ImportError as exc:  # pragma: no cover
        raise ImportError("run_pysis() needs pysisyphus, which is not installed in this environment") from exc
    run.CALC_DICT["uma_pysis"] = uma_pysis
    run.run()
