"""Multi-GPU evaluation of a reaction string: one process per GPU (1, 2), or several GPUs from ONE process (3).

1. IMAGE SHARDING (the default): images of one string split into contiguous blocks, ONE all-gather of
   per-image [E | F(3N)] (float64) per string iteration -- :class:`ShardedImageEvaluator`.
2. GRAPH-PARALLEL SINGLE IMAGE (rows a12 / f4; for fewer images than GPUs, e.g. one 20 000-atom structure): the
   reference's ``workers > 1`` semantics (``uma_pysis.py:220-242``) -- the graph of ONE image partitioned by target node over
   the ranks, node-level buffers all-reduced at the engine's exchange points -- :class:`GraphParallelEvaluator`.
3. LOCAL ENGINE POOL: G engines in one process, no ``torch.distributed`` and no launcher -- what the reference's single-process
   ``workers=G`` calculator does (``uma_pysis.py:220-242``, ``path_opt.py:545-559,823``).  Batches are dealt over the engines in
   the blocks of (1), one host thread per engine; one image is evaluated graph-parallel as in (2) with the exchange done by
   ``umx_peer_sum`` (the engines' partial-sum buffers are addressable from every device of the process) --
   :class:`LocalEnginePool`.

The reference evaluates the images serially through one shared calculator (``path_opt.py:949-954``,
``GS_KW["scheduler"] = None`` at ``path_opt.py:184``); its ``workers>1`` knob is graph-parallelism
inside one image (``uma_pysis.py:220-242``).  Images are independent, so the data path needs no
collective; the only exchange is the result gather in front of the (replicated, deterministic)
string update.  Payload at 2000 atoms x 16 images: 768 KB -> latency bound, a single
``all_gather_into_tensor`` over RCCL/xGMI.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist


def shard_bounds(n_images: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous block of images owned by ``rank`` (first ``n_images % world`` ranks get one more)."""
    base, rem = divmod(n_images, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


class ShardedImageEvaluator:
    """Evaluate a string's images on their owner ranks and return the gathered (E, F) on every rank.

    ``evaluate_local(coords_local[k,N,3]) -> (E[k] float64, F[k,N,3])`` runs on this rank's device.

    Every rank ALWAYS completes the collective.  A rank whose ``evaluate_local`` raises (a non-finite coordinate in its shard, the
    sticky ``UMX_ERR_RANGE`` of the asynchronous device-pointer entry, a HIP error) fills its slot with NaN, sets the STATUS column
    of the slot and enters the all-gather like everybody else; afterwards every rank raises -- the failing rank its own exception,
    the peers a ``RuntimeError`` naming the failing ranks -- instead of the peers blocking in the collective until the backend's
    timeout.
    """

    def __init__(self, evaluate_local: Callable, n_images: int, n_atoms: int, device: torch.device,
                 group: Optional["dist.ProcessGroup"] = None, engine=None, check: str = "sync", force_collective: bool = False):
        """force_collective: issue the all-gather even in a one-rank group (it is the identity there) -- exercises the RCCL call on
        the evaluator's own buffers where only one GPU is available (tests).

        engine: the ``Engine`` behind ``evaluate_local`` when that goes through the asynchronous device-pointer entry
        (``umx_energy_forces_dev`` cannot refuse a non-finite energy itself).  With it, the gathered energies are checked:
        they are the same on every rank, so every rank takes the same decision without a further collective.

        check = "sync" (default): looked at right after the gather (one scalar read per call = one host synchronisation); a non-finite
        energy widens the engine to bf16 forward planes on all ranks (``Engine.widen``, fast split-f16 mode only) and evaluates again,
        or raises.  check = "deferred": no host synchronisation of its own -- the flag of call i is computed on the device, copied to
        pinned host memory on the same stream, and read at the START of call i+1 behind the engine's own per-call synchronisation
        (the D2H read of the edge counts), or by ``flush()``; a non-finite energy then raises on every rank (the caller has already
        consumed the bad energies, so there is nothing to repeat).  For loops that never leave the device (bench.py, device string
        updates): at the 52-ms 2-image shard of the 8-GPU run a forced synchronisation per iteration is no longer free."""
        if check not in ("sync", "deferred"):
            raise ValueError(f"check must be 'sync' or 'deferred', got {check!r}")
        self.evaluate_local = evaluate_local
        self.engine = engine
        self.check = check
        self.n_images, self.n_atoms, self.device, self.group = n_images, n_atoms, device, group
        initialised = dist.is_available() and dist.is_initialized()
        self.distributed = initialised and (dist.get_world_size(group) > 1 or bool(force_collective))
        self.world = dist.get_world_size(group) if self.distributed else 1
        self.rank = dist.get_rank(group) if self.distributed else 0
        self.lo, self.hi = shard_bounds(n_images, self.world, self.rank)
        self.width = 2 + 3 * n_atoms                             # [E | status | F(3N)]
        # equal-size slots so a single all_gather_into_tensor works for ragged shards
        self.slot = -(-n_images // self.world)
        self._send = torch.zeros(self.slot, self.width, dtype=torch.float64, device=device)
        self._recv = torch.zeros(self.world * self.slot, self.width, dtype=torch.float64, device=device)
        # gloo has no device collectives: stage through the host (rehearsal of the N>1 path on boxes without RCCL peers)
        self._stage_cpu = self.distributed and device.type != "cpu" and dist.get_backend(group) == "gloo"
        self._calls = 0
        self._pending = None                                     # (call number, event behind the flag copy) of the deferred check
        if check == "deferred":
            pin = device.type == "cuda"
            self._flag_host = torch.zeros(2, dtype=torch.float64, pin_memory=pin)
            self._flag_dev = torch.zeros(2, dtype=torch.float64, device=device)

    def _raise_status(self, failed_ranks, own_exc):
        if own_exc is not None:
            raise own_exc
        raise RuntimeError(f"sharded string evaluation: evaluate_local raised on rank(s) {failed_ranks} (this is rank {self.rank}); "
                           "their error text is on those ranks")

    def _take_deferred(self):
        """Look at the flags of the previous call (already in pinned host memory: the engine synchronised the stream they were copied on)."""
        if self._pending is None:
            return
        n, ev = self._pending
        self._pending = None
        if ev is not None and not ev.query():                    # normally complete: the engine call of this iteration began with a
            ev.synchronize()                                     # stream synchronisation (a rank without images, or a caller without an engine, waits here)
        bad_e, failed = float(self._flag_host[0]), float(self._flag_host[1])
        if failed > 0.0:
            raise RuntimeError(f"sharded string evaluation: evaluate_local raised on a peer rank in call {n}")
        if bad_e > 0.0:
            if self.engine is not None:
                self.engine.take_range_error()
            raise RuntimeError(f"non-finite energy in call {n} of a sharded string evaluation (precision mode "
                               f"{self.engine.precision_mode() if self.engine is not None else '?'}; found by the deferred check, the "
                               "caller has consumed it): non-finite coordinates, or an activation beyond the operand range of the fast split-f16 mode")

    def flush(self):
        """Deferred mode: synchronise and check the last call's flags (call once after a loop)."""
        if self.check == "deferred" and self._pending is not None:
            if self.device.type == "cuda":
                torch.cuda.current_stream(self.device).synchronize()
            self._take_deferred()

    def __call__(self, coords: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        k = self.hi - self.lo
        own_exc = None
        self._calls += 1
        if k > 0:
            try:
                e, f = self.evaluate_local(coords[self.lo:self.hi])
                # (the engine call above began with its own stream synchronisation: the previous call's flags have landed)
                self._send[:k, 0] = e.to(torch.float64)
                self._send[:k, 1] = 0.0
                self._send[:k, 2:] = f.reshape(k, -1).to(torch.float64)
            except Exception as exc:      # noqa: BLE001 -- whatever it is, the peers are waiting in the collective
                own_exc = exc
                self._send[:k] = float("nan")
                self._send[:k, 1] = 1.0
        if self.check == "deferred" and own_exc is None:
            self._take_deferred()
        if not self.distributed:
            out = self._send[: self.n_images]
        else:
            if self._stage_cpu:
                recv = torch.empty(self._recv.shape, dtype=torch.float64)
                dist.all_gather_into_tensor(recv, self._send.cpu(), group=self.group)
                self._recv.copy_(recv)
            else:
                dist.all_gather_into_tensor(self._recv, self._send, group=self.group)
            rows = []
            for r in range(self.world):
                lo, hi = shard_bounds(self.n_images, self.world, r)
                rows.append(self._recv[r * self.slot: r * self.slot + (hi - lo)])
            out = torch.cat(rows, dim=0)
        if own_exc is not None:                                  # the collective is complete: now this rank may leave
            self._raise_status([self.rank], own_exc)
        if self.check == "deferred":
            self._flag_dev[0] = (~torch.isfinite(out[:, 0])).any().to(torch.float64)
            self._flag_dev[1] = (out[:, 1] > 0).any().to(torch.float64)
            self._flag_host.copy_(self._flag_dev, non_blocking=True)
            ev = None
            if self.device.type == "cuda":
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
            self._pending = (self._calls, ev)
            return out[:, 0].clone(), out[:, 2:].reshape(self.n_images, self.n_atoms, 3).clone()
        status = out[:, 1]
        if bool((status > 0).any()):                             # identical on every rank
            failed = sorted({r for r in range(self.world)
                             if bool((status[shard_bounds(self.n_images, self.world, r)[0]: shard_bounds(self.n_images, self.world, r)[1]] > 0).any())})
            self._raise_status(failed, None)
        if self.engine is not None and not bool(torch.isfinite(out[:, 0]).all()):
            self.engine.take_range_error()                      # collect (clear) the sticky flag of this rank's engine, if it was the one
            if self.engine.widen("non-finite energy in a sharded string evaluation"):
                return self(coords)                             # every rank is here with the same gathered energies: all widen, all repeat
            bad = torch.nonzero(~torch.isfinite(out[:, 0])).flatten().tolist()
            raise RuntimeError(f"non-finite energy for image(s) {bad} (precision mode {self.engine.precision_mode()}): non-finite "
                               "coordinates, or an overflow that wider forward planes cannot cure")
        return out[:, 0].clone(), out[:, 2:].reshape(self.n_images, self.n_atoms, 3).clone()


class _DeviceView:
    """A float32 device buffer owned by the engine, exposed through ``__cuda_array_interface__`` so that torch can wrap it
    without a copy (the all-reduce must happen IN PLACE in the engine's workspace)."""

    def __init__(self, ptr: int, count: int):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<f4", "data": (int(ptr), False), "version": 2}


class GraphParallelEvaluator:
    """E + F of ONE image with its graph partitioned over the ranks of ``group`` (reference ``workers > 1``).

    Every rank calls ``evaluator(pos)`` with the same float32 positions ``(N, 3)`` on its device.  Rank r owns the target
    nodes ``shard_bounds(N, world, r)`` and builds / processes only their incoming edges; the engine pauses at 10 exchange
    points (edge-degree aggregate, one node aggregate and one node gradient per layer, forces) whose buffers are summed
    over the ranks in place -- RCCL all-reduce over xGMI on the caller's stream (``backend="nccl"``), or a host-staged
    all-reduce when the group is gloo (rehearsal of the N > 1 path with several ranks on one GPU).  Energies are complete
    on every rank (node-level work is replicated), forces after the last all-reduce.  Payload per evaluation:
    9 x N x 1152 x 4 B + N x 12 B (92 MB per all-reduce at 20 000 atoms).

    ``virial=True``: the call returns ``(E, F, W)`` with ``W`` (3, 3) float64 = dE/d eps (``umx_gp_begin_virial``).  Every rank's engine
    leaves its own share of W -- the edges whose target it owns -- next to the forces; after the last step ONE ``all_gather`` of the
    (9,) float64 shares follows and every rank adds them in rank order: the same bits on all ranks, no further collective.
    ``virial=False`` is the evaluator without any of it, call for call.
    """

    def __init__(self, engine, n_atoms: int, device: torch.device, group: Optional["dist.ProcessGroup"] = None,
                 force_collective: bool = False, virial: bool = False):
        """force_collective: issue the all-reduces even in a one-rank group (they are the identity there) -- exercises the in-place
        RCCL call on the engine's own workspace memory where only one GPU is available."""
        self.engine, self.n_atoms, self.device, self.group = engine, int(n_atoms), device, group
        initialised = dist.is_available() and dist.is_initialized()
        self.distributed = initialised and (dist.get_world_size(group) > 1 or bool(force_collective))
        self.world = dist.get_world_size(group) if self.distributed else 1
        self.rank = dist.get_rank(group) if self.distributed else 0
        self.lo, self.hi = shard_bounds(self.n_atoms, self.world, self.rank)
        self._stage_cpu = self.distributed and dist.get_backend(group) == "gloo"
        self.n_exchanges = 0
        self._e = torch.zeros(1, dtype=torch.float64, device=device)
        self._f = torch.zeros(self.n_atoms, 3, dtype=torch.float32, device=device)
        self.virial = bool(virial)
        self._w = torch.zeros(9, dtype=torch.float64, device=device) if self.virial else None
        self.last_partials = None               # virial: (world, 9) float64, the ranks' shares as gathered (rank order)

    def _sum_partials(self) -> torch.Tensor:
        """W (3, 3) on the device: this rank's share, gathered over the ranks once and added in rank order."""
        if not self.distributed:
            parts = self._w.reshape(1, 9).clone()
        elif self._stage_cpu:
            rows = [torch.empty(9, dtype=torch.float64) for _ in range(self.world)]
            dist.all_gather(rows, self._w.cpu(), group=self.group)
            parts = torch.stack(rows).to(self.device)
        else:
            parts = torch.empty(self.world, 9, dtype=torch.float64, device=self.device)
            dist.all_gather_into_tensor(parts.reshape(-1), self._w, group=self.group)
        w = parts[0].clone()
        for r in range(1, parts.shape[0]):          # rank order: float64 addition does not associate
            w = w + parts[r]
        self.last_partials = parts
        return w.reshape(3, 3)

    def __call__(self, pos_ang: torch.Tensor, _retry: bool = False):
        pos = pos_ang.to(device=self.device, dtype=torch.float32).contiguous()
        if pos.shape != (self.n_atoms, 3):
            raise ValueError(f"positions must be ({self.n_atoms}, 3), got {tuple(pos.shape)}")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if self.virial:
            self.engine.gp_begin(pos.data_ptr(), self.lo, self.hi, self._e.data_ptr(), self._f.data_ptr(), stream, d_virial=self._w.data_ptr())
        else:
            self.engine.gp_begin(pos.data_ptr(), self.lo, self.hi, self._e.data_ptr(), self._f.data_ptr(), stream)
        self.n_exchanges = 0
        while True:
            ptr, count, done = self.engine.gp_step()
            if done:
                break
            self.n_exchanges += 1
            if not self.distributed:
                continue
            buf = torch.as_tensor(_DeviceView(ptr, count), device=self.device)
            if self._stage_cpu:
                host = buf.cpu()
                dist.all_reduce(host, group=self.group)
                buf.copy_(host)
            else:
                dist.all_reduce(buf, group=self.group)
        if not bool(torch.isfinite(self._e).all()):
            # energies are complete on every rank (node-level work is replicated): every rank sees the same value and takes the same path
            self.engine.take_range_error()
            if not _retry and self.engine.widen("non-finite energy in a graph-parallel evaluation"):
                return self(pos_ang, _retry=True)
            raise RuntimeError(f"non-finite energy in graph-parallel mode (precision mode {self.engine.precision_mode()}): non-finite "
                               "coordinates, or an overflow that wider forward planes cannot cure")
        if self.virial:
            return self._e.clone(), self._f.clone(), self._sum_partials()
        return self._e.clone(), self._f.clone()


class ShardedStringEvaluator:
    """``evaluator(x[k, 3N]) -> (E[k], F[k, 3N])`` for ANY batch size k (a growing string changes it): the k images are sharded contiguously
    over the ranks of `group` through a :class:`ShardedImageEvaluator` cached per k; ``local_fn(x_local[kl, N, 3]) -> (E[kl], F[kl, N, 3])``
    evaluates this rank's block on `device`.  The device contract of ``gsm.GrowingStringDriver(evaluate_device=...)``."""

    def __init__(self, local_fn: Callable, n_atoms: int, device: torch.device, group: Optional["dist.ProcessGroup"] = None, engine=None,
                 check: str = "sync", force_collective: bool = False):
        self.local_fn, self.n_atoms, self.device, self.group, self.engine, self.check = local_fn, int(n_atoms), device, group, engine, check
        self.force_collective = bool(force_collective)
        self._ev: dict = {}

    def __call__(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        k = x.shape[0]
        ev = self._ev.get(k)
        if ev is None:
            ev = self._ev[k] = ShardedImageEvaluator(self.local_fn, k, self.n_atoms, self.device, group=self.group, engine=self.engine, check=self.check,
                                                     force_collective=self.force_collective)
        e, f = ev(x.reshape(k, self.n_atoms, 3))
        return e, f.reshape(k, -1)

    def flush(self):
        for ev in self._ev.values():
            ev.flush()


class EngineStringEvaluator(ShardedStringEvaluator):
    """Device evaluator of string images for a device-resident driver (``gsm.GrowingStringDriver(evaluate_device=...)``, bench.py):
    ``evaluator(x[k, 3N] Bohr float64 on the engine's GPU) -> (E[k] Hartree float64, F[k, 3N] Hartree/Bohr float64)`` on the same
    device, exactly what ``uma_pysis.get_forces_batch`` returns per image (``uma_pysis.py:695-706``: float32 Angstrom positions into
    the model, frozen-atom force rows zeroed in eV/A, unit conversion in float64) -- but nothing crosses PCIe: positions are converted
    on the device, the engine runs through its device-pointer entry on torch's current stream, and with more than one rank the k
    images are sharded contiguously over the ranks with ONE all-gather of [E | F] (``ShardedImageEvaluator``; one cached per batch
    size, since a growing string changes k)."""

    def __init__(self, engine, n_atoms: int, device: torch.device, frozen: Sequence[int] = (), group: Optional["dist.ProcessGroup"] = None,
                 check: str = "sync", max_images: int = 0, force_collective: bool = False, gp_singles: bool = True):
        """gp_singles: with more than one rank, a ONE-image batch (the serial probes of the climbing image's Lanczos recursion,
        ``gsm._single_forces``; reference ``GS_KW["climb_lanczos"]``, ``path_opt.py:181-182``) is evaluated GRAPH-PARALLEL over all ranks
        (:class:`GraphParallelEvaluator`: the image's edges partitioned by target node, 10 all-reduces) instead of on rank 0 while the
        others wait in the all-gather -- every rank calls the evaluator with the same geometry anyway (SPMD driver)."""
        from ._calculator_base import BOHR2ANG
        from .hessian import EV_PER_ANG_TO_AU, EV_TO_HARTREE

        super().__init__(self._local, n_atoms, device, group=group, engine=engine, check=check, force_collective=force_collective)
        self._b2a, self._e2h, self._f2au = float(BOHR2ANG), float(EV_TO_HARTREE), float(EV_PER_ANG_TO_AU)
        self._frozen = torch.as_tensor(sorted(set(int(i) for i in frozen)), dtype=torch.long, device=device)
        self._cap = 0
        self._pos32 = self._e = self._f = None
        initialised = dist.is_available() and dist.is_initialized()
        self._world = dist.get_world_size(group) if initialised else 1
        self._gp_singles = bool(gp_singles) and self._world > 1
        self._gp: Optional[GraphParallelEvaluator] = None
        self.gp_single_calls = 0
        if max_images:
            self._reserve(int(max_images))
            engine.reserve_images(int(max_images))

    def _reserve(self, k: int):
        if k > self._cap:
            self._pos32 = torch.empty(k, self.n_atoms, 3, dtype=torch.float32, device=self.device)
            self._e = torch.empty(k, dtype=torch.float64, device=self.device)
            self._f = torch.empty(k, self.n_atoms, 3, dtype=torch.float32, device=self.device)
            self._cap = k

    def __call__(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._gp_singles and x.shape[0] == 1:
            if self._gp is None:
                self._gp = GraphParallelEvaluator(self.engine, self.n_atoms, self.device, group=self.group)
            self.flush()                                                             # a deferred flag of the batched calls is read before the mode changes
            e, f = self._gp((x.reshape(self.n_atoms, 3) * self._b2a).to(torch.float32))
            self.gp_single_calls += 1
            f = f.to(torch.float64) * self._f2au
            if self._frozen.numel():
                f[self._frozen, :] = 0.0
            return e.to(torch.float64) * self._e2h, f.reshape(1, -1)
        return super().__call__(x)

    def hvp(self, x0: torch.Tensor, q: torch.Tensor, dx: float, scheme: str = "central", base=None, return_base: bool = False):
        """``H(x0) . q`` in Hartree/Bohr^2, (3N,) float64 on the device, through ``umx_hvp_dev`` on torch's current stream: ``x0`` (3N,)
        Bohr and ``q`` (3N,) stay on the device, the displaced images ``x0 +- dx q`` are formed there in float64 and evaluated on the
        pinned graph of ``x0`` (the engine pins it for the call unless the caller holds a pin).  Rows of frozen atoms are zeroed in ``q``
        before the displacement and in the result: the product of the active block.  ``scheme="central"``: two images; ``"forward"``:
        the base and one image -- ``return_base=True`` also returns the base's forces (a float32 device tensor, eV/A), and handing them
        back as ``base`` makes every further product at the same ``x0`` cost ONE image.  ``images_last`` says what the call cost.
        Single rank only: a product through the sharded evaluators is not provided (``ValueError``)."""
        from .hessian import EV_PER_ANG2_TO_AU

        if self._world > 1:
            raise ValueError("EngineStringEvaluator.hvp: Hessian-vector products through the sharded evaluators are not provided (one rank only)")
        n = self.n_atoms
        b = (x0.reshape(n, 3).to(torch.float64) * self._b2a).contiguous()
        d = q.reshape(n, 3).to(torch.float64).clone()
        if self._frozen.numel():
            d[self._frozen, :] = 0.0
        hv = torch.empty(n, 3, dtype=torch.float64, device=self.device)
        f0 = base if base is not None else (torch.empty(n, 3, dtype=torch.float32, device=self.device) if return_base else None)
        self.engine.hvp_dev(1, b.data_ptr(), 1, d.data_ptr(), hv.data_ptr(), step=float(dx) * self._b2a, scheme=scheme,
                            d_f0=f0.data_ptr() if f0 is not None else 0, given_f0=base is not None,
                            stream=torch.cuda.current_stream(self.device).cuda_stream)
        self.images_last = 2 if (scheme == "central" or base is None) else 1
        hv = hv * float(EV_PER_ANG2_TO_AU)
        if self._frozen.numel():
            hv[self._frozen, :] = 0.0
        return (hv.reshape(-1), f0) if return_base else hv.reshape(-1)

    def hvp_pin(self, x0: torch.Tensor) -> None:
        """Pin the graph of ``x0`` (3N,) Bohr -- the float64 Angstrom geometry ``hvp`` takes as its base, read to the host ONCE -- so
        that the products of a whole recursion at ``x0`` replay it: no read-back, no graph build, no allocation per product
        (``gsm.GrowingStringDriver`` pins around each Lanczos recursion).  The graph is the one ``hvp`` would pin for itself: same bits."""
        self.engine.pin_graph((x0.reshape(self.n_atoms, 3).to(torch.float64) * self._b2a).cpu().numpy(), double_positions=True)

    def hvp_unpin(self) -> None:
        self.engine.unpin_graph()

    def _local(self, c_bohr: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        kl = c_bohr.shape[0]
        self._reserve(kl)
        self._pos32[:kl].copy_(c_bohr.reshape(kl, self.n_atoms, 3) * self._b2a)      # AtomicData.pos is float32 Angstrom
        # the engine enqueues on torch's current stream: producer (the copy above) and consumers (conversion below, the all-gather)
        # are ordered with it by the stream alone
        self.engine.energy_forces_dev(kl, self._pos32.data_ptr(), self._e.data_ptr(), self._f.data_ptr(),
                                      stream=torch.cuda.current_stream(self.device).cuda_stream)
        f = self._f[:kl].to(torch.float64) * self._f2au
        if self._frozen.numel():
            f[:, self._frozen, :] = 0.0                                              # uma_pysis.py:561-567
        return self._e[:kl] * self._e2h, f


# ================================================================================================================================
#                                   several engines in ONE process (no process group)
# ================================================================================================================================
def process_group_active() -> bool:
    return bool(dist.is_available() and dist.is_initialized())


def local_devices_for(workers: int, device_count: Optional[Callable[[], int]] = None) -> Optional[List[int]]:
    """Device ordinals of an in-process pool for ``workers`` (> 1) engines, or None when there is nothing to build one from.

    ``UMX_LOCAL_DEVICES="0,1,2,3"`` names them explicitly; an ordinal may repeat (``"0,0"``: several engines share that device -- the
    rehearsal of the path on a one-GPU box).  Its length must equal ``workers`` (``ValueError`` otherwise).  Without the variable: the
    first ``workers`` visible devices when there are that many, else None (the caller keeps its single engine)."""
    workers = int(workers)
    env = os.environ.get("UMX_LOCAL_DEVICES", "").strip()
    if env:
        try:
            devs = [int(t) for t in env.split(",")]
        except ValueError:
            raise ValueError(f"UMX_LOCAL_DEVICES={env!r}: expected comma-separated device ordinals such as '0,1,2,3'") from None
        if any(d < 0 for d in devs):
            raise ValueError(f"UMX_LOCAL_DEVICES={env!r}: device ordinals are non-negative")
        if len(devs) != workers:
            raise ValueError(f"UMX_LOCAL_DEVICES={env!r} names {len(devs)} device(s) but workers={workers}: the two must agree")
        return devs
    n = int(device_count() if device_count is not None else torch.cuda.device_count())
    return list(range(workers)) if workers > 1 and n >= workers else None


def shared_workspace_limits(devices: Sequence[int], free_bytes: Callable[[int], int]) -> List[int]:
    """Workspace cap in bytes per engine of a pool (0 = leave the engine's own rule): engines that share a device ordinal share its
    HBM, so the cap one engine would have -- ``UMX_WS_GB`` GiB (default 160), but no more than the automatic 85 % of what is free on
    the device now, which is all there is with ``UMX_WS_GB=0`` -- is divided among them."""
    devices = [int(d) for d in devices]
    env_gb = int(os.environ.get("UMX_WS_GB", "160") or 0)
    out = []
    for d in devices:
        share = devices.count(d)
        if share == 1:
            out.append(0)
            continue
        cap = int(free_bytes(d) * 0.85)
        if env_gb > 0:
            cap = min(cap, env_gb << 30)
        out.append(max(cap // share, 1))
    return out


GP_FLOAT32_ONLY = ("graph_parallel=True with double_positions=True: the graph-parallel entries (umx_gp_begin[_virial]) take float32 "
                   "positions only -- leave one of the two off (a single geometry with double positions runs on engine 0)")


class LocalEnginePool:
    """G engines owned by ONE process, one per listed device ordinal, all with the same weights, precision mode and system.

    * ``energy_forces(coords[K,N,3])`` with K >= 2: engine r evaluates the contiguous block ``shard_bounds(K, G, r)`` on a host
      thread of its own (the ctypes call releases the GIL); results are concatenated in image order.  Engines whose block is empty
      do nothing.  Results do not depend on how a batch is chunked (include/umx.h), so this IS the single-engine result, bit for bit.
      When engines raise, all threads are joined first and the error of the lowest engine index is raised.  An fp16 range violation
      (fast split-f16 mode) that widened one engine widens ALL of them and the whole batch is evaluated again, so that one result
      never mixes two arithmetics.
    * K == 1 with a virial (``energy_forces_virial`` / ``energy_forces_stress``): engine 0 alone by default; ``graph_parallel=True``
      takes the route below with ``umx_gp_begin_virial`` -- every engine's share of W comes back with its forces and the shares are
      added in engine order in float64 on the host.
    * K == 1: graph-parallel over the pool (unless ``gp=False`` / ``UMX_WORKERS_GP=0``: engine 0 alone).  Engine r builds the incoming
      edges of the target nodes ``shard_bounds(N, G, r)``; all engines step to the next exchange point, ``umx_peer_sum`` adds their
      partial-sum buffers in place in engine order, and so on until done (10 exchanges).  Energies and forces are then complete --
      and identical in every bit -- on every engine; engine 0's are returned.

    More than one PHYSICAL device has never run: two engines on device 0 show the host path and the sum only.
    """

    def __init__(self, engines: Sequence, *, gp: Optional[bool] = None, peer_sum: Optional[Callable] = None,
                 tensor_device: Optional[Callable] = None, free_bytes: Optional[Callable[[int], int]] = None):
        """engines: G engines (``engine.Engine`` or anything with its methods), weights loaded; ``create`` builds them.
        gp: None = the ``UMX_WORKERS_GP`` switch (default on).  peer_sum / tensor_device / free_bytes: the device exchange
        (``engine.peer_sum``), where engine r's staging tensors live (``cuda:<engine.device>``) and the free HBM of an ordinal
        (``torch.cuda.mem_get_info``) -- replaceable so that the host logic can be exercised without a GPU."""
        if len(engines) < 1:
            raise ValueError("LocalEnginePool needs at least one engine")
        self.engines = list(engines)
        self.devices = [int(e.device) for e in self.engines]
        self.gp = (os.environ.get("UMX_WORKERS_GP", "1") != "0") if gp is None else bool(gp)
        if peer_sum is None:
            from .engine import peer_sum
        self._peer_sum = peer_sum
        self._tensor_device = tensor_device or (lambda eng: torch.device("cuda", int(eng.device)))
        self._threads = ThreadPoolExecutor(max_workers=len(self.engines), thread_name_prefix="umx-pool")
        self._gp_buf = None                     # per engine: (device, stream, pos, e, f) of the graph-parallel route, made at first use
        self.natoms = int(getattr(self.engines[0], "natoms", 0) or 0)
        self.n_exchanges = 0                    # exchange points of the most recent one-image evaluation
        self.last_route = None                  # "batch" | "graph-parallel" | "single"
        self.last_blocks: List[Tuple[int, int]] = []
        self.last_all = None                    # graph-parallel route: [(E, F)] of EVERY engine (they must agree in every bit)
        self.last_partials = None               # graph-parallel route with a virial: [W_r (9,) float64] of every engine, its own share
        self._gp_wbuf = None                    # per engine: the (9,) float64 device buffer of that share, made at first use
        self._cells = None                      # per-image cells (``set_cells``): (cells (K,3,3) float64, pbc flags (3,)), else None
        self._cells_on = [None] * len(self.engines)   # what engine r has bound of them: its block (lo, hi), or "single" for cells[0] alone
        self.recompute = None                   # what ``create`` / ``set_recompute`` gave every engine (None: the engines' own setting)
        self._pinned = False                    # a graph is pinned on every engine (``pin_graph``): a single geometry goes to engine 0 alone
        self._pin_refs = 0                      # references pinned on every engine (``pin_graphs``; 1: ``pin_graph``)
        self._pin_assign = None                 # the reference of image k of a call (``pin_assign``), None: the engines' default
        self._assign_on = [None] * len(self.engines)   # the slice of the assignment engine r holds now (a tuple), None: its default
        if len(set(self.devices)) < len(self.devices):
            free = free_bytes or (lambda d: torch.cuda.mem_get_info(d)[0])
            for eng, lim in zip(self.engines, shared_workspace_limits(self.devices, free)):
                if lim:
                    eng.set_workspace_limit(lim)

    @classmethod
    def create(cls, devices: Sequence[int], weights, *, precision: Optional[str] = None, engine_factory: Optional[Callable] = None,
               recompute: Optional[int] = None, **pool_kw) -> "LocalEnginePool":
        """One engine per entry of ``devices`` (ordinals may repeat), each loaded with ``weights``; bind the system with ``set_system``.
        recompute: None = every engine's own ``UMX_RECOMPUTE``, else 0 | 1 | 2 for every engine (``Engine.set_recompute``)."""
        if engine_factory is None:
            from .engine import Engine as engine_factory
        engines = []
        try:
            for d in devices:
                eng = engine_factory(int(d), precision=precision)
                engines.append(eng)
                if recompute is not None:
                    eng.set_recompute(int(recompute))
                eng.load_weights(weights)
        except Exception:
            for eng in engines:
                eng.close()
            raise
        pool = cls(engines, **pool_kw)
        pool.recompute = None if recompute is None else int(recompute)
        return pool

    def __len__(self) -> int:
        return len(self.engines)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self) -> None:
        self._gp_buf = self._gp_wbuf = None
        for eng in self.engines:
            eng.close()
        self.engines = []
        self._threads.shutdown(wait=True)

    # ---- the same setup on every engine ------------------------------------------------------------------------------------------
    def set_system(self, atomic_numbers, **kw) -> None:
        for eng in self.engines:
            eng.set_system(atomic_numbers, **kw)
        self.natoms = len(atomic_numbers)
        self._gp_buf = self._gp_wbuf = None
        self._unpinned()                        # (umx_set_system unpins)

    # ---- pinned neighbour graph ----------------------------------------------------------------------------------------------------
    def pin_graph(self, pos_ang, double_positions: bool = False) -> None:
        """``Engine.pin_graph`` on EVERY engine, with the cell each has in force: a batch dealt over the pool then sees one edge set, as on
        one engine.  While pinned, a single geometry is evaluated on engine 0 alone (``last_route == "single"``): the graph-parallel
        entries build their own graph and refuse a pinned engine.  If an engine refuses, the ones pinned before it are unpinned again."""
        from .engine import dp_kw

        done = []
        try:
            for eng in self.engines:
                eng.pin_graph(pos_ang, **dp_kw(double_positions))
                done.append(eng)
        except Exception:
            for eng in done:
                eng.unpin_graph()
            self._unpinned()
            raise
        self._unpinned()
        self._pinned, self._pin_refs = True, 1

    def _unpinned(self) -> None:
        self._pinned, self._pin_refs, self._pin_assign, self._assign_on = False, 0, None, [None] * len(self.engines)

    def pin_graphs(self, refs, double_positions: bool = False, assign=None) -> None:
        """``Engine.pin_graphs`` on EVERY engine: each pins all references, so that whichever block of a batch an engine is dealt, the
        references its images name are there.  ``assign`` as ``pin_assign``.  Routing and failure as ``pin_graph``."""
        from .engine import dp_kw

        r_count = int(np.asarray(refs).shape[0]) if np.asarray(refs).ndim == 3 else 1
        done = []
        try:
            for eng in self.engines:
                eng.pin_graphs(refs, **dp_kw(double_positions))
                done.append(eng)
            self._unpinned()
            self._pinned, self._pin_refs = True, r_count
            self.pin_assign(assign)
        except Exception:
            for eng in done:
                eng.unpin_graph()
            self._unpinned()
            raise

    def pin_assign(self, assign=None) -> None:
        """Which reference image k of the calls that follow replays (``Engine.pin_assign``), for the WHOLE call: the pool keeps the
        assignment and gives every engine the slice of its contiguous block right before that engine evaluates.  ``None``: the
        default -- reference k for image k when several are pinned, the one reference for every image otherwise.  An entry outside
        [0, R) raises ``ValueError`` and the previous assignment stays."""
        if not self._pinned:
            raise ValueError("pin_assign: nothing is pinned (pin_graphs)")
        if assign is None or len(assign) == 0:
            self._pin_assign = None
            for r, eng in enumerate(self.engines):          # (with one reference nothing is dealt: the engines' own default again)
                if self._assign_on[r] is not None:
                    eng.pin_assign(None)
                    self._assign_on[r] = None
            return
        a = tuple(int(x) for x in np.asarray(assign).reshape(-1))
        if any(x < 0 or x >= self._pin_refs for x in a):
            raise ValueError(f"pin_assign: entries must lie in [0, {self._pin_refs}), got {a}")
        self._pin_assign = a

    def _bind_assign(self, k: int, blocks) -> None:
        """Pinned references: make every engine hold the slice of the call's assignment that belongs to its block (None: one geometry,
        engine 0 alone).  The call's assignment is the one of ``pin_assign``, else reference k for image k when several are pinned."""
        if not self._pinned or (self._pin_assign is None and self._pin_refs <= 1):
            return
        a = self._pin_assign if self._pin_assign is not None else tuple(range(self._pin_refs))
        if len(a) != k:
            raise ValueError(f"{k} images, but " + (f"pin_assign assigned references to {len(a)}" if self._pin_assign is not None
                                                      else f"{len(a)} graphs are pinned and image k replays reference k by default"))
        for r, eng in enumerate(self.engines):
            lo, hi = (0, 1 if r == 0 else 0) if blocks is None else blocks[r]
            if hi <= lo or a[lo:hi] == self._assign_on[r]:
                continue
            self._assign_on[r] = None
            eng.pin_assign(a[lo:hi])
            self._assign_on[r] = a[lo:hi]

    def pinned_graphs(self):
        """Engine 0's ``pinned_graphs()``: (edges of every reference, max_degree), or None when nothing is pinned."""
        return self.engines[0].pinned_graphs() if self._pinned else None

    def pinned_each(self, refs, assign=None, double_positions: bool = False):
        """``with pool.pinned_each(refs, assign): ...`` -- ``pin_graphs`` on every engine for the block, unpinned on the way out, also on
        an exception."""
        from .engine import _Pinned, dp_kw

        return _Pinned(self, refs, dict(dp_kw(double_positions), assign=assign), "pin_graphs")

    def unpin_graph(self) -> None:
        """``Engine.unpin_graph`` on every engine (all are tried; the first error is raised afterwards)."""
        first = None
        for eng in self.engines:
            try:
                eng.unpin_graph()
            except Exception as exc:      # noqa: BLE001
                first = first or exc
        self._unpinned()
        if first is not None:
            raise first

    def pinned_graph(self):
        """Engine 0's ``pinned_graph()``: (edges, max_degree), or None when nothing is pinned."""
        return self.engines[0].pinned_graph() if self._pinned else None

    def pinned(self, pos_ang, double_positions: bool = False):
        """``with pool.pinned(x_ref): ...`` -- pinned on every engine for the block, unpinned on the way out, also on an exception."""
        from .engine import _Pinned, dp_kw

        return _Pinned(self, pos_ang, dp_kw(double_positions))

    def set_cell(self, cell=None, pbc=None) -> None:
        """``Engine.set_cell`` on every engine: batches dealt over the pool and the graph-parallel single image see the same cell."""
        for eng in self.engines:
            eng.set_cell(cell, pbc)
        self._cells, self._cells_on = None, [None] * len(self.engines)

    def set_cells(self, cells=None, pbc=None) -> None:
        """Per-image cells (``Engine.set_cells``) for the batches that follow: cell k belongs to image k.  The pool keeps them and gives
        every engine the cells of its contiguous block right before that engine evaluates (once, for as long as the blocks stay the
        same); a single geometry binds ``cells[0]`` with ``set_cell`` on every engine.  ``None`` for either argument, or no flag set:
        open boundaries on every engine."""
        flags = None if pbc is None else np.broadcast_to(np.asarray(pbc, dtype=bool), (3,))
        if cells is None or flags is None or not flags.any():
            self.set_cell(None, None)
            return
        c = np.array(cells, dtype=np.float64)
        if c.ndim != 3 or c.shape[1:] != (3, 3) or c.shape[0] == 0:
            raise ValueError(f"cells must be (K,3,3) with K >= 1, got {c.shape}")
        self._cells, self._cells_on = (c, tuple(bool(x) for x in flags)), [None] * len(self.engines)

    def _bind_cells(self, k: int, blocks) -> None:
        """Per-image cells: make every engine hold what it needs for a call of ``k`` images dealt in ``blocks`` (None: one geometry)."""
        if self._cells is None:
            return
        cells, flags = self._cells
        if len(cells) != k:
            raise ValueError(f"{k} images, but set_cells bound cells for {len(cells)} (cell k belongs to image k)")
        for r, eng in enumerate(self.engines):
            want = "single" if blocks is None else tuple(blocks[r])
            if want == self._cells_on[r] or (blocks is not None and want[1] <= want[0]):
                continue
            self._cells_on[r] = None
            if blocks is None:
                eng.set_cell(cells[0], flags)
            else:
                eng.set_cells(cells[want[0]: want[1]], flags)
            self._cells_on[r] = want

    def cell_volumes(self) -> np.ndarray:
        """[K] |det cell_k| of the per-image cells (``set_cells``), else engine 0's one volume; ``ValueError`` unless fully periodic."""
        if self._cells is None:
            return np.array([self.engines[0].cell_volume()], dtype=np.float64)
        if not all(self._cells[1]):
            raise ValueError("stress needs cells that are periodic along all three axes (set_cells): the volume is otherwise undefined")
        return np.abs(np.linalg.det(self._cells[0])).astype(np.float64)

    def last_graph_shifts(self) -> int:
        return int(self.engines[0].last_graph_shifts())

    def reserve_images(self, n_images: int) -> None:
        """Batches of up to ``n_images`` images are coming: every engine is told its share (``umx_reserve_images``)."""
        g = len(self.engines)
        for r, eng in enumerate(self.engines):
            lo, hi = shard_bounds(int(n_images), g, r)
            eng.reserve_images(hi - lo)

    def precision_mode(self) -> str:
        return self.engines[0].precision_mode()

    def set_recompute(self, mode: int) -> None:
        """``Engine.set_recompute`` on every engine.  Mode 2 is a one-GPU plan: a single image then goes to engine 0 alone, not to the
        graph-parallel route (``umx_gp_begin`` refuses an engine in mode 2)."""
        for eng in self.engines:
            eng.set_recompute(int(mode))
        self.recompute = int(mode)

    def last_recompute(self) -> int:
        """1 when any engine's most recent evaluation ran a recompute plan."""
        return int(any(eng.last_recompute() for eng in self.engines))

    # ---- evaluation --------------------------------------------------------------------------------------------------------------
    def _run_all(self, fn: Callable[[int], object], ranks: Sequence[int]) -> list:
        """fn(r) for every r of ``ranks``, one host thread each; every thread has ended before this returns or raises; the error of
        the lowest engine index wins."""
        futs = [(r, self._threads.submit(fn, r)) for r in ranks]
        out, first = {}, None
        for r, fu in futs:
            try:
                out[r] = fu.result()
            except BaseException as exc:      # noqa: BLE001 -- collected; the other threads are still joined
                if first is None:
                    first = exc
        if first is not None:
            raise first
        return [out[r] for r in ranks]

    def _widen_all(self, why: str) -> None:
        for eng in self.engines:
            if not getattr(eng, "widened", False):
                eng.widen(why)

    def _images(self, pos_ang, double_positions: bool = False) -> np.ndarray:
        """(K,N,3) float32 -- float64 with ``double_positions`` -- of what a caller passed as (K,N,3) or (N,3)."""
        p = np.ascontiguousarray(pos_ang, dtype=np.float64 if double_positions else np.float32)
        if p.ndim == 2:
            p = p[None]
        if p.ndim != 3 or p.shape[1] != self.natoms or p.shape[2] != 3:
            raise ValueError(f"positions must be (K,{self.natoms},3), got {p.shape}")
        return p

    def _deal(self, p: np.ndarray, call: Callable) -> list:
        """The batch route of every evaluation method: ``call(engine r, p[block r])`` for the engines with a non-empty contiguous block
        ``shard_bounds(K, G, r)``, one host thread each; the results in engine (= image) order."""
        k, g = p.shape[0], len(self.engines)
        blocks = [shard_bounds(k, g, r) for r in range(g)]
        busy = [r for r in range(g) if blocks[r][1] > blocks[r][0]]
        self.last_route, self.last_blocks = "batch", blocks
        self._bind_cells(k, blocks)
        self._bind_assign(k, blocks)
        return self._run_in_one_arithmetic(lambda r: call(self.engines[r], p[blocks[r][0]: blocks[r][1]]), busy)

    def _run_in_one_arithmetic(self, fn: Callable[[int], object], busy: Sequence[int]) -> list:
        """``_run_all(fn, busy)`` such that one result never mixes two arithmetics: when an engine left the fp16 operand range during the
        run and moved itself to bf16 forward planes (``Engine.energy_forces``, ``Engine.hvp``), the blocks of the others are in the
        narrower arithmetic -- all engines move, and the WHOLE batch is run again, once."""
        for attempt in range(2):
            was_wide = [bool(getattr(eng, "widened", False)) for eng in self.engines]
            res = self._run_all(fn, busy)
            if attempt == 1 or [bool(getattr(eng, "widened", False)) for eng in self.engines] == was_wide:
                return res
            self._widen_all("fp16 range violation on another engine of the local pool")

    def _deal_products(self, who: str, shared: str, m: int, blocks: list) -> list:
        """What ``hvp`` and ``hvp_candidates`` do before they run: per-image cells (``set_cells``) are taken only when exactly one is
        bound; the ``blocks`` of the ``m`` products become ``last_blocks``.  Returns the engines with a non-empty block."""
        if self._cells is not None:
            if len(self._cells[0]) != 1:
                raise ValueError(f"{who}: set_cells bound cells for {len(self._cells[0])} images; {shared} (set_cell)")
            self._bind_cells(1, None)
        self.last_route, self.last_blocks = ("batch" if m > 1 else "single"), blocks
        return [r for r in range(len(blocks)) if blocks[r][1] > blocks[r][0]]

    def energy_forces(self, pos_ang, forces: bool = True, double_positions: bool = False) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """pos_ang: (K,N,3) or (N,3) Angstrom -> (E [K] eV float64, F [K,N,3] eV/A float32 | None): ``Engine.energy_forces`` over the pool.

        double_positions (``Engine.energy_forces``): batches are dealt as before, every engine taking its block as float64.  A SINGLE
        geometry is then evaluated on engine 0 alone (``last_route == "single"``), not graph-parallel: the graph-parallel entry
        (``umx_gp_begin``) takes float32 positions only."""
        from .engine import dp_kw

        p = self._images(pos_ang, double_positions)
        kw = dp_kw(double_positions)
        if p.shape[0] == 1:
            self._bind_cells(1, None)
            if self.gp and len(self.engines) > 1 and self.recompute != 2 and not double_positions and not self._pinned:
                return self._graph_parallel(p[0], forces)
            self.last_route, self.last_blocks = "single", [(0, 1)]
            self._bind_assign(1, None)
            return self.engines[0].energy_forces(p, forces=forces, **kw)
        res = self._deal(p, lambda eng, block: eng.energy_forces(block, forces=forces, **kw))
        e = np.concatenate([r[0] for r in res])
        f = np.concatenate([r[1] for r in res]) if forces else None
        return e, f

    def hvp(self, base, dirs, base_of=None, step: float = 1e-3, scheme: str = "central", pin: bool = True, return_curvature: bool = False):
        """``Engine.hvp`` over the pool: the M directions are dealt over the engines in the contiguous blocks ``shard_bounds(M, G, r)``;
        every engine gets ALL bases and its slice of ``base_of``, pins (or replays) the graphs as ``Engine.hvp`` does and returns its
        rows of ``hv`` (and ``curv``).  A single direction runs on engine 0 (``last_route == "single"``).  Every displaced image is its
        evaluation alone on the pinned graph of its base, so the result is the single engine's, bit for bit.  Per-image cells
        (``set_cells``) are taken only when exactly one is bound, as ``Engine.hvp`` takes them."""
        b, d = self._images(base, True), self._images(dirs, True)
        m, g = d.shape[0], len(self.engines)
        a = None if base_of is None else np.ascontiguousarray(base_of, dtype=np.int32).reshape(-1)
        if a is not None and len(a) != m:
            raise ValueError(f"hvp: {m} directions, but base_of has {len(a)} entries")
        blocks = [shard_bounds(m, g, r) for r in range(g)] if m > 1 else [(0, 1)] + [(0, 0)] * (g - 1)
        busy = self._deal_products("hvp", "the displaced images of a base share its one cell", m, blocks)

        def call(r):
            lo, hi = blocks[r]
            return self.engines[r].hvp(b, d[lo:hi], None if a is None else a[lo:hi], step=step, scheme=scheme, pin=pin, return_curvature=True)

        res = self._run_in_one_arithmetic(call, busy)
        hv = np.concatenate([r[0] for r in res])
        return (hv, np.concatenate([r[1] for r in res])) if return_curvature else hv

    def lowest_modes(self, base, masses, k: int = 1, *, frozen=(), project: str = "auto", step: float = 1e-3, scheme: str = "central",
                     block=None, max_subspace=None, tol=None, max_iter: int = 200, v0=None, seed: int = 0):
        """``Engine.lowest_modes`` over the pool: the host backend of ``modes.lowest_modes`` on ``pool.hvp`` -- every iteration's block
        of directions is dealt over the engines, the small block algebra runs in NumPy in the kernels' operation order.  The graph of
        ``base`` is pinned on every engine for the call.  Products being the single engine's bit for bit, so is the result (that of
        the host backend over ``Engine.hvp``).  The forward scheme evaluates the base with every block (``pool.hvp`` hands no base
        forces back)."""
        from . import modes

        pbc = getattr(self.engines[0], "_pbc_flags", lambda: None)
        return modes.lowest_modes(modes.HostBackend(self.hvp, pinner=self), base, masses, k, frozen=frozen, project=project, step=step,
                                  scheme=scheme, block=block, max_subspace=max_subspace, tol=tol, max_iter=max_iter, v0=v0, seed=seed,
                                  periodic=self._cells is not None or pbc() is not None)

    def hvp_candidates(self, bases, dirs, base_of=None, step: float = 1e-3, scheme: str = "forward", return_base: bool = False, base_forces=None):
        """``Engine.hvp`` for K candidates with ONE direction each (``base_of = arange(K)``, what a batched dimer asks for), dealt over
        the engines in the contiguous blocks ``shard_bounds(K, G, r)`` as ``hvp`` deals directions -- but every engine gets only the
        bases of ITS candidates, so the bases' own evaluations (``return_base``: ``(hv, e0, f0)``) are dealt too, and ``base_forces`` are
        handed back block by block.  A single candidate is block (0, 1) of engine 0 (``last_route == "single"``), as ``hvp`` runs a single
        direction.  Every image is its evaluation alone on the pinned graph of its base: the single engine's bits.  This is what
        ``refine_saddles`` deals through; it is not meant as an entry of its own."""
        b, d = self._images(bases, True), self._images(dirs, True)
        k, g = d.shape[0], len(self.engines)
        if b.shape[0] != k or (base_of is not None and not np.array_equal(np.asarray(base_of).reshape(-1), np.arange(k))):
            raise ValueError(f"hvp_candidates: one direction per base in order is needed, got {b.shape[0]} bases, {k} directions, base_of {base_of!r}")
        f_in = None if base_forces is None else np.ascontiguousarray(base_forces, dtype=np.float32).reshape(b.shape)
        blocks = [shard_bounds(k, g, r) for r in range(g)]
        busy = self._deal_products("hvp_candidates", "the candidates share one cell", k, blocks)

        def call(r):
            lo, hi = blocks[r]
            out = self.engines[r].hvp(b[lo:hi], d[lo:hi], np.arange(hi - lo, dtype=np.int32), step=step, scheme=scheme, return_base=return_base,
                                      base_forces=None if f_in is None else f_in[lo:hi])
            return out if return_base else (out,)

        res = self._run_in_one_arithmetic(call, busy)              # (forces handed in are stale after a widening: the dimer repeats its cycle)
        hv = np.concatenate([r[0] for r in res])
        return (hv, np.concatenate([r[1] for r in res]), np.concatenate([r[2] for r in res])) if return_base else hv

    def refine_saddles(self, x0, modes0=None, *, frozen=(), project: str = "auto", thresh="gau", step: float = 1e-3, max_cycles: int = 200,
                       max_rot: int = 2, rot_tol: float = 0.1, max_step: float = 0.1, masses=None, verify: bool = False):
        """``Engine.refine_saddles`` over the pool: the host backend of ``dimer.refine_saddles`` on ``hvp_candidates`` -- the candidates
        of every product round are dealt over the engines, the row algebra runs in NumPy in the kernels' operation order.  Products
        being the single engine's bit for bit, so is the result (that of the host backend over ``Engine.hvp``)."""
        from . import dimer

        pbc = getattr(self.engines[0], "_pbc_flags", lambda: None)
        return dimer.refine_saddles(dimer.HostBackend(self.hvp_candidates, pinner=self, lowest_modes=self.lowest_modes), x0, modes0, frozen=frozen,
                                    project=project, thresh=thresh, step=step, max_cycles=max_cycles, max_rot=max_rot, rot_tol=rot_tol,
                                    max_step=max_step, masses=masses, verify=verify, periodic=self._cells is not None or pbc() is not None)

    def energy_forces_virial(self, pos_ang, graph_parallel: bool = False, double_positions: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``Engine.energy_forces_virial`` over the pool: (E [K], F [K,N,3], W [K,3,3] float64).  A batch is dealt over the engines in
        the same contiguous blocks as ``energy_forces`` and is the single-engine result bit for bit (W does not depend on the batch an
        image is in).  A SINGLE geometry is evaluated on engine 0 alone by default (``last_route == "single"``: the single-engine W, bit
        for bit).  ``graph_parallel=True`` with more than one engine sends it over the whole pool instead (``umx_gp_begin_virial``,
        ``last_route == "graph-parallel"``): an image that needs the pool's combined memory, all engines at work; every engine's share
        of W (``last_partials``) is added in engine order in float64 on the host.  That W differs from engine 0's as the graph-parallel
        forces do, at float32 summation order.  The opt-in cannot run with recompute mode 2 (a one-GPU plan): ``ValueError``, no silent
        fallback.  It says nothing about batches.
        double_positions (``Engine.energy_forces_virial``): batches as before; a single geometry on engine 0.  Together with
        ``graph_parallel=True`` it raises ``ValueError``: the graph-parallel entries take float32 positions only."""
        from .engine import dp_kw

        if graph_parallel and double_positions:
            raise ValueError(GP_FLOAT32_ONLY)
        if graph_parallel and self._pinned:
            raise ValueError("graph_parallel=True: a graph is pinned (pin_graph) and the graph-parallel entries build their own -- unpin, or leave graph_parallel off")
        p = self._images(pos_ang, double_positions)
        kw = dp_kw(double_positions)
        if p.shape[0] == 1:
            if graph_parallel and len(self.engines) > 1:
                if self.recompute == 2:
                    raise ValueError("graph_parallel=True: the graph-parallel virial cannot run with recompute mode 2 (a one-GPU plan; "
                                     "umx_gp_begin refuses it) -- set mode 0 or 1 on the pool, or leave graph_parallel off")
                self._bind_cells(1, None)
                return self._graph_parallel(p[0], True, virial=True)
            self._bind_cells(1, None)
            self.last_route, self.last_blocks = "single", [(0, 1)]
            self._bind_assign(1, None)
            return self.engines[0].energy_forces_virial(p, **kw)
        res = self._deal(p, lambda eng, block: eng.energy_forces_virial(block, **kw))
        return tuple(np.concatenate([r[i] for r in res]) for i in range(3))

    def energy_forces_stress(self, pos_ang, graph_parallel: bool = False, double_positions: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``Engine.energy_forces_stress`` over the pool: (E [K], F [K,N,3], stress [K,6] eV/A^3, Voigt xx, yy, zz, yz, xz, xy), routed
        as ``energy_forces_virial`` (``graph_parallel`` included); ``ValueError`` unless the cell (``set_cell``) is periodic along all
        three axes.  With per-image cells (``set_cells``) image k is divided by the volume of cell k.  ``double_positions`` as there."""
        from .engine import dp_kw, voigt_stress

        if graph_parallel and double_positions:
            raise ValueError(GP_FLOAT32_ONLY)                                 # before the cell is looked at, as energy_forces_virial says it
        vol = self.engines[0].cell_volume() if self._cells is None else self.cell_volumes()
        e, f, w = self.energy_forces_virial(pos_ang, graph_parallel=graph_parallel, **dp_kw(double_positions))
        return e, f, voigt_stress(w, vol)

    def _gp_buffers(self):
        if self._gp_buf is None:
            bufs = []
            for eng in self.engines:
                dev = self._tensor_device(eng)
                cuda = dev.type == "cuda"
                stream = torch.cuda.Stream(device=dev) if cuda else None
                bufs.append((dev, stream,
                             torch.zeros(self.natoms, 3, dtype=torch.float32, device=dev),
                             torch.zeros(1, dtype=torch.float64, device=dev),
                             torch.zeros(self.natoms, 3, dtype=torch.float32, device=dev)))
                if cuda:
                    torch.cuda.synchronize(dev)         # the fills ran on torch's current stream, the buffers are used on `stream`
            self._gp_buf = bufs
        return self._gp_buf

    def _gp_virial_buffers(self, bufs):
        if self._gp_wbuf is None:
            self._gp_wbuf = [torch.zeros(9, dtype=torch.float64, device=dev) for dev, *_ in bufs]
            for dev, *_ in bufs:
                if dev.type == "cuda":
                    torch.cuda.synchronize(dev)         # as in _gp_buffers: filled on torch's current stream, used on the engine's
        return self._gp_wbuf

    def _graph_parallel(self, pos: np.ndarray, forces: bool, _retry: bool = False, virial: bool = False):
        """virial: every engine also leaves its share of W (``umx_gp_begin_virial``); returns (E [1], F [1,N,3], W [1,3,3])."""
        if not np.isfinite(pos).all():
            raise ValueError("non-finite position")
        g, n = len(self.engines), self.natoms
        bufs = self._gp_buffers()
        wbufs = self._gp_virial_buffers(bufs) if virial else None
        host = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32))
        handles = []
        for dev, stream, d_pos, _, _ in bufs:
            if stream is not None:
                with torch.cuda.stream(stream):
                    d_pos.copy_(host)
                handles.append(int(stream.cuda_stream))
            else:
                d_pos.copy_(host)
                handles.append(0)
        self.last_route, self.last_blocks = "graph-parallel", [shard_bounds(n, g, r) for r in range(g)]

        def begin(r):
            lo, hi = self.last_blocks[r]
            _, _, d_pos, d_e, d_f = bufs[r]
            if virial:
                self.engines[r].gp_begin(d_pos.data_ptr(), lo, hi, d_e.data_ptr(), d_f.data_ptr(), handles[r], d_virial=wbufs[r].data_ptr())
            else:
                self.engines[r].gp_begin(d_pos.data_ptr(), lo, hi, d_e.data_ptr(), d_f.data_ptr(), handles[r])

        try:
            self._run_all(begin, range(g))
            self.n_exchanges = 0
            while True:
                steps = self._run_all(lambda r: self.engines[r].gp_step(), range(g))
                done = [s[2] for s in steps]
                if all(done):
                    break
                counts = {s[1] for s in steps}
                if any(done) or len(counts) != 1:
                    raise RuntimeError(f"local pool: the engines disagree at exchange point {self.n_exchanges} (done {done}, counts {sorted(counts)})")
                self._peer_sum([s[0] for s in steps], counts.pop(), self.devices, handles)
                self.n_exchanges += 1
        except BaseException:
            self._abandon()
            raise
        out = []
        for (dev, stream, _, d_e, d_f) in bufs:
            if stream is not None:
                stream.synchronize()
            out.append((d_e.cpu().numpy().copy(), d_f.cpu().numpy().copy()))
        self.last_all = out
        self.last_partials = [wb.cpu().numpy().copy() for wb in wbufs] if virial else None      # (behind the stream synchronisations above)
        e, f = out[0]
        if not np.isfinite(e).all():
            # energies are complete on every engine (node-level work is replicated): collect every sticky flag, then all widen together
            for eng in self.engines:
                eng.take_range_error()
            if not _retry and any([eng.widen("non-finite energy in a graph-parallel evaluation over the local pool") for eng in self.engines]):
                return self._graph_parallel(pos, forces, _retry=True, virial=virial)
            raise RuntimeError(f"non-finite energy in graph-parallel mode over the local pool (precision mode {self.precision_mode()}): "
                               "non-finite coordinates, or an overflow that wider forward planes cannot cure")
        if virial:
            w = self.last_partials[0].copy()
            for part in self.last_partials[1:]:         # engine order: float64 addition does not associate
                w = w + part
            return e, f[None], w.reshape(1, 3, 3)
        return e, (f[None] if forces else None)

    def _abandon(self) -> None:
        """An error between gp_begin and the last step: let the device drain so that no engine is left waiting on a peer's event
        (an evaluation left half-way is dropped by the engine's next gp_begin)."""
        for buf in self._gp_buf or []:
            if buf[1] is not None:
                try:
                    buf[1].synchronize()
                except Exception:       # noqa: BLE001 -- the original error is the one to report
                    pass
