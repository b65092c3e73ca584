"""Host logic of the in-process engine pool (``parallel.LocalEnginePool``) and of the calculator switch that builds it
(``UMAcore(workers=G)`` outside a process group, ``UMX_LOCAL_DEVICES``) on fake engines -- no GPU, no library call.

A fake engine's "energy" of an image is a function of the image alone, so a result in the wrong order, a block evaluated twice or an
image dropped shows; its graph-parallel side hands out a small CPU tensor per exchange point, which a fake peer sum adds in list order."""
import importlib
import threading
import time

import numpy as np
import pytest
import torch

from pdb2reaction_amd import parallel as P

U = importlib.import_module("pdb2reaction_amd.uma_pysis")

N_ATOMS = 4


def image_energy(p):
    return float(np.asarray(p, dtype=np.float64).sum()) * 3.0 + 1.0


class FakeEngine:
    N_EXCHANGES = 10

    def __init__(self, device=0, precision=None):
        self.device, self.precision = int(device), precision
        self.natoms, self.widened, self.closed = N_ATOMS, False, False
        self.calls = []                 # (thread name, number of images) of every batch call
        self.fail = None                # exception to raise from energy_forces
        self.delay = 0.0
        self.range_violation = False    # the next batch call "leaves the fp16 range": the engine widens itself, as Engine.energy_forces does
        self.ws_limit = None
        self.reserved = None
        self.system = None
        self.gp_calls = []
        self._gp = None

    def load_weights(self, w):
        self.weights = w

    def set_system(self, z, **kw):
        self.natoms, self.system = len(z), (list(z), kw)

    def set_workspace_limit(self, nbytes):
        self.ws_limit = int(nbytes)

    def reserve_images(self, n):
        self.reserved = int(n)

    def precision_mode(self):
        return "split-bf16" if self.widened else "split-f16"

    def widen(self, why=""):
        if self.widened:
            return False
        self.widened = True
        return True

    def take_range_error(self):
        return False

    def close(self):
        self.closed = True

    def energy_forces(self, p, forces=True):
        p = np.asarray(p, dtype=np.float32)
        if p.ndim == 2:
            p = p[None]
        self.calls.append((threading.current_thread().name, p.shape[0]))
        if self.delay:
            time.sleep(self.delay)
        if self.fail is not None:
            raise self.fail
        if self.range_violation:
            self.range_violation = False
            self.widened = True
        scale = 2.0 if self.widened else 1.0            # "another arithmetic": a result that mixes the two is visible
        e = np.array([image_energy(x) * scale for x in p], dtype=np.float64)
        return e, ((p * np.float32(-scale)) if forces else None)

    # graph-parallel side: partial sums = this engine's share of a per-atom constant
    def gp_begin(self, d_pos, lo, hi, d_e, d_f, stream=0):
        self.gp_calls.append((lo, hi))
        self._gp = {"at": 0, "lo": lo, "hi": hi, "buf": torch.zeros(self.natoms * 3, dtype=torch.float32)}

    def gp_step(self):
        g = self._gp
        if g["at"] == self.N_EXCHANGES:
            self._gp = None
            return 0, 0, True
        g["at"] += 1
        g["buf"].zero_()
        g["buf"][3 * g["lo"]: 3 * g["hi"]] = float(g["at"])
        return g["buf"].data_ptr(), g["buf"].numel(), False


def make_pool(g, **kw):
    engines = [FakeEngine(r) for r in range(g)]
    sums = []

    def fake_peer_sum(ptrs, count, devices, streams):
        live = [e._gp["buf"] for e in engines]
        assert [b.data_ptr() for b in live] == list(ptrs) and all(b.numel() == count for b in live)
        total = live[0].clone()
        for b in live[1:]:
            total += b
        for b in live:
            b.copy_(total)
        sums.append((count, list(devices), total.clone()))

    pool = P.LocalEnginePool(engines, peer_sum=fake_peer_sum, tensor_device=lambda e: torch.device("cpu"), **kw)
    return pool, engines, sums


def images(k, seed=0):
    return np.random.default_rng(seed).standard_normal((k, N_ATOMS, 3)).astype(np.float32)


@pytest.mark.parametrize("k,g", [(16, 8), (8, 8), (5, 3), (2, 3)])
def test_blocks_and_image_order(k, g):
    pool, engines, _ = make_pool(g)
    p = images(k, seed=k * 10 + g)
    for eng in engines:
        eng.delay = 0.05                                   # long enough for every engine's call to be in flight at once
    e, f = pool.energy_forces(p)
    assert pool.last_route == "batch"
    assert pool.last_blocks == [P.shard_bounds(k, g, r) for r in range(g)]
    assert pool.last_blocks[0][0] == 0 and pool.last_blocks[-1][1] == k
    assert all(pool.last_blocks[r][1] == pool.last_blocks[r + 1][0] for r in range(g - 1))           # contiguous, in order
    assert np.array_equal(e, np.array([image_energy(x) for x in p])) and e.dtype == np.float64
    assert np.array_equal(f, -p) and f.dtype == np.float32 and f.shape == (k, N_ATOMS, 3)
    for r, eng in enumerate(engines):
        lo, hi = pool.last_blocks[r]
        assert [c[1] for c in eng.calls] == ([hi - lo] if hi > lo else [])                           # an engine without images does nothing
    threads = {c[0] for eng in engines for c in eng.calls}
    assert len(threads) == min(k, g) and all(t.startswith("umx-pool") for t in threads)             # one host thread per engine with work
    e2, f2 = pool.energy_forces(p, forces=False)
    assert f2 is None and np.array_equal(e2, e)
    pool.close()
    assert all(eng.closed for eng in engines)


def test_one_image_takes_the_graph_parallel_route(monkeypatch):
    monkeypatch.delenv("UMX_WORKERS_GP", raising=False)
    pool, engines, sums = make_pool(3)
    p = images(1)
    pool.energy_forces(p)                                  # (1,N,3)
    assert pool.last_route == "graph-parallel" and pool.n_exchanges == FakeEngine.N_EXCHANGES == len(sums)
    assert [eng.gp_calls for eng in engines] == [[P.shard_bounds(N_ATOMS, 3, r)] for r in range(3)]
    assert all(not eng.calls for eng in engines)           # no batch call anywhere
    for i, (count, devices, total) in enumerate(sums):
        assert count == 3 * N_ATOMS and devices == [0, 1, 2]
        assert torch.equal(total, torch.full((3 * N_ATOMS,), float(i + 1)))      # every node summed exactly once per exchange
    assert len(pool.last_all) == 3
    pool.energy_forces(p[0])                               # (N,3) is one image too
    assert len(sums) == 2 * FakeEngine.N_EXCHANGES


def test_workers_gp_zero_keeps_single_images_on_engine_zero(monkeypatch):
    monkeypatch.setenv("UMX_WORKERS_GP", "0")
    pool, engines, sums = make_pool(3)
    p = images(1)
    e, f = pool.energy_forces(p)
    assert pool.last_route == "single" and not sums
    assert [len(eng.calls) for eng in engines] == [1, 0, 0] and not any(eng.gp_calls for eng in engines)
    assert e[0] == image_energy(p[0]) and f.shape == (1, N_ATOMS, 3)
    pool.energy_forces(images(4))                          # batches are dealt as usual
    assert pool.last_route == "batch"


def test_error_in_engine_one_is_raised_after_all_threads_ended():
    pool, engines, _ = make_pool(4)
    engines[1].fail = RuntimeError("engine one")
    engines[2].fail = ValueError("engine two")
    engines[0].delay = engines[3].delay = 0.3             # the healthy engines are still busy when the errors occur
    done = []
    real = FakeEngine.energy_forces

    def tracked(self, p, forces=True):
        try:
            return real(self, p, forces)
        finally:
            done.append(self.device)

    for eng in engines:
        eng.energy_forces = tracked.__get__(eng)
    with pytest.raises(RuntimeError, match="engine one"):                                          # the lowest failing engine index wins
        pool.energy_forces(images(8))
    assert sorted(done) == [0, 1, 2, 3]                                                            # every thread had ended by then
    for eng in engines:
        eng.fail, eng.delay = None, 0.0
    e, _ = pool.energy_forces(images(8))                                                            # the pool stays usable
    assert np.array_equal(e, np.array([image_energy(x) for x in images(8)]))


def test_widen_on_one_engine_widens_all_and_repeats_the_batch():
    pool, engines, _ = make_pool(3)
    engines[2].range_violation = True
    p = images(7)
    e, f = pool.energy_forces(p)
    assert all(eng.widened for eng in engines)
    assert [len(eng.calls) for eng in engines] == [2, 2, 2]                                        # the WHOLE batch again, on every engine
    assert np.array_equal(e, 2.0 * np.array([image_energy(x) for x in p])) and np.array_equal(f, -2.0 * p)    # one arithmetic throughout
    pool.energy_forces(p)
    assert [len(eng.calls) for eng in engines] == [3, 3, 3]                                        # once widened: one pass


def test_local_devices_parsing(monkeypatch):
    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,1,2,3")
    assert P.local_devices_for(4, device_count=lambda: 0) == [0, 1, 2, 3]
    monkeypatch.setenv("UMX_LOCAL_DEVICES", " 0,0 ")
    assert P.local_devices_for(2, device_count=lambda: 1) == [0, 0]                                # an ordinal may repeat
    with pytest.raises(ValueError, match=r"0,0.*2 device.*workers=3"):
        P.local_devices_for(3, device_count=lambda: 8)
    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,x")
    with pytest.raises(ValueError, match="UMX_LOCAL_DEVICES"):
        P.local_devices_for(2)
    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,-1")
    with pytest.raises(ValueError, match="non-negative"):
        P.local_devices_for(2)
    monkeypatch.delenv("UMX_LOCAL_DEVICES")
    assert P.local_devices_for(4, device_count=lambda: 8) == [0, 1, 2, 3]                          # the first G visible devices
    assert P.local_devices_for(4, device_count=lambda: 4) == [0, 1, 2, 3]
    assert P.local_devices_for(4, device_count=lambda: 3) is None                                  # too few: today's single engine
    assert P.local_devices_for(1, device_count=lambda: 8) is None


def test_engines_that_share_a_device_share_its_workspace_cap(monkeypatch):
    monkeypatch.delenv("UMX_WS_GB", raising=False)
    free = {0: 200 << 30, 1: 100 << 30}
    lims = P.shared_workspace_limits([0, 0, 1, 0], lambda d: free[d])
    assert lims == [(160 << 30) // 3] * 2 + [0] + [(160 << 30) // 3]           # the default 160 GiB cap (< 85 % of 200); 0: an engine alone keeps its own rule
    monkeypatch.setenv("UMX_WS_GB", "30")
    assert P.shared_workspace_limits([0, 0], lambda d: free[d]) == [15 << 30, 15 << 30]            # the explicit cap
    assert P.shared_workspace_limits([1, 1], lambda d: 20 << 30) == [int((20 << 30) * 0.85) // 2] * 2     # ... but never more than is there
    monkeypatch.setenv("UMX_WS_GB", "0")
    assert P.shared_workspace_limits([1, 1], lambda d: free[d]) == [int((100 << 30) * 0.85) // 2] * 2     # 0: the automatic 85 %
    monkeypatch.setenv("UMX_WS_GB", "30")
    pool = P.LocalEnginePool([FakeEngine(0), FakeEngine(0), FakeEngine(1)], free_bytes=lambda d: free[d])
    assert [e.ws_limit for e in pool.engines] == [15 << 30, 15 << 30, None]
    pool.reserve_images(8)
    assert [e.reserved for e in pool.engines] == [3, 3, 2]


def _fake_engine_module(monkeypatch):
    import pdb2reaction_amd.engine as E

    made = []

    class Recorded(FakeEngine):
        def __init__(self, device=0, precision=None):
            super().__init__(device, precision)
            made.append(self)

    monkeypatch.setattr(E, "Engine", Recorded)
    return made


def test_core_builds_a_pool_from_the_variable(monkeypatch):
    made = _fake_engine_module(monkeypatch)
    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,0")
    monkeypatch.setenv("UMX_WS_GB", "16")
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda d=None: (64 << 30, 64 << 30), raising=False)
    core = U.UMAcore(["O", "H", "H"], model="synthetic", workers=2)
    assert core.local_devices == [0, 0] and len(made) == 2 and core.engine is made[0] and core.parallel_predict
    assert [e.ws_limit for e in made] == [8 << 30, 8 << 30]
    assert all(e.system is not None and e.system[0] == [8, 1, 1] for e in made)                    # the same system on every engine
    r = core.compute_batch(np.zeros((4, 3, 3)) + np.arange(4)[:, None, None])
    assert r["energy"].shape == (4,) and [len(e.calls) for e in made] == [1, 1]
    core.close()
    assert all(e.closed for e in made)
    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,0,0")
    with pytest.raises(ValueError, match=r"3 device.*workers=2"):
        U.UMAcore(["O", "H", "H"], model="synthetic", workers=2)
    assert len(made) == 2                                                                           # refused before any engine exists


def test_fewer_devices_than_workers_keeps_one_engine(monkeypatch, recwarn):
    made = _fake_engine_module(monkeypatch)
    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    core = U.UMAcore(["O", "H", "H"], model="synthetic", workers=8)
    assert len(made) == 1 and core.local_devices == [0] and len(core.local_devices) == 1
    assert core._pool is None and core.parallel_predict and core.engine is made[0]                  # today's behaviour, side effect included
    assert not [w for w in recwarn.list if "worker" in str(w.message).lower()]                     # nothing new warned
    core.compute_batch(np.zeros((4, 3, 3)))
    assert [c[1] for c in made[0].calls] == [4]
    # enough devices: the first G
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 4)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda d=None: (1 << 30, 1 << 30), raising=False)
    core = U.UMAcore(["O", "H", "H"], model="synthetic", workers=3)
    assert core.local_devices == [0, 1, 2] and [e.device for e in made[1:]] == [0, 1, 2]
