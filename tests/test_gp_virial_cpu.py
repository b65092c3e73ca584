"""Host logic of the graph-parallel virial (``umx_gp_begin_virial``) above the library, on fake engines -- no GPU, no library call.

1. the pool's default route for a single geometry with a virial is engine 0 alone, as before;
2. ``graph_parallel=True`` hands every engine a virial pointer through ``gp_begin`` and adds the engines' shares in engine order in
   float64 -- held, bit for bit, to ``np.add`` in that order (the shares are chosen so that another order gives other bits);
3. the opt-in raises ``ValueError`` with recompute mode 2 and leaves batches alone;
4. ``UMXCalculator(gp_stress=...)`` forwards the opt-in to a pool and to nothing else;
5. ``GraphParallelEvaluator(virial=True)`` without a process group returns the engine's own share, and ``virial=False`` calls
   ``gp_begin`` as it always did;
6. the new entry is declared, exported and bound.

The fake engine of tests/test_local_pool_cpu.py is reused: its ``gp_begin`` takes no virial pointer, which is what the default route
and ``virial=False`` are held to (a stray keyword would be a ``TypeError``)."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from pdb2reaction_amd import parallel as P
from test_local_pool_cpu import FakeEngine, N_ATOMS, images

A = importlib.import_module("pdb2reaction_amd.ase_calculator")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# shares whose float64 sum depends on the order: (a + b) + c != a + (b + c) != (c + b) + a component by component
SHARES = [np.array([1.0e16, 1.0, -3.0, 0.1, 1e-17, 2.0 ** 53, 7.0, -1.0e16, 0.3]),
          np.array([1.0, 1.0e16, 0.2, 0.2, 1.0, 1.0, -7.0, 1.0, 0.6]),
          np.array([-1.0e16, -1.0e16, 1e-16, 0.3, -1.0, 1.0, 1e-16, 1.0e16, -0.9])]


class VirialFake(FakeEngine):
    """The fake engine with the virial side of ``Engine.gp_begin``: the share is written where the pointer says, at the last step."""

    def __init__(self, device=0, precision=None):
        super().__init__(device, precision)
        self.virial_ptrs, self.virial_calls, self.recompute_seen = [], [], None

    def gp_begin(self, d_pos, lo, hi, d_e, d_f, stream=0, d_virial=0):
        super().gp_begin(d_pos, lo, hi, d_e, d_f, stream)
        self.virial_ptrs.append(int(d_virial))
        self._gp["w"] = int(d_virial)
        (ctypes.c_double * 1).from_address(d_e)[0] = 5.0

    def gp_step(self):
        g = self._gp
        if g["at"] == self.N_EXCHANGES and g["w"]:
            (ctypes.c_double * 9).from_address(g["w"])[:] = list(SHARES[self.device] * (1.0 + g["lo"]))
        return super().gp_step()

    def energy_forces_virial(self, p):
        p = np.asarray(p, dtype=np.float32)
        self.virial_calls.append(len(p))
        return np.full(len(p), 2.0), -p, np.full((len(p), 3, 3), 10.0 + self.device)

    def set_recompute(self, mode):
        self.recompute_seen = int(mode)

    def cell_volume(self):
        return 210.0


def make_pool(g, cls=VirialFake, **kw):
    engines = [cls(r) for r in range(g)]

    def fake_peer_sum(ptrs, count, devices, streams):
        live = [e._gp["buf"] for e in engines]
        total = live[0].clone()
        for b in live[1:]:
            total += b
        for b in live:
            b.copy_(total)

    return P.LocalEnginePool(engines, peer_sum=fake_peer_sum, tensor_device=lambda e: torch.device("cpu"), **kw), engines


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_default_route_of_a_single_geometry_is_unchanged():
    pool, engines = make_pool(3)
    p = images(1)
    e, f, w = pool.energy_forces_virial(p)
    assert pool.last_route == "single" and pool.last_blocks == [(0, 1)]
    assert [eng.virial_calls for eng in engines] == [[1], [], []] and not any(eng.gp_calls for eng in engines)
    assert w.shape == (1, 3, 3) and (w == 10.0).all()
    pool.energy_forces_virial(p[0], graph_parallel=False)
    assert pool.last_route == "single" and engines[0].virial_calls == [1, 1] and not any(eng.gp_calls for eng in engines)
    # the plain graph-parallel route still calls gp_begin as it always did (the base fake takes no virial pointer)
    plain, plain_engines = make_pool(3, cls=FakeEngine)
    plain.energy_forces(p)
    assert plain.last_route == "graph-parallel" and plain.last_partials is None
    assert all(len(eng.gp_calls) == 1 for eng in plain_engines)
    pool.close(); plain.close()


@pytest.mark.parametrize("g", [2, 3])
def test_opt_in_adds_the_engines_shares_in_engine_order(g):
    pool, engines = make_pool(g)
    p = images(1, seed=g)
    e, f, w = pool.energy_forces_virial(p, graph_parallel=True)
    assert pool.last_route == "graph-parallel" and pool.n_exchanges == FakeEngine.N_EXCHANGES
    assert pool.last_blocks == [P.shard_bounds(N_ATOMS, g, r) for r in range(g)]
    assert [eng.gp_calls for eng in engines] == [[P.shard_bounds(N_ATOMS, g, r)] for r in range(g)]
    ptrs = [eng.virial_ptrs for eng in engines]
    assert all(len(q) == 1 and q[0] != 0 for q in ptrs) and len({q[0] for q in ptrs}) == g        # a pointer of its own on every engine
    assert not any(eng.virial_calls for eng in engines)                                           # no one-engine call anywhere
    shares = [SHARES[r] * (1.0 + pool.last_blocks[r][0]) for r in range(g)]
    assert len(pool.last_partials) == g and all(same_bits(pool.last_partials[r], shares[r]) for r in range(g))
    want = shares[0].copy()
    for s in shares[1:]:
        want = np.add(want, s)
    assert e.shape == (1,) and e[0] == 5.0 and f.shape == (1, N_ATOMS, 3) and w.shape == (1, 3, 3) and w.dtype == np.float64
    assert same_bits(w[0], want.reshape(3, 3))
    if g == 3:                                              # the shares make the order visible: right to left gives other bits
        other = np.add(np.add(shares[2], shares[1]), shares[0])
        assert not same_bits(other, want)
    e2, f2, w2 = pool.energy_forces_virial(p[0], graph_parallel=True)                             # (N,3) is one image too; same bits again
    assert same_bits(w2, w)
    e3, f3, s3 = pool.energy_forces_stress(p, graph_parallel=True)
    assert pool.last_route == "graph-parallel" and s3.shape == (1, 6)
    sym = 0.5 * (w[0] + w[0].T) / 210.0
    assert same_bits(s3[0], np.array([sym[0, 0], sym[1, 1], sym[2, 2], sym[1, 2], sym[0, 2], sym[0, 1]]))
    pool.close()


def test_batches_and_one_engine_pools_ignore_the_opt_in():
    pool, engines = make_pool(3)
    e, f, w = pool.energy_forces_virial(images(5), graph_parallel=True)
    assert pool.last_route == "batch" and w.shape == (5, 3, 3) and not any(eng.gp_calls for eng in engines)
    assert [eng.virial_calls for eng in engines] == [[hi - lo] for lo, hi in pool.last_blocks]
    pool.close()
    one, (eng,) = make_pool(1)
    one.energy_forces_virial(images(1), graph_parallel=True)
    assert one.last_route == "single" and eng.virial_calls == [1] and not eng.gp_calls
    one.close()


def test_opt_in_with_recompute_mode_two_is_refused():
    pool, engines = make_pool(2)
    pool.set_recompute(2)
    assert [eng.recompute_seen for eng in engines] == [2, 2]
    with pytest.raises(ValueError, match="recompute mode 2"):
        pool.energy_forces_virial(images(1), graph_parallel=True)
    with pytest.raises(ValueError, match="recompute mode 2"):
        pool.energy_forces_stress(images(1), graph_parallel=True)
    assert not any(eng.gp_calls or eng.virial_calls for eng in engines)                           # refused, not routed elsewhere
    pool.energy_forces_virial(images(1))                                                          # the default still runs on engine 0
    assert pool.last_route == "single" and engines[0].virial_calls == [1]
    pool.energy_forces_virial(images(4), graph_parallel=True)                                     # and batches are untouched
    assert pool.last_route == "batch"
    pool.set_recompute(1)
    pool.energy_forces_virial(images(1), graph_parallel=True)
    assert pool.last_route == "graph-parallel"
    pool.close()


# ---- the facade ------------------------------------------------------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.kw, self.natoms = [], 0

    def set_system(self, z, **kw):
        self.natoms = len(z)

    def set_cell(self, cell=None, pbc=None):
        pass

    def energy_forces_stress(self, pos, **kw):
        self.kw.append(kw)
        p = np.asarray(pos, dtype=np.float64)
        return np.full(len(p), 3.0), np.ones_like(p), np.zeros((len(p), 6))

    def close(self):
        pass


class _Atoms:
    def __init__(self, pos):
        self.numbers, self._pos, self.info = np.array([8, 1, 1]), np.asarray(pos, dtype=np.float64), {}
        self.cell, self.pbc = np.diag([5.0, 6.0, 7.0]), True

    def get_positions(self):
        return self._pos


POS3 = np.array([[0.0, 0, 0], [0.96, 0, 0], [-0.3, 0.9, 0]])


@pytest.mark.parametrize("gp_stress,devices,want", [(True, [0, 0], {"graph_parallel": True}), (False, [0, 0], {}), (True, [0], {}),
                                                    (True, None, {})])
def test_facade_forwards_gp_stress_to_a_pool_only(monkeypatch, gp_stress, devices, want):
    from pdb2reaction_amd import weights as W

    monkeypatch.setattr(W, "check_merged_for", lambda *a, **k: None)
    c = A.UMXCalculator(model="synthetic", stress=True, workers=2, gp_stress=gp_stress)
    assert c.gp_stress is gp_stress
    c._engine, c._weights, c.local_devices = _Recorder(), None, devices
    c.get_stress(_Atoms(POS3))
    c.calculate_images([_Atoms(POS3 + 0.1)], stress=True)
    assert c._engine.kw == [want, want]
    assert A.UMXCalculator(model="synthetic").gp_stress is False                                  # off by default


# ---- the rank-level evaluator without a process group ----------------------------------------------------------------------------------
def test_evaluator_virial_keyword(monkeypatch):
    class Stream:
        cuda_stream = 0

    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: Stream())
    dev = torch.device("cpu")
    pos = torch.zeros(N_ATOMS, 3)
    eng = VirialFake(0)
    gp = P.GraphParallelEvaluator(eng, N_ATOMS, dev, virial=True)
    e, f, w = gp(pos)
    assert eng.gp_calls == [(0, N_ATOMS)] and eng.virial_ptrs[0] == gp._w.data_ptr() != 0
    assert w.shape == (3, 3) and w.dtype == torch.float64 and same_bits(w.numpy(), SHARES[0].reshape(3, 3))
    assert gp.last_partials.shape == (1, 9) and gp.n_exchanges == FakeEngine.N_EXCHANGES
    plain = FakeEngine(0)                                  # takes no virial pointer: virial=False is the old call
    plain_gp = P.GraphParallelEvaluator(plain, N_ATOMS, dev)
    out = plain_gp(pos)
    assert len(out) == 2 and plain_gp._w is None and plain.gp_calls == [(0, N_ATOMS)]


# ---- the C ABI and its binding -----------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_exported_and_bound():
    from pdb2reaction_amd import engine as E

    lib = E.load_library()
    txt = open(os.path.join(ROOT, "include", "umx.h")).read()
    assert "umx_gp_begin_virial(" in txt and "umx_gp_begin_virial" in E.EXPORTED_SYMBOLS and hasattr(lib, "umx_gp_begin_virial")
    assert "IN RANK ORDER" in txt                                                                  # whose job the sum is, and in which order
    assert lib.umx_abi_version() == 10                                                            # additive: no version bump
    assert lib.umx_gp_begin_virial(None, None, 0, 0, None, None, None, None) != 0                 # no engine: refused, not a crash
    assert len(lib.umx_gp_begin_virial.argtypes) == len(lib.umx_gp_begin.argtypes) + 1
    calls = []

    class Lib:
        def umx_gp_begin(self, *a):
            calls.append(("plain", len(a)))
            return 0

        def umx_gp_begin_virial(self, *a):
            calls.append(("virial", len(a), a[6].value))
            return 0

    eng = object.__new__(E.Engine)
    eng.lib, eng._h = Lib(), ctypes.c_void_p()
    eng.gp_begin(16, 0, 4, 32, 48)
    eng.gp_begin(16, 0, 4, 32, 48, 7, d_virial=0)
    eng.gp_begin(16, 0, 4, 32, 48, 7, d_virial=64)
    assert calls == [("plain", 7), ("plain", 7), ("virial", 8, 64)]
    eng._h = None                                           # (nothing to destroy)
