"""The pinned neighbour graph without a GPU: the C ABI's declarations against the ctypes binding, and the Python layers above the engine
(``uma_pysis(hessian_pin_graph=True)``, ``LocalEnginePool.pin_graph``) against stub engines.  The last test is a YARDSTICK ONLY: it runs
the float64 checker alone and passes with or without the feature."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import pinned_cases as PC
from pdb2reaction_amd import parallel as P
from pdb2reaction_amd import synth

U = importlib.import_module("pdb2reaction_amd.uma_pysis")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_the_four_exports_and_their_ctypes_signatures():
    from pdb2reaction_amd import engine as E

    lib = E.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "umx.h")).read(), flags=re.S)
    vp, fp, dp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    decl = {
        "umx_pin_graph": r"int\s+umx_pin_graph\s*\(\s*umx_engine\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*\)",
        "umx_pin_graph_f64": r"int\s+umx_pin_graph_f64\s*\(\s*umx_engine\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*\)",
        "umx_unpin_graph": r"int\s+umx_unpin_graph\s*\(\s*umx_engine\s*\*\s*\w+\s*\)",
        "umx_pinned_graph": r"int\s+umx_pinned_graph\s*\(\s*const\s+umx_engine\s*\*\s*\w+\s*,\s*int64_t\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)",
    }
    for sym, pattern in decl.items():
        assert re.search(pattern, txt), sym
        assert hasattr(lib, sym) and sym in (E.EXPORTED_SYMBOLS_F64 if sym.endswith("f64") else E.EXPORTED_SYMBOLS)
    assert lib.umx_abi_version() == 10                                       # additive: no version bump
    assert lib.umx_pin_graph.argtypes == [vp, fp] and lib.umx_pin_graph_f64.argtypes == [vp, dp]
    assert lib.umx_unpin_graph.argtypes == [vp]
    assert lib.umx_pinned_graph.argtypes == [vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)]
    # no engine: refused, not a crash
    assert lib.umx_pin_graph(None, None) != 0 and lib.umx_pin_graph_f64(None, None) != 0
    assert lib.umx_unpin_graph(None) != 0 and lib.umx_pinned_graph(None, None, None) != 0
    for name in ("pin_graph", "unpin_graph", "pinned_graph", "pinned"):
        assert callable(getattr(E.Engine, name)) and callable(getattr(P.LocalEnginePool, name))


# ---- uma_pysis.get_hessian ---------------------------------------------------------------------------------------------------------------
class _PinEngine:
    """Records pin / unpin and every batch, in order."""

    def __init__(self, log, name="e"):
        self.log, self.name, self.device, self.natoms, self.widened = log, name, 0, 3, False

    def pin_graph(self, pos, **kw):
        self.log.append((self.name, "pin", np.array(pos, dtype=np.float64), kw))

    def unpin_graph(self):
        self.log.append((self.name, "unpin"))


class _Core:
    parallel_predict, has_torch_model, _gp, _pool = False, False, None, None
    device = torch.device("cpu")

    def __init__(self, log, fail_at=None):
        self.log, self.engine, self.fail_at, self.batches = log, _PinEngine(log), fail_at, 0

    def compute(self, coord_ang, *, forces=False, hessian=False):
        self.log.append(("core", "base"))
        return {"energy": 1.0, "forces": np.zeros((3, 3), np.float32), "hessian": None}

    def compute_batch(self, coords_ang, *, forces=True):
        self.log.append(("core", "batch", len(coords_ang)))
        self.batches += 1
        if self.fail_at == self.batches:
            raise RuntimeError("the batch call failed")
        c = np.asarray(coords_ang, dtype=np.float64)
        return {"energy": np.zeros(len(c)), "forces": (-2.0 * c).astype(np.float32)}     # E = |x|^2: the Hessian is 2


def _calc(log, fail_at=None, **kw):
    calc = U.uma_pysis(model="synthetic", **kw)
    calc._core = _Core(log, fail_at)
    return calc


X = np.array([[0.0, 0.0, 0.0], [1.1, 0.1, 0.0], [-0.3, 0.9, 0.4]])


def test_get_hessian_pins_evaluates_and_unpins_in_that_order():
    log = []
    calc = _calc(log, hessian_pin_graph=True, out_hess_torch=False)
    out = calc.get_hessian(["C", "H", "O"], X.reshape(-1) * U.ANG2BOHR)
    kinds = [entry[:2] for entry in log]
    assert kinds == [("core", "base"), ("e", "pin"), ("core", "batch"), ("e", "unpin")]
    assert np.allclose(log[1][2], X, atol=1e-12) and log[1][3] == {}          # pinned at the geometry it was given
    h = np.asarray(out["hessian"]).reshape(9, 9)
    assert np.allclose(h, 2.0 * np.eye(9) * U.H_EVAA_2_AU, atol=1e-3 * U.H_EVAA_2_AU)           # (float32 forces over 2h)
    # without the keyword nothing is pinned, and the keyword never reaches the core's constructor
    log2 = []
    _calc(log2, out_hess_torch=False).get_hessian(["C", "H", "O"], X.reshape(-1) * U.ANG2BOHR)
    assert [entry[:2] for entry in log2] == [("core", "base"), ("core", "batch")]
    assert "hessian_pin_graph" not in calc._core_kw
    # double positions: the pin takes the float64 geometry through the float64 entry
    log3 = []
    _calc(log3, hessian_pin_graph=True, double_positions=True, out_hess_torch=False).get_hessian(["C", "H", "O"], X.reshape(-1) * U.ANG2BOHR)
    assert log3[1][:2] == ("e", "pin") and log3[1][3] == {"double_positions": True}


def test_get_hessian_unpins_when_the_batch_call_raises():
    log = []
    calc = _calc(log, fail_at=1, hessian_pin_graph=True)
    with pytest.raises(RuntimeError, match="the batch call failed"):
        calc.get_hessian(["C", "H", "O"], X.reshape(-1) * U.ANG2BOHR)
    assert [entry[:2] for entry in log] == [("core", "base"), ("e", "pin"), ("core", "batch"), ("e", "unpin")]


def test_hessian_pin_graph_with_the_graph_parallel_mode_raises():
    log = []
    calc = _calc(log, hessian_pin_graph=True)
    calc._core._gp = object()                                                # the core evaluates graph-parallel
    with pytest.raises(ValueError, match="graph-parallel"):
        calc.get_hessian(["C", "H", "O"], X.reshape(-1) * U.ANG2BOHR)
    assert log == []                                                         # refused before anything was evaluated or pinned
    calc._core._gp = None
    calc._core.enable_graph_parallel = lambda on, group=None: log.append("enabled")
    with pytest.raises(ValueError, match="graph-parallel"):
        calc.enable_graph_parallel(["C", "H", "O"], True)
    assert log == []


# ---- LocalEnginePool ---------------------------------------------------------------------------------------------------------------------
class _PoolEngine(_PinEngine):
    def __init__(self, log, name, device, refuse=False):
        super().__init__(log, name)
        self.device, self.refuse = device, refuse

    def pin_graph(self, pos, **kw):
        if self.refuse:
            raise RuntimeError("refused")
        super().pin_graph(pos, **kw)

    def set_system(self, z, **kw):
        self.natoms = len(z)

    def energy_forces(self, p, forces=True, **kw):
        self.log.append((self.name, "eval", len(p)))
        return np.zeros(len(p)), np.zeros(np.shape(p), np.float32)

    def close(self):
        pass


def _pool(log, refuse_last=False):
    engines = [_PoolEngine(log, f"e{r}", r, refuse=refuse_last and r == 2) for r in range(3)]
    return P.LocalEnginePool(engines, gp=True, peer_sum=lambda *a: None, tensor_device=lambda e: torch.device("cpu"))


def test_the_pool_forwards_to_every_engine_and_routes_a_single_geometry_to_engine_0():
    log = []
    pool = _pool(log)
    try:
        pool.natoms = 3
        went_gp = []
        pool._graph_parallel = lambda p, forces, **kw: went_gp.append(1) or (np.zeros(1), np.zeros((1, 3, 3), np.float32))
        pool.energy_forces(X)
        assert went_gp == [1] and pool.last_route != "single"               # nothing pinned: a single geometry goes graph-parallel
        assert pool.pinned_graph() is None
        pool.pin_graph(X)
        assert [entry[:2] for entry in log] == [("e0", "pin"), ("e1", "pin"), ("e2", "pin")]
        pool.energy_forces(X)
        assert went_gp == [1] and pool.last_route == "single" and log[-1] == ("e0", "eval", 1)
        pool.energy_forces(np.stack([X] * 4))                                # a batch is dealt as ever
        assert pool.last_route == "batch"
        with pytest.raises(ValueError, match="pinned"):
            pool.energy_forces_virial(X, graph_parallel=True)
        del log[:]
        pool.unpin_graph()
        assert log == [("e0", "unpin"), ("e1", "unpin"), ("e2", "unpin")]
        pool.energy_forces(X)
        assert went_gp == [1, 1]
        # the with block unpins on an exception; set_system drops the pool's own mark
        del log[:]
        with pytest.raises(KeyError):
            with pool.pinned(X, double_positions=True):
                assert log[0][3] == {"double_positions": True}
                raise KeyError("inside")
        assert [entry[:2] for entry in log][-3:] == [("e0", "unpin"), ("e1", "unpin"), ("e2", "unpin")]
        pool.pin_graph(X)
        pool.set_system([6, 1, 8])
        pool.energy_forces(X)
        assert went_gp == [1, 1, 1]
    finally:
        pool.close()


def test_a_refusing_engine_leaves_the_pool_unpinned():
    log = []
    pool = _pool(log, refuse_last=True)
    try:
        with pytest.raises(RuntimeError, match="refused"):
            pool.pin_graph(X)
        assert [entry[:2] for entry in log] == [("e0", "pin"), ("e1", "pin"), ("e0", "unpin"), ("e1", "unpin")]
        assert pool.pinned_graph() is None
    finally:
        pool.close()


# ---- yardstick only: passes with or without the feature ---------------------------------------------------------------------------------
def test_yardstick_only_the_checkers_fixed_graph_fd_hessian_against_its_autograd_hessian(weights):
    """YARDSTICK ONLY (no engine code runs).  8 atoms, ``max_neigh = 4``: the float64 checker's central-difference Hessian on the graph
    of the base geometry held fixed (h = 1e-3 A, the calculator's step) against its float64 autograd Hessian on the same graph.
    Measured (profiles/pinned_graph.txt): max|H_fd - H_ad| = 5.2e-5 eV/A^2 at max|H| = 3.4 eV/A^2, autograd asymmetry 4e-16.  Bound: the
    central difference's truncation h^2 / 6 |d^3 F / dx^3| with third derivatives of the forces below 600 eV/A^4, i.e. 1e-4 eV/A^2
    (the measured figure corresponds to 310 eV/A^4); float64 roundoff (1e-13 eV/A over 2h) is far below it."""
    z, pos = synth.make_cluster(8, seed=5)
    x0 = pos.astype(np.float32).astype(np.float64)
    orc = PC.checker(weights)
    g0 = PC.graph_of(orc, x0)
    zt = torch.as_tensor(z, dtype=torch.long)
    rmsd = float(orc.p["normalizer.rmsd"][0])
    h_ad = torch.autograd.functional.hessian(lambda p: orc.model_energy(zt, p.reshape(8, 3), graph=g0) * rmsd,
                                             torch.as_tensor(x0.reshape(-1))).numpy()
    h_fd = np.zeros((24, 24))
    for k in range(24):
        xp, xm = x0.copy().reshape(-1), x0.copy().reshape(-1)
        xp[k] += PC.FD_H
        xm[k] -= PC.FD_H
        fp = PC.energy_forces_on(orc, z, xp.reshape(8, 3), g0)[1].reshape(-1)
        fm = PC.energy_forces_on(orc, z, xm.reshape(8, 3), g0)[1].reshape(-1)
        h_fd[:, k] = -(fp - fm) / (2 * PC.FD_H)
    asym, dev = np.abs(h_ad - h_ad.T).max(), np.abs(h_fd - h_ad).max()
    print(f"[yardstick] autograd asymmetry {asym:.2e}  max|H_fd - H_ad| = {dev:.3e} eV/A^2  max|H| = {np.abs(h_ad).max():.3f}")
    assert asym <= 1e-12 and dev <= 1e-4
