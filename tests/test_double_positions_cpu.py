"""CPU tests of the float64-position path (``umx_energy_forces_f64[_dev]``, ``double_positions=True``): the exports, the way the flag
travels from ``uma_pysis``, ``UMXCalculator``, ``LocalEnginePool`` and ``hessian.fd_hessian`` down to the engine's entry -- against stub
engines and the toy core -- and a numpy restatement of the edge-vector rule the GPU tests rest on.  With the flag off every layer must
make exactly the call it made before the keyword existed (the stubs here take no such keyword).  The kernels are covered by
tests/test_gpu_double_positions.py."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from toy_core import ToyPairCore, toy_geometry
from pdb2reaction_amd import hessian as H
from pdb2reaction_amd import synth, weights as W

A = importlib.import_module("pdb2reaction_amd.ase_calculator")
U = importlib.import_module("pdb2reaction_amd.uma_pysis")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T = np.array([1024.0, -2048.0, 512.0])
Q = 2.0 ** -20


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_exported_and_refuse_a_null_engine():
    from pdb2reaction_amd import engine as E

    lib = E.load_library()
    txt = open(os.path.join(ROOT, "include", "umx.h")).read()
    dp, fp, vp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.c_void_p
    for sym in ("umx_energy_forces_f64", "umx_energy_forces_f64_dev"):
        assert sym + "(" in txt and sym in E.EXPORTED_SYMBOLS_F64 and hasattr(lib, sym)
    assert lib.umx_abi_version() == 10                                       # additive: no version bump
    assert lib.umx_energy_forces_f64.argtypes == [vp, ctypes.c_int, dp, dp, fp, dp]
    assert lib.umx_energy_forces_f64_dev.argtypes == [vp, ctypes.c_int, vp, vp, vp, vp, vp]
    pos, e = np.zeros((1, 2, 3)), np.zeros(1)
    assert lib.umx_energy_forces_f64(None, 1, pos.ctypes.data_as(dp), e.ctypes.data_as(dp), None, None) != 0      # refused, not a crash
    assert lib.umx_energy_forces_f64_dev(None, 1, None, None, None, None, None) != 0
    assert "umx_gp_begin[_virial] stay float32" in txt                       # what is not provided is said


# ---- Engine, without a device --------------------------------------------------------------------------------------------------------
class _Lib:
    """The three host entries of libumx, recording which one ran on what."""

    def __init__(self):
        self.calls = []

    def _entry(self, name, ctype):
        def fn(h, k, pos, e, f, *w):
            self.calls.append((name, pos._type_, k, f is not None, bool(w) and w[0] is not None))
            assert pos._type_ is ctype
            return 0
        return fn

    def __getattr__(self, name):
        if name in ("umx_energy_forces", "umx_energy_forces_virial"):
            return self._entry(name, ctypes.c_float)
        if name == "umx_energy_forces_f64":
            return self._entry(name, ctypes.c_double)
        raise AttributeError(name)


def test_engine_picks_the_entry_by_the_flag():
    from pdb2reaction_amd import engine as E

    eng = object.__new__(E.Engine)
    eng.lib, eng._h, eng.natoms = _Lib(), None, 4
    x = np.random.default_rng(0).normal(size=(2, 4, 3)) + T
    e, f = eng.energy_forces(x)
    assert f.dtype == np.float32 and f.shape == (2, 4, 3) and e.dtype == np.float64
    eng.energy_forces(x, forces=False)
    eng.energy_forces_virial(x)
    eng.energy_forces(x, double_positions=True)
    eng.energy_forces(x[0], forces=False, double_positions=True)
    e, f, w = eng.energy_forces_virial(x, double_positions=True)
    assert f.dtype == np.float32 and w.shape == (2, 3, 3) and w.dtype == np.float64
    cf, cd = ctypes.c_float, ctypes.c_double
    assert eng.lib.calls == [("umx_energy_forces", cf, 2, True, False), ("umx_energy_forces", cf, 2, False, False),
                             ("umx_energy_forces_virial", cf, 2, True, True), ("umx_energy_forces_f64", cd, 2, True, False),
                             ("umx_energy_forces_f64", cd, 1, False, False), ("umx_energy_forces_f64", cd, 2, True, True)]
    with pytest.raises(ValueError, match="positions must be"):
        eng.energy_forces(x[:, :3], double_positions=True)
    # the stress follows: the keyword goes down only when it is set
    eng._cell, eng._cells = (np.eye(3) * 9.0, (True, True, True)), None
    seen = []
    eng.energy_forces_virial = lambda pos, **kw: seen.append(kw) or (np.zeros(2), np.zeros((2, 4, 3), np.float32), np.zeros((2, 3, 3)))
    eng.energy_forces_stress(x)
    eng.energy_forces_stress(x, double_positions=True)
    assert seen == [{}, {"double_positions": True}]


# ---- uma_pysis and the toy core -----------------------------------------------------------------------------------------------------
def test_uma_pysis_hands_the_flag_to_its_core(monkeypatch):
    made = []

    class Core(ToyPairCore):
        def __init__(self, elem, **kw):
            made.append(kw)
            super().__init__(len(elem))

    monkeypatch.setattr(U, "UMAcore", Core)
    elem, x = ["C", "H", "O"], toy_geometry(3)
    U.uma_pysis().get_energy(elem, x * U.ANG2BOHR)
    U.uma_pysis(double_positions=True).get_energy(elem, x * U.ANG2BOHR)
    assert "double_positions" not in made[0] and made[1]["double_positions"] is True      # the default core sees the reference's keywords only


class _RecordingEngine:
    natoms = 3

    def __init__(self):
        self.calls = []

    def energy_forces(self, pos, forces=True, **kw):
        p = np.asarray(pos)
        self.calls.append((p.dtype, p.shape, kw))
        return np.zeros(len(p)), np.zeros(p.shape, np.float32)


def _core(flag):
    core = object.__new__(U.UMAcore)
    core.z, core._gp, core._pool, core.engine, core.double_positions = np.array([6, 1, 8]), None, None, _RecordingEngine(), flag
    return core


def test_umacore_passes_float64_through_when_the_flag_is_set():
    x = toy_geometry(3) + T
    for flag, kw in ((False, {}), (True, {"double_positions": True})):
        core = _core(flag)
        core.compute(x, forces=True)
        core.compute_batch(np.stack([x, x]), forces=True)
        assert core.engine.calls == [(np.dtype(np.float64), (1, 3, 3), kw), (np.dtype(np.float64), (2, 3, 3), kw)]
        # the device entry holds the tensor's dtype to the flag, before anything touches a GPU
        wrong = torch.zeros(2, 3, 3, dtype=torch.float32 if flag else torch.float64)
        with pytest.raises(TypeError, match="double_positions"):
            core.compute_batch_dev(wrong)
    with pytest.raises(ValueError, match="float32 positions only"):
        _core(True).enable_graph_parallel(True)


def test_fd_hessian_keeps_float64_displacements_when_asked():
    n = 3
    core = ToyPairCore(n)
    x = toy_geometry(n) + T
    host, dev = [], []

    def batch_forces(c):
        host.append(np.asarray(c).dtype)
        return core.compute_batch(c)["forces"]

    def batch_forces_dev(c):
        dev.append((c.dtype, c.detach().clone()))
        return torch.from_numpy(core.compute_batch(c.numpy())["forces"])

    kw = dict(device=torch.device("cpu"), double=True, partial=False)
    h_host = H.fd_hessian(batch_forces, x, [], **kw)
    assert host and all(d == np.float64 for d in host)                       # the host form hands down what it always did
    H.fd_hessian(batch_forces, x, [], batch_forces_dev=batch_forces_dev, **kw)
    assert dev and all(d == torch.float32 for d, _ in dev)                   # default: rounded to the model's float32 positions
    del dev[:]
    h_dev = H.fd_hessian(batch_forces, x, [], batch_forces_dev=batch_forces_dev, double_positions=True, **kw)
    assert dev and all(d == torch.float64 for d, _ in dev)
    c = dev[0][1].reshape(-1, 3 * n)
    assert c.shape[0] == 2 * 3 * n
    # the realised displacement is the step to float64's rounding at 2048 A, not to half a float32 ulp (1.2e-4 A there)
    assert float((c[0::2] - c[1::2]).abs().max() - 2 * H.FD_STEP_ANG) < 1e-12
    assert torch.equal(h_dev, h_host)                                        # the toy core rounds to float32 itself: the same columns
    host.clear()
    H.fd_hessian(batch_forces, x, [], double_positions=True, **kw)
    assert host and all(d == np.float64 for d in host)


def test_get_hessian_on_the_toy_core_with_and_without_the_flag():
    """The default path is unchanged, and the flag changes nothing for a core that rounds to float32 itself."""
    n = 3
    elem, x = ["C", "H", "O"], toy_geometry(n)
    out = []
    for kw in ({}, {"double_positions": True}):
        calc = U.uma_pysis(out_hess_torch=False, **kw)
        calc._core = ToyPairCore(n, has_torch_model=False)
        out.append(calc.get_hessian(elem, (x * U.ANG2BOHR).reshape(-1)))
        assert all(s.dtype == np.float64 for s in calc._core.seen)
    assert np.array_equal(out[0]["hessian"], out[1]["hessian"]) and out[0]["energy"] == out[1]["energy"]


# ---- the calculator facade against a stub engine ---------------------------------------------------------------------------------------
class _StubEngine:
    def __init__(self):
        self.log, self.natoms = [], 0

    def set_system(self, z, **kw):
        self.natoms = len(z)

    def set_cell(self, cell=None, pbc=None):
        pass

    def set_cells(self, cells=None, pbc=None):
        pass

    def energy_forces(self, pos, forces=True, **kw):
        p = np.asarray(pos)
        self.log.append(("ef", p.dtype, kw))
        return np.arange(len(p), dtype=np.float64), np.ones(p.shape, np.float32)

    def energy_forces_stress(self, pos, **kw):
        p = np.asarray(pos)
        self.log.append(("efs", p.dtype, kw))
        return np.arange(len(p), dtype=np.float64), np.ones(p.shape, np.float32), np.tile(np.arange(6.0), (len(p), 1))

    def close(self):
        pass


class _Atoms:
    def __init__(self, z, pos, cell=None, pbc=None):
        self.numbers, self._pos, self.info = np.asarray(z), np.asarray(pos, dtype=np.float64), {}
        if cell is not None:
            self.cell, self.pbc = cell, pbc

    def get_positions(self):
        return self._pos


@pytest.mark.parametrize("flag", [False, True])
def test_the_facade_forwards_the_flag_everywhere(monkeypatch, flag):
    c = A.UMXCalculator(model="synthetic", stress=True, **({"double_positions": True} if flag else {}))
    c._engine, c._weights = _StubEngine(), None
    monkeypatch.setattr(W, "check_merged_for", lambda *a, **k: None)
    kw = {"double_positions": True} if flag else {}
    z, pos, cell = [8, 1, 1], np.array([[0.0, 0, 0], [0.96, 0, 0], [-0.3, 0.9, 0]]) + T, np.eye(3) * 9.0
    ims = [_Atoms(z, pos + 0.1 * k, cell=cell * (1 + 0.1 * k), pbc=True) for k in range(3)]
    c.calculate(_Atoms(z, pos), ["energy", "forces"])                        # a cluster: no stress
    c.calculate(ims[0], ["energy", "forces", "stress"])
    c.calculate_images([_Atoms(z, pos), _Atoms(z, pos + 0.1)])
    c.calculate_images(ims, per_image_cells=True)
    c.calculate_images(ims, stress=True, per_image_cells=True)
    f64 = np.dtype(np.float64)
    assert c._engine.log == [("ef", f64, kw), ("efs", f64, kw), ("ef", f64, kw), ("ef", f64, kw), ("efs", f64, kw)]


# ---- the local pool against stub engines ---------------------------------------------------------------------------------------------
class _PoolStub:
    def __init__(self, rank):
        self.device, self.natoms, self.rank, self.log = rank, 3, rank, []

    def energy_forces(self, pos, forces=True, **kw):
        p = np.asarray(pos)
        self.log.append(("ef", p.dtype, len(p), kw))
        return np.full(len(p), float(self.rank)), p.astype(np.float32)

    def energy_forces_virial(self, pos, **kw):
        p = np.asarray(pos)
        self.log.append(("efv", p.dtype, len(p), kw))
        return np.full(len(p), float(self.rank)), p.astype(np.float32), np.tile(np.eye(3), (len(p), 1, 1))

    def cell_volume(self):
        return 2.0

    def close(self):
        pass


def test_the_pool_deals_float64_blocks_and_keeps_one_geometry_on_engine_0():
    from pdb2reaction_amd.parallel import LocalEnginePool

    engines = [_PoolStub(r) for r in range(2)]
    pool = LocalEnginePool(engines, gp=True)                                 # graph-parallel on: a single float32 geometry would take it
    try:
        pos = np.random.default_rng(1).normal(size=(5, 3, 3)) + T
        f32, f64, on = np.dtype(np.float32), np.dtype(np.float64), {"double_positions": True}
        e, f = pool.energy_forces(pos)
        e, f = pool.energy_forces(pos, double_positions=True)
        assert pool.last_route == "batch" and pool.last_blocks == [(0, 3), (3, 5)]
        assert engines[0].log == [("ef", f32, 3, {}), ("ef", f64, 3, on)] and engines[1].log == [("ef", f32, 2, {}), ("ef", f64, 2, on)]
        pool.energy_forces_virial(pos, double_positions=True)
        pool.energy_forces_stress(pos, double_positions=True)
        assert engines[1].log[2:] == [("efv", f64, 2, on)] * 2
        pool.energy_forces(pos[0], double_positions=True)                    # one geometry: engine 0 alone, no graph-parallel route
        pool.energy_forces_virial(pos[0], double_positions=True)
        assert pool.last_route == "single" and engines[0].log[4:] == [("ef", f64, 1, on), ("efv", f64, 1, on)] and len(engines[1].log) == 4
        for call in (pool.energy_forces_virial, pool.energy_forces_stress):
            with pytest.raises(ValueError, match="float32 positions only"):
                call(pos[0], graph_parallel=True, double_positions=True)
        assert len(engines[0].log) == 6
    finally:
        pool.close()


# ---- the edge-vector rule, restated in numpy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [14, 70])
def test_float64_difference_rounded_once_is_the_float32_difference_and_is_translation_invariant(n):
    """What GPU tests 1 and 2 rest on.  Coordinates quantised to 2^-20 A with |x| < 16 A are float32 values; a difference is a multiple
    of 2^-20 below 32 A, at most 25 bits: float32 subtraction gives the nearest float32 of the exact difference (exactly it below 16 A),
    which is also what one rounding of the (exact) float64 difference gives.  x + T is exact in float64, so the float64 differences
    at x + T are the same real numbers."""
    z, imgs, _ = synth.make_images(n, 3, seed=21)
    x = np.round(imgs / Q) * Q
    assert np.abs(x).max() < 16.0 and np.array_equal(x.astype(np.float32).astype(np.float64), x)
    x32 = x.astype(np.float32)
    d32 = x32[:, :, None, :] - x32[:, None, :, :]                            # the float entry's rule
    d64 = (x[:, :, None, :] - x[:, None, :, :]).astype(np.float32)           # the double entry's rule
    assert d32.dtype == np.float32 and d32.tobytes() == d64.tobytes()
    inexact = (d32.astype(np.float64) != x[:, :, None, :] - x[:, None, :, :]).mean()
    xt = x + T
    assert np.array_equal(xt - T, x)
    dt = (xt[:, :, None, :] - xt[:, None, :, :]).astype(np.float32)
    assert dt.tobytes() == d64.tobytes()                                     # invariant under T
    xt32 = xt.astype(np.float32)
    old = xt32[:, :, None, :] - xt32[:, None, :, :]
    assert old.tobytes() != d32.tobytes()                                    # the float32 rule at x + T is not
    print(f"[edge-vector rule n={n}] float32 rule at x + T: max |d - d(x)| = {np.abs(old - d32).max():.3e} A; differences that round: {100 * inexact:.1f} %")
