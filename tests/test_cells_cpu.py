"""CPU tests of per-image cells (``umx_set_cells``): the export and its refusal without an engine, the cell family of the GPU tests,
``Engine.energy_forces_stress`` with per-image volumes on an engine object without a device, and the calculator facade and the local
pool against stub engines.  Every test here fails without the feature; the kernels and the host code of the library are covered by
tests/test_gpu_cells.py."""
import ctypes
import importlib
import os

import numpy as np
import pytest

from cells_cases import FAMILIES, assert_image_is_clear, family, table_entries
from stress_oracle import TRICLINIC, voigt_stress
from pdb2reaction_amd import weights as W

A = importlib.import_module("pdb2reaction_amd.ase_calculator")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_set_cells_is_exported_and_refuses_a_null_engine():
    from pdb2reaction_amd import engine as E

    lib = E.load_library()
    txt = open(os.path.join(ROOT, "include", "umx.h")).read()
    assert "umx_set_cells(" in txt and "umx_set_cells" in E.EXPORTED_SYMBOLS and hasattr(lib, "umx_set_cells")
    assert lib.umx_abi_version() == 10                                       # additive: no version bump
    assert lib.umx_set_cells.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
    cells = np.ascontiguousarray(np.stack([TRICLINIC, TRICLINIC * 1.3]))
    flags = np.ones(3, dtype=np.intc)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    assert lib.umx_set_cells(None, 2, cells.ctypes.data_as(dp), flags.ctypes.data_as(ip)) != 0      # no engine: refused, not a crash
    assert lib.umx_set_cells(None, 0, None, None) != 0
    for m in ("set_cells", "cell_volumes"):
        assert hasattr(E.Engine, m)


# ---- the cell family of tests/test_gpu_cells.py ------------------------------------------------------------------------------------------
def test_the_family_has_tables_of_different_sizes_and_clear_images():
    counts = {}
    for name in FAMILIES:
        z, p32, cells, pbc = family(name)
        counts[name] = [table_entries(c, pbc) for c in cells]
        for k in range(len(cells)):
            assert_image_is_clear(p32[k], cells[k], pbc)                     # no image is excused
            assert_image_is_clear(p32[k], cells[k], pbc, 7)
        assert p32.dtype == np.float32 and p32.shape[0] == len(cells)
    # (2 N_a + 1)(2 N_b + 1)(2 N_c + 1) with N_k = floor(6 A / h_k) + 1: the strained cells cross thresholds of N_k
    assert counts == {"triclinic": [5 * 5 * 3, 3 * 3 * 3, 5 * 5 * 5, 5 * 5 * 3, 5 * 5 * 3], "slab": [3 * 3, 5 * 5]}
    z, p_all, c_all, _ = family("triclinic")
    _, p_sel, c_sel, _ = family("triclinic", [0, 2])
    assert np.array_equal(p_sel, p_all[[0, 2]]) and np.array_equal(c_sel, c_all[[0, 2]])
    assert np.array_equal(family("triclinic", 3)[1], p_all[:3])


# ---- Engine, without a device ----------------------------------------------------------------------------------------------------------
def test_engine_stress_divides_every_image_by_its_own_volume():
    from pdb2reaction_amd import engine as E

    eng = object.__new__(E.Engine)
    Wm = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 10.0]])
    w3 = np.stack([Wm, 2 * Wm, -Wm])
    eng.energy_forces_virial = lambda pos: (np.zeros(3), np.zeros((3, 2, 3), np.float32), w3)
    cells = np.stack([TRICLINIC, TRICLINIC * 2.0, -TRICLINIC * 0.5])          # volumes 210, 1680, 26.25 (a left-handed cell: |det|)
    eng._cell, eng._cells = None, (cells, (True, True, True))
    assert np.allclose(eng.cell_volumes(), [210.0, 1680.0, 26.25], rtol=1e-14, atol=0)
    _, _, s = eng.energy_forces_stress(np.zeros((3, 2, 3)))
    assert s.shape == (3, 6)
    for k in range(3):
        assert np.allclose(s[k], voigt_stress(w3[k], cells[k]), rtol=1e-14, atol=0)
    assert np.allclose(s[1], 2 * np.array([1.0, 5.0, 10.0, 7.0, 5.0, 3.0]) / 1680.0, rtol=1e-14, atol=0)
    with pytest.raises(ValueError, match="periodic along all three"):
        eng.cell_volume()                                                    # the one-cell volume stays what it is
    eng._cells = (cells, (True, True, False))
    with pytest.raises(ValueError, match="periodic along all three"):
        eng.energy_forces_stress(np.zeros((3, 2, 3)))
    eng._cell, eng._cells = (TRICLINIC.copy(), (True, True, True)), None      # one shared cell: that volume
    assert np.array_equal(eng.cell_volumes(), np.array([eng.cell_volume()]))


# ---- the calculator facade against a stub engine ---------------------------------------------------------------------------------------
class _StubEngine:
    def __init__(self):
        self.log, self.natoms = [], 0

    def set_system(self, z, **kw):
        self.natoms = len(z)

    def set_cell(self, cell=None, pbc=None):
        self.log.append(("set_cell", None if cell is None else np.array(cell, dtype=np.float64), None if pbc is None else tuple(bool(p) for p in pbc)))

    def set_cells(self, cells=None, pbc=None):
        self.log.append(("set_cells", np.array(cells, dtype=np.float64), tuple(bool(p) for p in pbc)))

    def energy_forces(self, pos, forces=True):
        self.log.append(("ef", len(pos)))
        p = np.asarray(pos, dtype=np.float64)
        return np.arange(len(p), dtype=np.float64), np.ones_like(p)

    def energy_forces_stress(self, pos):
        self.log.append(("efs", len(pos)))
        p = np.asarray(pos, dtype=np.float64)
        return np.arange(len(p), dtype=np.float64), np.ones_like(p), np.tile(np.arange(6.0), (len(p), 1))

    def close(self):
        pass


class _Atoms:
    def __init__(self, z, pos, cell=None, pbc=None):
        self.numbers, self._pos, self.info = np.asarray(z), np.asarray(pos, dtype=np.float64), {}
        if cell is not None:
            self.cell, self.pbc = cell, pbc

    def get_positions(self):
        return self._pos


Z3, POS3 = [8, 1, 1], np.array([[0.0, 0, 0], [0.96, 0, 0], [-0.3, 0.9, 0]])


def _calc(monkeypatch):
    c = A.UMXCalculator(model="synthetic", stress=True)
    c._engine, c._weights = _StubEngine(), None
    monkeypatch.setattr(W, "check_merged_for", lambda *a, **k: None)
    return c


def test_per_image_cells_reach_set_cells_once(monkeypatch):
    c = _calc(monkeypatch)
    cells = [TRICLINIC * s for s in (1.0, 1.3, 0.8)]
    ims = [_Atoms(Z3, POS3 + 0.1 * k, cell=cells[k], pbc=True) for k in range(3)]
    with pytest.raises(ValueError, match="share the cell"):
        c.calculate_images(ims)                                              # the default: one cell per call
    c._engine.log.clear()
    e, f, s = c.calculate_images(ims, stress=True, per_image_cells=True)
    log = c._engine.log
    assert [entry[0] for entry in log] == ["set_cells", "efs"] and log[1][1] == 3
    assert log[0][1].shape == (3, 3, 3) and np.array_equal(log[0][1], np.stack(cells)) and log[0][2] == (True, True, True)
    assert e.shape == (3,) and f.shape == (3, 3, 3) and f.dtype == np.float64 and s.shape == (3, 6)
    e, f = c.calculate_images(ims, per_image_cells=True)                      # the same cells again: they are bound already
    assert [entry[0] for entry in log] == ["set_cells", "efs", "ef"]
    # the single-image cache claims no binding that no longer holds: calculate() binds the image's own cell again
    c.calculate(ims[1], ["energy"])
    assert log[3][0] == "set_cell" and np.array_equal(log[3][1], cells[1]) and [entry[0] for entry in log[4:]] == ["efs"]
    c.calculate_images(ims, per_image_cells=True)                             # ... and the cells come back after it
    assert [entry[0] for entry in log[5:]] == ["set_cells", "ef"]


def test_per_image_cells_want_one_set_of_flags_and_a_cell_everywhere(monkeypatch):
    c = _calc(monkeypatch)
    ims = [_Atoms(Z3, POS3, cell=TRICLINIC, pbc=True), _Atoms(Z3, POS3, cell=TRICLINIC * 1.1, pbc=[True, True, False])]
    with pytest.raises(ValueError, match="pbc flags"):
        c.calculate_images(ims, per_image_cells=True)
    ims = [_Atoms(Z3, POS3, cell=TRICLINIC, pbc=True), _Atoms(Z3, POS3)]
    with pytest.raises(ValueError, match="needs a cell"):
        c.calculate_images(ims, per_image_cells=True)
    assert not any(entry[0] in ("set_cells", "ef", "efs") for entry in c._engine.log)
    slabs = [_Atoms(Z3, POS3, cell=TRICLINIC * s, pbc=[True, True, False]) for s in (1.0, 1.2)]
    with pytest.raises(A.PropertyNotImplementedError):
        c.calculate_images(slabs, stress=True, per_image_cells=True)         # no volume
    assert c.calculate_images(slabs, per_image_cells=True)[0].shape == (2,)


# ---- the local pool against stub engines ---------------------------------------------------------------------------------------------
class _PoolStub:
    def __init__(self, rank):
        self.device, self.natoms, self.rank, self.log = rank, 3, rank, []

    def set_cell(self, cell=None, pbc=None):
        self.log.append(("set_cell", None if cell is None else np.array(cell), pbc))

    def set_cells(self, cells=None, pbc=None):
        self.log.append(("set_cells", np.array(cells), pbc))

    def energy_forces_virial(self, pos):
        p = np.asarray(pos, dtype=np.float32)
        self.log.append(("efv", len(p)))
        return np.full(len(p), float(self.rank)), p, np.tile(np.eye(3), (len(p), 1, 1))

    def cell_volume(self):
        raise AssertionError("per-image cells: the pool's own volumes are used")

    def close(self):
        pass


def test_pool_deals_the_cells_in_the_blocks_of_the_images():
    from pdb2reaction_amd.parallel import LocalEnginePool, shard_bounds

    engines = [_PoolStub(r) for r in range(3)]
    pool = LocalEnginePool(engines, gp=False)
    try:
        cells = np.stack([TRICLINIC * (1.0 + 0.05 * k) for k in range(7)])
        pos = np.zeros((7, 3, 3), dtype=np.float32)
        pool.set_cells(cells, True)
        assert all(eng.log == [] for eng in engines)                          # kept; bound when an engine evaluates
        e, f, s = pool.energy_forces_stress(pos)
        blocks = [shard_bounds(7, 3, r) for r in range(3)]
        assert pool.last_blocks == blocks
        for r, (lo, hi) in enumerate(blocks):
            log = engines[r].log
            assert [entry[0] for entry in log] == ["set_cells", "efv"] and log[1][1] == hi - lo
            assert np.array_equal(log[0][1], cells[lo:hi]) and log[0][2] == (True, True, True)
        vols = np.abs(np.linalg.det(cells))
        assert vols.max() / vols.min() > 2 and np.allclose(s[:, 0], 1.0 / vols, rtol=1e-14, atol=0) and np.array_equal(pool.cell_volumes(), vols)
        pool.energy_forces_virial(pos)                                       # the same blocks: nothing is bound again
        assert all([entry[0] for entry in eng.log] == ["set_cells", "efv", "efv"] for eng in engines)
        with pytest.raises(ValueError, match=r"5 images.*7"):
            pool.energy_forces_virial(pos[:5])
        pool.set_cells(cells[4:5], True)                                     # K = 1: set_cell(cells[0]) on every engine
        pool.energy_forces_virial(pos[0])
        for eng in engines:
            assert eng.log[3][0] == "set_cell" and np.array_equal(eng.log[3][1], cells[4]) and eng.log[3][2] == (True, True, True)
        assert engines[0].log[4:] == [("efv", 1)] and engines[1].log[4:] == []
        pool.set_cell(TRICLINIC, True)                                       # set_cell forwards as before and drops the cells
        assert all(eng.log[-1][0] == "set_cell" for eng in engines)
        pool.energy_forces_virial(pos)
        assert all([entry[0] for entry in eng.log[-2:]] == ["set_cell", "efv"] for eng in engines)
    finally:
        pool.close()
