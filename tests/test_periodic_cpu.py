"""CPU tests of periodic boundary conditions: the float64 periodic checker (tests/periodic_oracle.py) against the parent oracle and the
invariants of a periodic system, the calculator facade against a stub engine, and the two new exports of the C ABI.

Tolerances are those of tests/test_oracle.py for the same kind of check: |dE| < 1e-9 eV and max|dF| < 1e-10 eV/A for an invariance,
1e-6 eV/A for forces against central differences (h = 1e-4 A)."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from periodic_oracle import PeriodicOracle, commensurate_atoms, lattice_translations, periodic_radius_graph
from pdb2reaction_amd import synth, weights as W

A = importlib.import_module("pdb2reaction_amd.ase_calculator")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRICLINIC = np.array([[5.0, 0.0, 0.0], [1.1, 6.0, 0.0], [0.7, -0.9, 7.0]])


@pytest.fixture(scope="module")
def small():
    """12 atoms in the small triclinic cell: several images per pair, self-image edges, +-2 translations along a."""
    z, pos = commensurate_atoms(TRICLINIC, (2, 2, 3), seed=5)
    return z, pos


def test_zero_translations_are_the_parent_oracle_bit_for_bit(weights, oracle):
    from oracle.escn_md_oracle import radius_graph

    z, pos = synth.make_cluster(16, seed=3)
    for mn in (None, 5):
        src, dst = radius_graph(torch.as_tensor(pos), W.CUTOFF, mn)
        s2, d2, shift, tidx = periodic_radius_graph(pos, None, None, W.CUTOFF, mn)
        assert torch.equal(src, s2) and torch.equal(dst, d2) and not shift.any() and not tidx.any()
    e, f = oracle.energy_forces(z, pos)
    for orc in (PeriodicOracle(weights), PeriodicOracle(weights, cell=np.eye(3) * 9.0, pbc=False)):
        e2, f2 = orc.energy_forces(z, pos)
        assert e2 == e and np.array_equal(f2, f)


def test_translation_table_reaches_the_cutoff():
    """|n| <= floor(cutoff / h) + 1 per periodic axis, lexicographic order: the 5 A edge takes -2 .. 2, an open axis only 0."""
    ints, h = lattice_translations(TRICLINIC, (True, True, False), 6.0)
    assert sorted(set(ints[:, 0])) == [-2, -1, 0, 1, 2] and {-1, 0, 1} <= set(ints[:, 1]) and set(ints[:, 2]) == {0}
    assert abs(h[0] - 5.0 * 6.0 / np.hypot(1.1, 6.0)) < 1e-12 and abs(h[1] - 6.0) < 1e-12      # plane distances within the a-b plane
    assert [tuple(r) for r in ints] == sorted(tuple(r) for r in ints) and np.isinf(h[2])
    ints, h = lattice_translations(np.eye(3) * 14.0, True, 6.0)
    assert len(ints) == 27 and np.allclose(h, 14.0)


def test_supercell_doubles_the_energy(weights, small):
    z, pos = small
    orc = PeriodicOracle(weights, cell=TRICLINIC, pbc=True)
    e, f = orc.energy_forces(z, pos)
    cell2 = TRICLINIC.copy()
    cell2[0] *= 2
    z2, pos2 = np.concatenate([z, z]), np.concatenate([pos, pos + TRICLINIC[0]])
    e2, f2 = PeriodicOracle(weights, cell=cell2, pbc=True).energy_forces(z2, pos2)
    assert abs(e2 - 2 * e) < 1e-9
    assert np.abs(f2 - np.concatenate([f, f])).max() < 1e-10


def test_rigid_translation_with_atoms_leaving_the_cell(weights, small):
    z, pos = small
    orc = PeriodicOracle(weights, cell=TRICLINIC, pbc=True)
    e, f = orc.energy_forces(z, pos)
    moved = pos + np.random.default_rng(2).uniform(-9.0, 9.0, size=3)
    from periodic_oracle import wrap_offsets

    assert wrap_offsets(moved, TRICLINIC, True).any()                     # atoms did leave the cell, and stay unwrapped
    e2, f2 = orc.energy_forces(z, moved)
    assert abs(e2 - e) < 1e-9
    assert np.abs(f2 - f).max() < 1e-10
    # and a per-atom lattice translation changes nothing either
    hop = moved.copy()
    hop[3] += 2 * TRICLINIC[1] - TRICLINIC[2]
    e3, f3 = orc.energy_forces(z, hop)
    assert abs(e3 - e) < 1e-9 and np.abs(f3 - f).max() < 1e-10


def test_forces_are_minus_gradient(weights, small):
    z, pos = small
    orc = PeriodicOracle(weights, cell=TRICLINIC, pbc=True)
    _, f = orc.energy_forces(z, pos)
    assert np.abs(f.sum(0)).max() < 1e-10
    h = 1e-4
    for a, c in [(0, 0), (5, 1), (11, 2)]:
        pp, pm = pos.copy(), pos.copy()
        pp[a, c] += h
        pm[a, c] -= h
        ep, _ = orc.energy_forces(z, pp, forces=False)
        em, _ = orc.energy_forces(z, pm, forces=False)
        assert abs(-(ep - em) / (2 * h) - f[a, c]) < 1e-6


def test_partial_pbc_uses_no_translation_along_c(weights, small):
    z, pos = small
    src, dst, shift, tidx = periodic_radius_graph(pos, TRICLINIC, (True, True, False), W.CUTOFF)
    coef = shift.numpy() @ np.linalg.inv(TRICLINIC)                       # translations in lattice coordinates
    assert np.abs(coef[:, 2]).max() < 1e-12 and np.abs(coef[:, :2]).max() > 0.5
    full = periodic_radius_graph(pos, TRICLINIC, True, W.CUTOFF)
    assert len(full[0]) > len(src)
    # the slab's energy is that of the fully periodic cell with a c vector too long to matter
    tall = TRICLINIC.copy()
    tall[2] = [0.0, 0.0, 40.0]
    e_slab, f_slab = PeriodicOracle(weights, cell=TRICLINIC, pbc=(True, True, False)).energy_forces(z, pos)
    e_tall, f_tall = PeriodicOracle(weights, cell=tall, pbc=True).energy_forces(z, pos)
    assert abs(e_slab - e_tall) < 1e-9 and np.abs(f_slab - f_tall).max() < 1e-10


def test_max_neigh_keeps_the_nearest_over_all_images(small):
    z, pos = small
    n, m = len(z), 7
    src, dst, shift, tidx = periodic_radius_graph(pos, TRICLINIC, True, W.CUTOFF)
    s2, d2, sh2, t2 = periodic_radius_graph(pos, TRICLINIC, True, W.CUTOFF, m)
    dist = np.linalg.norm(pos[src.numpy()] + shift.numpy() - pos[dst.numpy()], axis=1)
    kept = np.linalg.norm(pos[s2.numpy()] + sh2.numpy() - pos[d2.numpy()], axis=1)
    assert np.bincount(dst.numpy(), minlength=n).min() > m                 # the cap binds for every atom
    images = set()
    for i in range(n):
        all_i, kept_i = np.sort(dist[dst.numpy() == i]), np.sort(kept[d2.numpy() == i])
        assert len(kept_i) == m and np.array_equal(kept_i, all_i[:m])
        images |= set(t2.numpy()[d2.numpy() == i])
    assert len(images) > 1                                                  # the kept ones do come from several images
    # rows are sorted by (target, source, translation index)
    order = np.lexsort((t2.numpy(), s2.numpy(), d2.numpy()))
    assert np.array_equal(order, np.arange(len(order)))


# ---- the calculator facade against a stub engine ---------------------------------------------------------------------------------
class _StubEngine:
    def __init__(self):
        self.cells, self.systems, self.evals = [], 0, 0

    def set_system(self, z, **kw):
        self.systems += 1
        self.natoms = len(z)

    def set_cell(self, cell=None, pbc=None):
        self.cells.append(None if cell is None else (np.array(cell, dtype=np.float64), tuple(bool(p) for p in pbc)))

    def energy_forces(self, pos, forces=True):
        self.evals += 1
        p = np.asarray(pos, dtype=np.float64)
        periodic = bool(self.cells) and self.cells[-1] is not None
        return np.full(len(p), 1.0 if periodic else 0.0) + self.evals, np.zeros_like(p)

    def close(self):
        pass


class _Atoms:
    def __init__(self, z, pos, cell=None, pbc=None, ase_style=False):
        self.numbers, self._pos, self.info = np.asarray(z), np.asarray(pos, dtype=np.float64), {}
        if cell is not None or pbc is not None:
            if ase_style:
                self.get_cell, self.get_pbc = (lambda: np.asarray(cell)), (lambda: np.asarray(pbc))
            else:
                self.cell, self.pbc = cell, pbc

    def get_positions(self):
        return self._pos


@pytest.fixture()
def calc(monkeypatch):
    c = A.UMXCalculator(model="synthetic")
    c._engine, c._weights = _StubEngine(), None
    monkeypatch.setattr(W, "check_merged_for", lambda *a, **k: None)
    return c


@pytest.mark.parametrize("ase_style", [False, True])
def test_cell_and_pbc_reach_set_cell(calc, ase_style):
    z, pos = [8, 1, 1], np.array([[0.0, 0, 0], [0.96, 0, 0], [-0.3, 0.9, 0]])
    calc.calculate(_Atoms(z, pos, cell=TRICLINIC, pbc=[True, True, False], ase_style=ase_style))
    eng = calc._engine
    assert eng.systems == 1 and len(eng.cells) == 1
    assert np.array_equal(eng.cells[0][0], TRICLINIC) and eng.cells[0][1] == (True, True, False)
    calc.calculate(_Atoms(z, pos, cell=TRICLINIC, pbc=[True, True, False], ase_style=ase_style))
    assert len(eng.cells) == 1 and eng.systems == 1 and eng.evals == 1     # unchanged image: bound once, evaluated once


def test_a_changed_cell_rebinds_and_invalidates_the_cache(calc):
    z, pos = [8, 1, 1], np.array([[0.0, 0, 0], [0.96, 0, 0], [-0.3, 0.9, 0]])
    eng = calc._engine
    calc.calculate(_Atoms(z, pos, cell=TRICLINIC, pbc=True))
    e1 = calc.results["energy"]
    calc.calculate(_Atoms(z, pos, cell=TRICLINIC * 1.01, pbc=True))        # same positions, another cell: a new evaluation
    assert eng.evals == 2 and len(eng.cells) == 2 and eng.systems == 1 and calc.results["energy"] != e1
    calc.calculate(_Atoms(z, pos, cell=TRICLINIC * 1.01, pbc=[True, False, True]))
    assert eng.evals == 3 and eng.cells[-1][1] == (True, False, True)
    calc.calculate(_Atoms(z, pos))                                          # back to open boundaries: the cell is cleared
    assert eng.evals == 4 and eng.cells[-1] is None and eng.systems == 1
    calc.calculate(_Atoms(z, pos, cell=TRICLINIC, pbc=False))               # a cell without a periodic axis is open boundaries
    assert eng.evals == 4 and len(eng.cells) == 4


def test_mixed_cells_in_calculate_images_raise(calc):
    z, pos = [8, 1, 1], np.array([[0.0, 0, 0], [0.96, 0, 0], [-0.3, 0.9, 0]])
    ims = [_Atoms(z, pos, cell=TRICLINIC, pbc=True), _Atoms(z, pos + 0.1, cell=TRICLINIC, pbc=True)]
    e, f = calc.calculate_images(ims)
    assert e.shape == (2,) and calc._engine.cells[-1][1] == (True, True, True)
    with pytest.raises(ValueError, match="cell"):
        calc.calculate_images(ims + [_Atoms(z, pos, cell=TRICLINIC * 1.1, pbc=True)])
    with pytest.raises(ValueError, match="cell"):
        calc.calculate_images(ims + [_Atoms(z, pos, cell=TRICLINIC, pbc=[True, True, False])])
    with pytest.raises(ValueError, match="cell"):
        calc.calculate_images(ims + [_Atoms(z, pos)])


def test_atoms_without_a_cell_behave_as_before(calc):
    z, pos = [8, 1, 1], np.array([[0.0, 0, 0], [0.96, 0, 0], [-0.3, 0.9, 0]])
    calc.calculate(_Atoms(z, pos))
    assert calc._engine.cells == [] and calc._engine.systems == 1 and calc.results["energy"] == 1.0
    e, _ = calc.calculate_images([_Atoms(z, pos), _Atoms(z, pos + 0.1)])
    assert calc._engine.cells == [] and e.shape == (2,)
    assert A.UMXCalculator.implemented_properties == ["energy", "forces"]


def test_the_pool_forwards_the_cell_to_every_engine():
    from pdb2reaction_amd.parallel import LocalEnginePool

    engines = [_StubEngine() for _ in range(3)]
    for r, eng in enumerate(engines):
        eng.device = r
    pool = LocalEnginePool(engines, gp=False)
    try:
        pool.set_cell(TRICLINIC, (True, True, False))
        pool.set_cell(None, None)
        for eng in engines:
            assert len(eng.cells) == 2 and np.array_equal(eng.cells[0][0], TRICLINIC) and eng.cells[1] is None
    finally:
        pool.close()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_set_cell_and_the_stats_call_are_exported():
    from pdb2reaction_amd import engine as E

    lib = E.load_library()
    txt = open(os.path.join(ROOT, "include", "umx.h")).read()
    for sym in ("umx_set_cell", "umx_last_graph_shifts"):
        assert sym in txt and sym in E.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert lib.umx_abi_version() == 10                                      # additive: no version bump
    assert lib.umx_last_graph_shifts(None) == 0
    assert lib.umx_set_cell(None, None, None) != 0                          # no engine: refused, not a crash
    assert hasattr(E.Engine, "set_cell") and hasattr(E.Engine, "last_graph_shifts")
    assert lib.umx_set_cell.argtypes[1] == ctypes.POINTER(ctypes.c_double)
