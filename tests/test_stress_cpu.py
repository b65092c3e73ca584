"""CPU tests of the strain derivative W = dE/d eps and the stress: the float64 checker (tests/stress_oracle.py) against central
differences of the energy and the identities a virial obeys; the two new exports of the C ABI; the calculator facade and the local
pool against stub engines.

The tests of the first section ("the checker") validate tests/stress_oracle.py ITSELF -- the yardstick tests/test_gpu_stress.py holds
the engine to -- and touch no code of the package: they pass with or without the feature and are NOT coverage of the engine.  The
engine's kernels, ABI entries and Python methods are covered by tests/test_gpu_stress.py; the sections "the C ABI", "the calculator
facade" and "the local pool" below cover the library's exports and the host-side Python and do fail without the feature.

Bounds: 1e-5 eV against central differences with h = 1e-4 (O(h^2) truncation on |W| of up to ~60 eV; the worst measured is 3.4e-6 eV);
1e-12 eV for identities that hold term by term in float64 (W = -sum r (x) F for a cluster, the symmetry of W for the spectral form);
1e-9 eV for the supercell rule, as tests/test_periodic_cpu.py asks of the energy."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from periodic_oracle import PeriodicOracle
from stress_oracle import CASES, TRICLINIC, make_case, strain_derivative, strained_energy, voigt_stress
from pdb2reaction_amd import synth, weights as W

A = importlib.import_module("pdb2reaction_amd.ase_calculator")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_cache = {}


def virial64(weights, name):
    """(z, pos float64 of the float32-rounded image, cell, pbc, checker, W float64) of a periodic case, evaluated once per session."""
    if name not in _cache:
        z, p32, cell, pbc = make_case(name)
        orc = PeriodicOracle(weights, cell=cell, pbc=pbc)
        pos = p32[0].astype(np.float64)
        _cache[name] = (z, pos, cell, pbc, orc, strain_derivative(orc, z, pos))
    return _cache[name]


# ---- the checker ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_checker_matches_central_differences_of_the_energy(weights, name):
    """dE/d eps_ab by autograd on the fixed graph against (E(+h) - E(-h)) / 2h with positions AND cell strained and the graph built anew
    on every strained geometry: the envelope takes an edge to zero smoothly at the cutoff, so the two agree."""
    z, pos, cell, pbc, orc, Wm = virial64(weights, name)
    h, worst = 1e-4, 0.0
    for a, b in ((0, 0), (1, 2), (2, 0)):
        eps = np.zeros((3, 3))
        eps[a, b] = h
        fd = (strained_energy(orc, z, pos, eps) - strained_energy(orc, z, pos, -eps)) / (2 * h)
        worst = max(worst, abs(fd - Wm[a, b]))
        print(f"[stress cpu {name}] W[{a},{b}] = {Wm[a, b]:+.9f} eV  central difference {fd:+.9f}  |d| = {abs(fd - Wm[a, b]):.2e}")
    assert worst <= 1e-5, (name, worst)


def test_open_cluster_virial_is_minus_sum_r_outer_f(weights):
    z, pos = synth.make_cluster(40, seed=4)
    pos = pos.astype(np.float32).astype(np.float64)
    orc = PeriodicOracle(weights)
    Wm = strain_derivative(orc, z, pos)
    _, f = orc.energy_forces(z, pos)
    assert np.abs(Wm + pos.T @ f).max() <= 1e-12, np.abs(Wm + pos.T @ f).max()


def test_supercell_doubles_the_virial(weights):
    z, pos, cell, pbc, orc, Wm = virial64(weights, "triclinic")
    cell2 = cell.copy()
    cell2[0] *= 2
    z2, pos2 = np.concatenate([z, z]), np.concatenate([pos, pos + cell[0]])
    W2 = strain_derivative(PeriodicOracle(weights, cell=cell2, pbc=pbc), z2, pos2)
    assert np.abs(W2 - 2 * Wm).max() <= 1e-9, np.abs(W2 - 2 * Wm).max()


@pytest.mark.parametrize("name", sorted(CASES))
def test_spectral_virial_is_symmetric(weights, name):
    """The spectral feed-forward is equivariant: the energy does not change under a rotation, the antisymmetric part of W vanishes."""
    Wm = virial64(weights, name)[5]
    assert np.abs(Wm).max() > 1.0                       # (eV: of order -4 ... -64 on these cases)
    assert np.abs(Wm - Wm.T).max() <= 1e-12, np.abs(Wm - Wm.T).max()


@pytest.mark.parametrize("name", ["triclinic", "slab"])
def test_grid_virial_is_not_symmetric(name):
    """The grid feed-forward samples the sphere on a finite grid and is equivariant only approximately: W has an antisymmetric part, far
    above what float32 arithmetic does to W.  This is what lets tests/test_gpu_stress.py see a transposed tensor."""
    w = W.make_synthetic_weights(0, ff_type="grid")
    z, p32, cell, pbc = make_case(name)
    orc = PeriodicOracle(w, cell=cell, pbc=pbc)
    pos = p32[0].astype(np.float64)
    W64 = strain_derivative(orc, z, pos)
    d32 = np.abs(strain_derivative(orc, z, pos, torch.float32) - W64).max()
    asym = np.abs(W64 - W64.T).max()
    print(f"[stress cpu grid {name}] asymmetry {asym:.3e} eV  float32 deviation {d32:.3e} eV")
    assert asym > 10 * d32, (name, asym, d32)


def test_voigt_helpers_agree():
    from pdb2reaction_amd.engine import voigt_stress as engine_voigt

    Wm = np.arange(9, dtype=np.float64).reshape(3, 3) + 1.0
    s = voigt_stress(Wm, TRICLINIC)
    vol = 5.0 * 6.0 * 7.0
    assert np.allclose(s, np.array([1.0, 5.0, 9.0, (6 + 8) / 2, (3 + 7) / 2, (2 + 4) / 2]) / vol, rtol=0, atol=1e-15)
    assert np.allclose(engine_voigt(Wm[None], vol)[0], s, rtol=1e-14, atol=0) and engine_voigt(np.stack([Wm, 2 * Wm]), vol).shape == (2, 6)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_the_virial_entries_are_exported():
    from pdb2reaction_amd import engine as E

    lib = E.load_library()
    txt = open(os.path.join(ROOT, "include", "umx.h")).read()
    for sym in ("umx_energy_forces_virial", "umx_energy_forces_virial_dev"):
        assert sym + "(" in txt and sym in E.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert lib.umx_abi_version() == 10                                      # additive: no version bump
    assert lib.umx_energy_forces_virial(None, 1, None, None, None, None) != 0        # no engine: refused, not a crash
    assert lib.umx_energy_forces_virial_dev(None, 1, None, None, None, None, None) != 0
    assert lib.umx_energy_forces_virial.argtypes[5] == ctypes.POINTER(ctypes.c_double)
    for m in ("energy_forces_virial", "energy_forces_virial_dev", "energy_forces_stress"):
        assert hasattr(E.Engine, m)


def test_engine_stress_divides_the_symmetric_part_by_the_volume():
    """Engine.energy_forces_stress on an engine object without a device: the cell set_cell accepted, Voigt order, ASE's sign."""
    from pdb2reaction_amd import engine as E

    eng = object.__new__(E.Engine)
    Wm = np.array([[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 10.0]]])
    eng.energy_forces_virial = lambda pos: (np.zeros(1), np.zeros((1, 2, 3), np.float32), Wm)
    eng._cell = None
    with pytest.raises(ValueError, match="periodic along all three"):
        eng.energy_forces_stress(np.zeros((1, 2, 3)))
    eng._cell = (TRICLINIC.copy(), (True, True, False))
    with pytest.raises(ValueError, match="periodic along all three"):
        eng.energy_forces_stress(np.zeros((1, 2, 3)))
    eng._cell = (-TRICLINIC, (True, True, True))                             # a left-handed cell: |det|
    _, _, s = eng.energy_forces_stress(np.zeros((1, 2, 3)))
    assert s.shape == (1, 6) and np.allclose(s[0], np.array([1.0, 5.0, 10.0, 7.0, 5.0, 3.0]) / 210.0, rtol=0, atol=1e-15)


# ---- the calculator facade against a stub engine ---------------------------------------------------------------------------------
W_STUB = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 10.0]])


class _StubEngine:
    def __init__(self, with_stress=True):
        self.cells, self.calls, self.natoms = [], [], 0
        if not with_stress:
            self.energy_forces_stress = None                    # touching it would be a TypeError

    def set_system(self, z, **kw):
        self.natoms = len(z)

    def set_cell(self, cell=None, pbc=None):
        self.cells.append(None if cell is None else (np.array(cell, dtype=np.float64), tuple(bool(p) for p in pbc)))

    def energy_forces(self, pos, forces=True):
        self.calls.append("ef")
        p = np.asarray(pos, dtype=np.float64)
        return np.full(len(p), 2.0), np.ones_like(p)

    def energy_forces_stress(self, pos):
        self.calls.append("efs")
        p = np.asarray(pos, dtype=np.float64)
        s = np.stack([voigt_stress(W_STUB * (k + 1), self.cells[-1][0]) for k in range(len(p))])
        return np.full(len(p), 3.0), np.ones_like(p), s

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


def _calc(monkeypatch, stress, with_stress=True):
    c = A.UMXCalculator(model="synthetic", stress=stress)
    c._engine, c._weights = _StubEngine(with_stress), None
    monkeypatch.setattr(W, "check_merged_for", lambda *a, **k: None)
    return c


def test_stress_is_an_instance_property(monkeypatch):
    assert A.UMXCalculator.implemented_properties == ["energy", "forces"]
    on, off = _calc(monkeypatch, True), _calc(monkeypatch, False)
    assert on.implemented_properties == ["energy", "forces", "stress"] and off.implemented_properties == ["energy", "forces"]
    assert A.UMXCalculator.implemented_properties == ["energy", "forces"]


def test_three_getters_are_one_evaluation(monkeypatch):
    c = _calc(monkeypatch, True)
    at = _Atoms(Z3, POS3, cell=TRICLINIC, pbc=True)
    assert c.get_potential_energy(at) == 3.0
    f, s = c.get_forces(at), c.get_stress(at)
    assert c._engine.calls == ["efs"]
    assert f.shape == (3, 3) and f.dtype == np.float64
    # Voigt xx, yy, zz, yz, xz, xy of the symmetric part over the volume 5 x 6 x 7
    assert np.allclose(s, np.array([1.0, 5.0, 10.0, 7.0, 5.0, 3.0]) / 210.0, rtol=0, atol=1e-15)
    moved = _Atoms(Z3, POS3 + 0.01, cell=TRICLINIC, pbc=True)
    c.get_stress(moved)
    assert c._engine.calls == ["efs", "efs"]


def test_an_image_that_is_not_fully_periodic_has_no_stress(monkeypatch):
    c = _calc(monkeypatch, True)
    for at in (_Atoms(Z3, POS3, cell=TRICLINIC, pbc=[True, True, False]), _Atoms(Z3, POS3)):
        assert c.get_potential_energy(at) == 2.0 and c.get_forces(at).shape == (3, 3)
        with pytest.raises(A.PropertyNotImplementedError):
            c.get_stress(at)
    assert set(c._engine.calls) == {"ef"}
    assert issubclass(A.PropertyNotImplementedError, NotImplementedError)


def test_stress_off_never_touches_the_new_engine_method(monkeypatch):
    c = _calc(monkeypatch, False, with_stress=False)
    at = _Atoms(Z3, POS3, cell=TRICLINIC, pbc=True)
    assert c.get_potential_energy(at) == 2.0 and c.get_forces(at).shape == (3, 3)
    e, f = c.calculate_images([at, _Atoms(Z3, POS3 + 0.1, cell=TRICLINIC, pbc=True)])
    assert e.shape == (2,) and c._engine.calls == ["ef", "ef"]
    with pytest.raises(A.PropertyNotImplementedError):
        c.get_stress(at)
    assert c._engine.calls == ["ef", "ef"]


def test_calculate_images_with_stress(monkeypatch):
    c = _calc(monkeypatch, True)
    ims = [_Atoms(Z3, POS3 + 0.1 * k, cell=TRICLINIC, pbc=True) for k in range(3)]
    e, f, s = c.calculate_images(ims, stress=True)
    assert e.shape == (3,) and f.shape == (3, 3, 3) and s.shape == (3, 6) and c._engine.calls == ["efs"]
    assert np.allclose(s[2], 3 * np.array([1.0, 5.0, 10.0, 7.0, 5.0, 3.0]) / 210.0, rtol=0, atol=1e-15)
    assert len(c.calculate_images(ims)) == 2 and c._engine.calls == ["efs", "ef"]
    with pytest.raises(A.PropertyNotImplementedError):
        c.calculate_images([_Atoms(Z3, POS3, cell=TRICLINIC, pbc=[True, False, True])], stress=True)


# ---- the local pool against stub engines ---------------------------------------------------------------------------------------------
class _PoolStub:
    def __init__(self, rank):
        self.device, self.natoms, self.rank, self.seen = rank, 3, rank, []

    def energy_forces_virial(self, pos):
        p = np.asarray(pos, dtype=np.float32)
        self.seen.append(len(p))
        k = len(p)
        return np.full(k, float(self.rank)), p + self.rank, np.full((k, 3, 3), 10.0 * self.rank) + p[:, 0, 0, None, None]

    def cell_volume(self):
        return 210.0

    def close(self):
        pass


@pytest.mark.parametrize("gp", [True, False])
def test_pool_deals_a_batch_in_blocks_and_sends_one_image_to_engine_0(gp):
    from pdb2reaction_amd.parallel import LocalEnginePool, shard_bounds

    engines = [_PoolStub(r) for r in range(3)]
    pool = LocalEnginePool(engines, gp=gp)
    try:
        pos = np.zeros((7, 3, 3), dtype=np.float32)
        pos[:, 0, 0] = np.arange(7)
        e, f, w = pool.energy_forces_virial(pos)
        blocks = [shard_bounds(7, 3, r) for r in range(3)]
        assert pool.last_route == "batch" and pool.last_blocks == blocks and [eng.seen for eng in engines] == [[hi - lo] for lo, hi in blocks]
        for r, (lo, hi) in enumerate(blocks):
            assert (e[lo:hi] == r).all() and np.array_equal(w[lo:hi, 1, 2], 10.0 * r + np.arange(lo, hi))
        assert e.shape == (7,) and f.shape == (7, 3, 3) and w.shape == (7, 3, 3)
        e1, f1, w1 = pool.energy_forces_virial(pos[4])                       # one geometry: engine 0 alone, never graph-parallel
        assert pool.last_route == "single" and engines[0].seen == [blocks[0][1] - blocks[0][0], 1] and engines[1].seen == [blocks[1][1] - blocks[1][0]]
        assert e1.shape == (1,) and w1[0, 0, 0] == 4.0
        e2, f2, s2 = pool.energy_forces_stress(pos)
        assert s2.shape == (7, 6) and np.allclose(s2[5, 0], w[5, 0, 0] / 210.0, rtol=0, atol=1e-15)
    finally:
        pool.close()
