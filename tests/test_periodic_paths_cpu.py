"""Reaction paths in a periodic cell without a GPU: the minimum-image helper against brute force, the growing-string driver's
unwrapping on a toy periodic evaluator, ``optimize_path_gsm`` and ``prestep`` with a stand-in calculator that carries a cell,
``uma_pysis`` with a stand-in core, and the C ABI's new export.  The engine side is tests/test_gpu_periodic_paths.py."""
import importlib
import os

import numpy as np
import pytest

import periodic_path_cases as PC
from pdb2reaction_amd import engine as E, periodic as P, prestep
from pdb2reaction_amd._calculator_base import ANG2BOHR
from pdb2reaction_amd.gsm import GrowingStringDriver, GSMResult
from pdb2reaction_amd.path_opt import optimize_path_gsm
from toy_core import ToyPairCore, toy_geometry

U = importlib.import_module("pdb2reaction_amd.uma_pysis")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- min_image against brute force --------------------------------------------------------------------------------------------------
def _pairs(cell, seed, n=400):
    return PC.atoms_in_cell(n, cell, seed + 1) - PC.atoms_in_cell(n, cell, seed)


@pytest.mark.parametrize("name", list(PC.CELLS))
def test_min_image_is_the_brute_force_minimum(name):
    cell, pbc = PC.CELLS[name]
    d = _pairs(cell, 3)
    got, want = P.min_image(d, cell, pbc), PC.brute_vectors(d, cell, pbc)
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), np.linalg.norm(want, axis=1), rtol=1e-13, atol=0)
    # an image of d: the difference is a lattice vector of the periodic axes, and open components are untouched
    a, b, _, _ = P.lattice(cell, pbc)
    k = (got - d) @ b.T
    assert np.abs(k - np.rint(k)).max() < 1e-12 and np.abs((got - d) - np.rint(k) @ a).max() < 1e-12
    # odd: the image of -d is minus the image of d, bit for bit (no ties among random pairs)
    assert np.array_equal(P.min_image(-d, cell, pbc), -got)


def test_lattice_ranges_and_refusals():
    assert tuple(P.lattice(*PC.CELLS["skew"])[3]) == (4, 4, 1)
    assert tuple(P.lattice(np.eye(3) * 10.0, True)[3]) == (2, 2, 2)                 # cubic: 5^3 = 125 candidates
    assert tuple(P.lattice(*PC.CELLS["slab"])[3])[2] == 0 and tuple(P.lattice(*PC.CELLS["wire"])[3])[:2] == (0, 0)
    with pytest.raises(ValueError, match="degenerate"):
        P.lattice(np.array([[5.0, 0, 0], [10.0, 0, 0], [0, 0, 8.0]]), True)
    with pytest.raises(ValueError, match="non-finite"):
        P.lattice(np.array([[5.0, 0, 0], [0, np.nan, 0], [0, 0, 8.0]]), True)
    with pytest.raises(ValueError, match="skewed"):
        P.lattice(np.array([[5.0, 0, 0], [9.5, 1.0, 0], [0, 0, 8.0]]), True)
    assert P.pbc_flags(None) is None and P.pbc_flags(False) is None and P.pbc_flags(True) == (True, True, True)


def test_the_skew_cell_needs_the_search():
    """At least one pair in ten has a nearest image that is not the rounded one: without this the search would be untested."""
    cell, pbc = PC.CELLS["skew"]
    d = _pairs(cell, 3)
    a, b, _, _ = P.lattice(cell, pbc)
    rounded = d - np.rint(d @ b.T) @ a
    shorter = np.linalg.norm(PC.brute_vectors(d, cell, pbc), axis=1) < np.linalg.norm(rounded, axis=1) * (1.0 - 1e-12)
    assert shorter.mean() >= 0.1, shorter.mean()


# ---- the driver on a toy periodic evaluator -----------------------------------------------------------------------------------------
CELL_BOHR = PC.SHEARED * 2.0          # multiples of 2^-10 Bohr, like the coordinates below: lattice shifts are exact


def _quantise(x):
    return np.round(np.asarray(x) * 1024.0) / 1024.0


def _toy_eval(x):
    """Springs on minimum-image distances (brute force, independent of the helper): E = sum_{i<j} k/2 (D_ij - r0)^2."""
    x = np.asarray(x, dtype=np.float64)
    es, fs = [], []
    for q in x.reshape(len(x), -1, 3):
        n = len(q)
        e, f = 0.0, np.zeros_like(q)
        for i in range(n):
            v = PC.brute_vectors(q - q[i], CELL_BOHR, (True, True, True))
            d = np.linalg.norm(v, axis=1)
            for j in range(i + 1, n):
                e += 0.5 * 0.05 * (d[j] - 4.0) ** 2
                g = 0.05 * (d[j] - 4.0) * v[j] / d[j]
                f[i] += g
                f[j] -= g
        es.append(e)
        fs.append(f.reshape(-1))
    return np.array(es), np.stack(fs)


def _endpoints():
    rng = np.random.default_rng(12)
    r = _quantise(PC.atoms_in_cell(5, CELL_BOHR, 12))
    p = _quantise(r + rng.uniform(-1.2, 1.2, r.shape))
    shifted = p.copy()
    shifted[1] += CELL_BOHR[0]
    shifted[3] -= CELL_BOHR[1] + 2.0 * CELL_BOHR[2]
    return r, p, shifted


def _driver(r, p, **kw):
    return GrowingStringDriver(["C"] * 5, r.reshape(-1), p.reshape(-1), evaluate=_toy_eval, gs_kw={"max_nodes": 3, "climb": False},
                               stopt_kw={"max_cycles": 4}, **kw)


def test_driver_unwraps_a_wrapped_product_bit_for_bit():
    r, p, shifted = _endpoints()
    assert np.abs(p - r).max() < 0.25 * np.linalg.norm(CELL_BOHR, axis=1).min()            # p is the nearest image already
    runs = [_driver(r, q, cell=CELL_BOHR, pbc=True).run() for q in (p, shifted)]
    assert np.array_equal(runs[0].coords[-1], p.reshape(-1)) and runs[0].cycles == 4
    assert np.array_equal(runs[0].coords, runs[1].coords) and np.array_equal(runs[0].energies, runs[1].energies)
    assert np.array_equal(runs[0].cell, CELL_BOHR) and runs[0].pbc == (True, True, True)
    # unwrap=False keeps the endpoint as given: the initial string differs (two atoms travel through the cell)
    kept = _driver(r, shifted, cell=CELL_BOHR, pbc=True, unwrap=False)
    assert np.array_equal(kept.coords[-1], shifted.reshape(-1))
    assert not np.array_equal(kept.coords, _driver(r, shifted, cell=CELL_BOHR, pbc=True).coords)
    # without a cell nothing is unwrapped and the result carries none
    open_drv = _driver(r, shifted)
    assert np.array_equal(open_drv.coords, kept.coords) and open_drv.cell is None and open_drv.pbc is None
    assert GSMResult.__dataclass_fields__["cell"].default is None and GSMResult.__dataclass_fields__["pbc"].default is None


def test_driver_unwraps_given_images_each_onto_its_predecessor():
    r, p, shifted = _endpoints()
    straight = np.stack([(r + w * (p - r)).reshape(-1) for w in np.linspace(0.0, 1.0, 5)])
    straight = _quantise(straight)
    straight[0], straight[-1] = r.reshape(-1), p.reshape(-1)
    wrapped = straight.copy().reshape(5, -1, 3)
    wrapped[2, 0] += CELL_BOHR[2]
    wrapped[3:, 4] -= CELL_BOHR[0]
    wrapped = wrapped.reshape(5, -1)
    drv = GrowingStringDriver(["C"] * 5, r.reshape(-1), wrapped[-1], evaluate=_toy_eval, gs_kw={"max_nodes": 3}, images=wrapped, cell=CELL_BOHR, pbc=True)
    assert np.array_equal(drv.coords, straight)


def test_from_calculator_takes_the_calculators_cell():
    r, p, shifted = _endpoints()

    class Calc:
        cell, pbc, freeze_atoms = CELL_BOHR / ANG2BOHR, (True, True, True), []

        def get_forces_batch(self, elem, x):
            e, f = _toy_eval(x)
            return {"energy": e, "forces": f}

    kw = dict(gs_kw={"max_nodes": 3}, stopt_kw={"max_cycles": 1})
    drv = GrowingStringDriver.from_calculator(["C"] * 5, r.reshape(-1), shifted.reshape(-1), Calc(), **kw)
    np.testing.assert_allclose(drv.cell, CELL_BOHR, rtol=1e-15)
    np.testing.assert_allclose(drv.coords[-1], p.reshape(-1), rtol=0, atol=1e-12)
    same = GrowingStringDriver.from_calculator(["C"] * 5, r.reshape(-1), shifted.reshape(-1), Calc(), cell=CELL_BOHR * (1 + 1e-12), pbc=True, **kw)
    assert np.array_equal(same.cell, CELL_BOHR * (1 + 1e-12))                               # the explicit cell wins
    for bad in (dict(cell=CELL_BOHR * 1.001, pbc=True), dict(cell=CELL_BOHR, pbc=(True, True, False))):
        with pytest.raises(ValueError, match="calculator"):
            GrowingStringDriver.from_calculator(["C"] * 5, r.reshape(-1), shifted.reshape(-1), Calc(), **bad, **kw)


# ---- optimize_path_gsm and prestep with a stand-in calculator that carries a cell ---------------------------------------------------
class _PeriodicCalc:
    """Batched interface of uma_pysis (Bohr in, Hartree out) on the toy periodic springs, with the calculator's cell attributes (A)."""

    def __init__(self, cell_ang=CELL_BOHR / ANG2BOHR, pbc=(True, True, True)):
        self.cell, self.pbc, self.freeze_atoms = cell_ang, pbc, []

    def get_forces_batch(self, elem, coords):
        e, f = _toy_eval(np.asarray(coords, dtype=float).reshape(len(coords), -1))
        return {"energy": e, "forces": f}

    def get_forces(self, elem, coords):
        e, f = _toy_eval(np.asarray(coords, dtype=float).reshape(1, -1))
        return {"energy": e[0], "forces": f[0]}


def test_optimize_path_gsm_skips_the_alignment_in_a_cell():
    r, p, shifted = _endpoints()
    elem = ["C"] * 5
    res = optimize_path_gsm(elem, r / ANG2BOHR, shifted / ANG2BOHR, calc=_PeriodicCalc(), max_nodes=3, max_cycles=2, fix_ends=True)
    assert res["align"] == [{"skipped": "periodic cell"}] and res["pbc"] == (True, True, True)
    np.testing.assert_allclose(res["cell"], CELL_BOHR / ANG2BOHR, rtol=1e-15)
    np.testing.assert_allclose(res["images_ang"][-1] * ANG2BOHR, p, rtol=0, atol=1e-9)      # unwrapped onto the reactant, not aligned
    # an explicit cell that agrees is accepted; one that does not is refused
    ok = optimize_path_gsm(elem, r / ANG2BOHR, shifted / ANG2BOHR, calc=_PeriodicCalc(), max_nodes=3, max_cycles=1, cell=CELL_BOHR / ANG2BOHR, pbc=True)
    assert ok["align"] == [{"skipped": "periodic cell"}]
    with pytest.raises(ValueError, match="calculator"):
        optimize_path_gsm(elem, r / ANG2BOHR, shifted / ANG2BOHR, calc=_PeriodicCalc(), max_nodes=3, max_cycles=1, cell=CELL_BOHR / ANG2BOHR * 1.01, pbc=True)
    # no cell anywhere: the result says so
    class Open(_PeriodicCalc):
        def __init__(self):
            super().__init__()
            self.cell = self.pbc = None
    res0 = optimize_path_gsm(elem, r / ANG2BOHR, p / ANG2BOHR, calc=Open(), max_nodes=3, max_cycles=1, align=False)
    assert res0["cell"] is None and res0["pbc"] is None and res0["align"] == []


def test_rigid_alignment_refuses_a_periodic_calculator():
    r, p, _ = _endpoints()
    with pytest.raises(ValueError, match="periodic cell"):
        prestep.align_and_refine_sequence(_PeriodicCalc(), ["C"] * 5, [r, p])
    with pytest.raises(ValueError, match="periodic cell"):
        prestep.align_and_refine_pair(_PeriodicCalc(), ["C"] * 5, r, p)


# ---- uma_pysis and a stand-in core --------------------------------------------------------------------------------------------------
def test_uma_pysis_hands_the_cell_to_its_core(monkeypatch):
    made, bound = [], []

    class Core(ToyPairCore):
        def __init__(self, elem, **kw):
            made.append(kw)
            super().__init__(len(elem))

        def set_cell(self, cell=None, pbc=None):
            bound.append((None if cell is None else np.array(cell), pbc))

    monkeypatch.setattr(U, "UMAcore", Core)
    elem, x = ["C", "H", "O"], toy_geometry(3)
    cell = np.array([[9.0, 0, 0], [1.0, 8.0, 0], [0, 0.5, 7.0]])
    U.uma_pysis().get_energy(elem, x * ANG2BOHR)
    assert "cell" not in made[0] and "pbc" not in made[0]                  # the default core sees the reference's keywords only
    calc = U.uma_pysis(cell=cell, pbc=(1, 1, 0))
    assert np.array_equal(calc.cell, cell) and calc.pbc == (True, True, False)
    calc.get_energy(elem, x * ANG2BOHR)
    assert np.array_equal(made[1]["cell"], cell) and made[1]["pbc"] == (True, True, False)
    # set_cell re-binds without rebuilding the core
    calc.set_cell(cell * 1.1, True)
    calc.set_cell(None)
    calc.get_energy(elem, x * ANG2BOHR)
    assert len(made) == 2 and calc.cell is None and calc.pbc is None
    assert np.array_equal(bound[0][0], cell * 1.1) and bound[0][1] == (True, True, True) and bound[1] == (None, None)
    # before the first call it only changes what the core is built with; no flag set is open boundaries
    late = U.uma_pysis()
    late.set_cell(cell, True)
    late.get_energy(elem, x * ANG2BOHR)
    assert np.array_equal(made[2]["cell"], cell)
    assert U.uma_pysis(cell=cell, pbc=False).cell is None
    with pytest.raises(ValueError, match="pbc"):
        U.uma_pysis(cell=cell)


def test_umacore_binds_the_cell_on_engine_or_pool():
    seen = []

    class Binder:
        def __init__(self, tag):
            self.tag = tag

        def set_cell(self, cell, pbc):
            seen.append((self.tag, cell, pbc))

    core = object.__new__(U.UMAcore)
    core._pool, core.engine = None, Binder("engine")
    core.set_cell("c", "p")
    core._pool = Binder("pool")
    core.set_cell(None, None)
    assert seen == [("engine", "c", "p"), ("pool", None, None)]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_new_entry_is_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "umx.h")).read()
    lib = E.load_library()
    assert "umx_bond_changes_cell(" in txt and "umx_bond_changes_cell" in E.EXPORTED_SYMBOLS and hasattr(lib, "umx_bond_changes_cell")
    assert lib.umx_abi_version() == 10                                       # additive: no version bump
