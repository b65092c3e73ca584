"""Reaction paths in a periodic cell on the GPU: the minimum-image bond-change kernel (``umx_bond_changes_cell``) against brute force,
and the cell carried through ``uma_pysis``, the device-resident growing-string driver and the in-process pool -- each, bit for bit, the
engine with that cell bound (``Engine.set_cell``).  The brute force and the cells are tests/periodic_path_cases.py."""
import ctypes as C
import importlib
import types

import numpy as np
import pytest
import torch

import periodic_path_cases as PC
from periodic_oracle import commensurate_atoms
from stress_oracle import TRICLINIC, make_case
from pdb2reaction_amd import bond_changes as B
from pdb2reaction_amd import hessian as H
from pdb2reaction_amd import synth
from pdb2reaction_amd.engine import Engine, UmxError
from pdb2reaction_amd.gsm import GrowingStringDriver

pytestmark = pytest.mark.gpu

U = importlib.import_module("pdb2reaction_amd.uma_pysis")
MAX_NEIGH = 4                      # binds in every case below (12 atoms within 6 A see dozens of images)
SLAB12 = np.array([[6.2, 0.0, 0.0], [0.9, 5.8, 0.0], [0.0, 0.0, 6.5]])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def light():
    e = Engine(0)                  # no weights, no system: the bond-change entries need neither
    yield e
    e.close()


# ---- 1. bond changes ----------------------------------------------------------------------------------------------------------------
def _pair_of_geometries(n, name):
    """n atoms inside the cell, a second geometry up to 0.4 off the first, element symbols; lengths in Angstrom (unit_scale = 1)."""
    cell, pbc = PC.CELLS[name]
    seed = 100 * n + sorted(PC.CELLS).index(name)
    rng = np.random.default_rng(seed)
    r1 = PC.atoms_in_cell(n, cell, seed)
    r2 = r1 + rng.uniform(-0.4, 0.4, r1.shape)
    atoms = [str(a) for a in rng.choice(["C", "H", "O", "N"], size=n)]
    return cell, pbc, atoms, r1, r2


@pytest.mark.parametrize("name", list(PC.CELLS))
@pytest.mark.parametrize("n", [2, 63, 64, 65, 130])
def test_bond_changes_are_the_brute_force_minimum_image(light, n, name):
    cell, pbc, atoms, r1, r2 = _pair_of_geometries(n, name)
    _, cov = B.element_radii(atoms, 1.0)
    d1, d2 = PC.brute_distances(r1, cell, pbc), PC.brute_distances(r2, cell, pbc)
    code, T = PC.classify(d1, d2, cov)
    assert PC.clear_of_thresholds(d1, d2, T)                                  # the condition on the inputs: no pair at a threshold
    g1, g2 = types.SimpleNamespace(atoms=atoms, coords3d=r1), types.SimpleNamespace(atoms=atoms, coords3d=r2)
    res = B.compare_structures(g1, g2, engine=light, unit_scale=1.0, cell=cell, pbc=pbc)
    print(f"[bond changes {name} n={n}] max|dD1| = {np.abs(res.distances_1 - d1).max():.3e}  max|dD2| = {np.abs(res.distances_2 - d2).max():.3e}  "
          f"formed {len(res.formed_covalent)} broken {len(res.broken_covalent)}")
    np.testing.assert_allclose(res.distances_1, d1, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(res.distances_2, d2, rtol=1e-13, atol=1e-13)
    assert res.formed_covalent == set(map(tuple, np.argwhere(code == 1).tolist()))
    assert res.broken_covalent == set(map(tuple, np.argwhere(code == 2).tolist()))
    for d in (res.distances_1, res.distances_2):
        assert same_bits(d, d.T.copy()) and not d.diagonal().any()


def test_a_bond_across_the_boundary_is_a_bond(light):
    ang = U.ANG2BOHR
    cell = np.eye(3) * 10.0 * ang
    atoms = ["C", "O", "H"]
    r1 = np.array([[0.2, 5, 5], [-1.0, 5, 5], [5, 5, 5]], float) * ang          # C-O 1.2 A apart; the H bonds to nothing
    r2 = np.array([[0.2, 5, 5], [9.0, 5, 5], [5, 5, 5]], float) * ang           # the O wrapped into the cell
    g1, g2 = types.SimpleNamespace(atoms=atoms, coords3d=r1), types.SimpleNamespace(atoms=atoms, coords3d=r2)
    opened = B.compare_structures(g1, g2, engine=light)
    assert opened.broken_covalent == {(0, 1)} and not opened.formed_covalent
    inside = B.compare_structures(g1, g2, engine=light, cell=cell, pbc=True)
    assert not inside.broken_covalent and not inside.formed_covalent
    np.testing.assert_allclose([inside.distances_1[0, 1], inside.distances_2[0, 1]], [1.2 * ang] * 2, rtol=1e-13)
    assert B.summarize_changes(g2, inside) == "Bond formed: None\nBond broken: None"


def _raw(eng, r1, r2, cov, cell, pbc, fill=7.0):
    """``umx_bond_changes_cell`` straight through ctypes on pre-filled outputs: (status, d1, d2, code)."""
    n = len(cov)
    dp = C.POINTER(C.c_double)
    d1, d2, code = np.full((n, n), fill), np.full((n, n), fill), np.full((n, n), 9, np.uint8)
    lat = None if cell is None else np.ascontiguousarray(cell, dtype=np.float64)
    flg = None if pbc is None else np.ascontiguousarray(pbc, dtype=np.intc)
    st = eng.lib.umx_bond_changes_cell(eng._h, n, np.ascontiguousarray(r1).ctypes.data_as(dp), np.ascontiguousarray(r2).ctypes.data_as(dp),
                                       np.ascontiguousarray(cov).ctypes.data_as(dp), None if lat is None else lat.ctypes.data_as(dp),
                                       None if flg is None else flg.ctypes.data_as(C.POINTER(C.c_int)), 1.2, 0.05, 0.05, d1.ctypes.data_as(dp),
                                       d2.ctypes.data_as(dp), code.ctypes.data_as(C.POINTER(C.c_uint8)))
    return st, d1, d2, code


def test_no_cell_is_the_open_entry_bit_for_bit(light):
    cell, pbc, atoms, r1, r2 = _pair_of_geometries(65, "sheared")
    _, cov = B.element_radii(atoms, 1.0)
    want = light.bond_changes(r1, r2, cov)
    for c_, p_ in ((None, pbc), (cell, None), (cell, (0, 0, 0))):
        st, d1, d2, code = _raw(light, r1, r2, cov, c_, p_)
        assert st == 0 and same_bits(d1, want[0]) and same_bits(d2, want[1]) and same_bits(code, want[2])
    for kw in ({}, {"cell": None, "pbc": True}, {"cell": cell}, {"cell": cell, "pbc": False}):
        got = light.bond_changes(r1, r2, cov, **kw)
        assert all(same_bits(a, b) for a, b in zip(got, want))
    periodic = light.bond_changes(r1, r2, cov, cell=cell, pbc=pbc)
    assert not same_bits(periodic[0], want[0])


def test_refused_cells_leave_the_outputs_untouched(light):
    cell, pbc, atoms, r1, r2 = _pair_of_geometries(5, "ortho")
    _, cov = B.element_radii(atoms, 1.0)
    nan = cell.copy()
    nan[1, 2] = np.nan
    cases = [(np.array([[5.0, 0, 0], [10.0, 0, 0], [0, 0, 8.0]]), (1, 1, 1), "degenerate cell: the periodic lattice vectors span no volume"),
             (np.array([[5.0, 0, 0], [10.0, 0, 0], [0, 0, 8.0]]), (1, 1, 0), "degenerate cell: the two periodic lattice vectors span no area"),
             (np.array([[0.0, 0, 0], [0, 6.0, 0], [0, 0, 8.0]]), (1, 0, 0), "degenerate cell: lattice vector a has zero length"),
             (nan, (1, 1, 1), "non-finite cell entry"),
             (np.array([[5.0, 0, 0], [9.5, 1.0, 0], [0, 0, 8.0]]), (1, 1, 1), "more than the 4 lattice translations")]   # h_b = 1: M_b = 11
    for bad, flags, why in cases:
        st, d1, d2, code = _raw(light, r1, r2, cov, bad, flags)
        assert st == -1 and why in light.lib.umx_last_error(light._h).decode(), (why, light.lib.umx_last_error(light._h))
        assert (d1 == 7.0).all() and (d2 == 7.0).all() and (code == 9).all()
        with pytest.raises(UmxError, match="umx_bond_changes_cell"):
            light.bond_changes(r1, r2, cov, cell=bad, pbc=flags)
    # the same degenerate row on an OPEN axis is no obstacle, and the skew cell sits exactly at the cap (M = 4, 4, 1)
    assert _raw(light, r1, r2, cov, np.array([[5.0, 0, 0], [10.0, 0, 0], [0, 0, 8.0]]), (1, 0, 1))[0] == 0
    assert _raw(light, r1, r2, cov, *PC.CELLS["skew"])[0] == 0


# ---- 2. the calculator ----------------------------------------------------------------------------------------------------------------
def elements(z):
    return [synth.SYMBOLS[int(a)] for a in z]


def _case(name):
    """(z, x (N,3) A float64, cell, pbc): the 12-atom triclinic case of the stress tests (self images), or a 12-atom slab open along c."""
    if name == "triclinic":
        z, imgs, cell, pbc = make_case("triclinic")
        return z, imgs[0].astype(np.float64), cell, pbc
    z, pos = commensurate_atoms(SLAB12, (2, 2, 3), 7)
    return z, pos.astype(np.float32).astype(np.float64), SLAB12, (True, True, False)


@pytest.fixture()
def eng(weights):
    e = Engine(0)
    e.load_weights(weights)
    yield e
    e.close()


def _in_units(e, f):
    """``uma_pysis``' own conversion of the engine's (eV, float32 eV/A) to (Hartree, float64 Hartree/Bohr)."""
    return np.asarray(e, dtype=np.float64) * U.EV2AU, np.asarray(f, dtype=np.float64) * U.F_EVAA_2_AU


@pytest.mark.parametrize("name", ["triclinic", "slab"])
def test_the_calculator_is_the_engine_with_the_cell_bound(eng, monkeypatch, name):
    z, x, cell, pbc = _case(name)
    elem = elements(z)
    rng = np.random.default_rng(4)
    xs = np.stack([x] + [x + 0.05 * rng.standard_normal(x.shape) for _ in range(3)])
    bohr = xs * U.ANG2BOHR
    eng.set_system(z, max_neigh=MAX_NEIGH)
    e_open, f_open = _in_units(*eng.energy_forces(bohr * U.BOHR2ANG))
    eng.set_cell(cell, pbc)
    e_cell, f_cell = _in_units(*eng.energy_forces(bohr * U.BOHR2ANG))
    assert eng.last_graph_shifts() > 1 and eng.graph_stats()[1] == MAX_NEIGH and not same_bits(e_cell, e_open)
    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    calc = U.uma_pysis(model="synthetic", max_neigh=MAX_NEIGH, cell=cell, pbc=pbc)
    try:
        one = calc.get_forces(elem, bohr[1].reshape(-1))
        assert same_bits(np.float64(one["energy"]), e_cell[1]) and same_bits(one["forces"], f_cell[1].reshape(-1))
        assert same_bits(np.float64(calc.get_energy(elem, bohr[2])["energy"]), e_cell[2])
        many = calc.get_forces_batch(elem, bohr.reshape(4, -1))
        assert same_bits(many["energy"], e_cell) and same_bits(many["forces"], f_cell.reshape(4, -1))
        assert same_bits(calc.get_energy_batch(elem, bohr)["energy"], e_cell)
        core = calc._core
        f_dev = core.compute_batch_dev(torch.as_tensor((bohr * U.BOHR2ANG).astype(np.float32), device=core.device))
        assert same_bits(np.asarray(f_dev.cpu().numpy(), dtype=np.float64) * U.F_EVAA_2_AU, f_cell)
        calc.set_cell(None)                                                   # open again, the same core
        assert calc._core is core
        many = calc.get_forces_batch(elem, bohr.reshape(4, -1))
        assert same_bits(many["energy"], e_open) and same_bits(many["forces"], f_open.reshape(4, -1))
        calc.set_cell(cell, pbc)
        assert same_bits(calc.get_forces_batch(elem, bohr.reshape(4, -1))["energy"], e_cell)
    finally:
        calc.close()


@pytest.mark.parametrize("double", [False, True], ids=["float", "double"])
@pytest.mark.parametrize("pin", [False, True], ids=["free", "pinned"])
def test_the_hessian_is_fd_hessian_over_the_engine_in_the_cell(eng, monkeypatch, pin, double):
    cell, pbc = TRICLINIC, (True, True, True)
    z, pos = commensurate_atoms(cell, (1, 2, 3), 5)                           # 6 atoms: every pair through several images
    x = pos.astype(np.float32).astype(np.float64) + (1e-6 * np.random.default_rng(1).standard_normal(pos.shape) if double else 0.0)
    bohr = (x * U.ANG2BOHR).reshape(-1)
    x = bohr.reshape(-1, 3) * U.BOHR2ANG                                      # the geometry the calculator sees: through Bohr and back
    dp = {"double_positions": True} if double else {}
    eng.set_system(z, max_neigh=MAX_NEIGH)
    eng.set_cell(cell, pbc)
    ref = object.__new__(U.UMAcore)                                           # UMAcore's own batch calls, over THIS engine
    ref.engine, ref._pool, ref._gp, ref.double_positions, ref.z = eng, None, None, double, z
    if pin:
        eng.pin_graph(x, **dp)
    want = H.fd_hessian(lambda c: ref.compute_batch(c, forces=True)["forces"], x, [], device=ref.device, double=True, partial=False, batch=U.FD_BATCH,
                        engine=eng, batch_forces_dev=ref.compute_batch_dev, **dp)
    if pin:
        eng.unpin_graph()
    want = H.hessian_to_au(want, double=True, as_torch=False)
    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    calc = U.uma_pysis(model="synthetic", max_neigh=MAX_NEIGH, cell=cell, pbc=pbc, hessian_pin_graph=pin, out_hess_torch=False, **dp)
    try:
        got = calc.get_hessian(elements(z), bohr)["hessian"]
    finally:
        calc.close()
    assert got.shape == (18, 18) and np.abs(got).max() > 0
    assert same_bits(np.asarray(got), np.asarray(want))
    # ... and not the open Hessian
    eng.set_cell(None)
    other = H.fd_hessian(lambda c: ref.compute_batch(c, forces=True)["forces"], x, [], device=ref.device, double=True, partial=False, batch=U.FD_BATCH,
                         engine=eng, batch_forces_dev=ref.compute_batch_dev, **dp)
    assert not same_bits(np.asarray(H.hessian_to_au(other, double=True, as_torch=False)), np.asarray(want))


# ---- 3. the device-resident driver ------------------------------------------------------------------------------------------------------
def test_the_device_resident_driver_unwraps_and_evaluates_in_the_cell(eng, monkeypatch):
    z, x, _, pbc = _case("triclinic")
    elem = elements(z)
    cell_bohr = np.round(TRICLINIC * U.ANG2BOHR * 1024.0) / 1024.0            # cell and coordinates on a 2^-10 Bohr grid: lattice shifts are exact
    cell_ang = cell_bohr * U.BOHR2ANG
    rng = np.random.default_rng(8)
    r = np.round(x * U.ANG2BOHR * 1024.0) / 1024.0
    p = np.round((r + rng.uniform(-0.5, 0.5, r.shape)) * 1024.0) / 1024.0
    wrapped = p.copy()
    wrapped[2] += cell_bohr[0] - cell_bohr[2]
    wrapped[7] -= 2.0 * cell_bohr[1]
    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    calc = U.uma_pysis(model="synthetic", max_neigh=MAX_NEIGH, cell=cell_ang, pbc=pbc)
    try:
        kw = dict(gs_kw={"max_nodes": 3}, stopt_kw={"max_cycles": 2}, cell=cell_bohr, pbc=pbc)
        runs = []
        for q in (p, wrapped):
            drv = GrowingStringDriver.from_calculator(elem, r.reshape(-1), q.reshape(-1), calc, **kw)
            assert drv.device.type == "cuda"
            runs.append(drv.run())
        assert same_bits(runs[0].coords[-1], p.reshape(-1))
        assert same_bits(runs[0].coords, runs[1].coords) and same_bits(runs[0].energies, runs[1].energies)
        assert same_bits(runs[0].cell, cell_bohr) and runs[0].pbc == (True, True, True)
        with pytest.raises(ValueError, match="calculator"):
            GrowingStringDriver.from_calculator(elem, r.reshape(-1), p.reshape(-1), calc, **{**kw, "cell": cell_bohr * 1.001})
    finally:
        calc.close()
    # the driver's energies are the engine's, in that cell, at the driver's coordinates
    eng.set_system(z, max_neigh=MAX_NEIGH)
    eng.set_cell(cell_ang, pbc)
    k = len(runs[0].coords)
    e_ref, _ = _in_units(*eng.energy_forces(runs[0].coords.reshape(k, -1, 3) * U.BOHR2ANG))
    assert same_bits(runs[0].energies, e_ref)
    eng.set_cell(None)
    assert not same_bits(runs[0].energies, _in_units(*eng.energy_forces(runs[0].coords.reshape(k, -1, 3) * U.BOHR2ANG))[0])


# ---- 4. the in-process pool ---------------------------------------------------------------------------------------------------------------
def test_a_pool_of_two_engines_binds_the_cell_on_both(eng, monkeypatch):
    z, x, cell, pbc = _case("triclinic")
    rng = np.random.default_rng(6)
    bohr = np.stack([x + 0.05 * rng.standard_normal(x.shape) for _ in range(4)]) * U.ANG2BOHR
    eng.set_system(z, max_neigh=MAX_NEIGH)
    eng.set_cell(cell, pbc)
    e_cell, f_cell = _in_units(*eng.energy_forces(bohr * U.BOHR2ANG))
    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,0")
    calc = U.uma_pysis(model="synthetic", max_neigh=MAX_NEIGH, workers=2, cell=cell, pbc=pbc)
    try:
        many = calc.get_forces_batch(elements(z), bohr.reshape(4, -1))
        pool = calc._core._pool
        assert len(pool) == 2 and pool.last_route == "batch" and all(e.last_graph_shifts() > 1 for e in pool.engines)
        assert same_bits(many["energy"], e_cell) and same_bits(many["forces"], f_cell.reshape(4, -1))
    finally:
        calc.close()
