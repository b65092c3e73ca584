"""Periodic boundary conditions on the GPU (``umx_set_cell``), through the C ABI: the engine against the float64 periodic checker
(tests/periodic_oracle.py) on the same synthetic weights, at the project's tolerances |dE| <= 1e-4 eV (UMX_ENERGY_TOL_EV) and
max|dF| <= 1e-3 eV/A (UMX_FORCE_TOL_EV_PER_A); and the equivalences the open-boundary engine is held to, with a cell.

Inputs sit on a jittered lattice commensurate with the cell (all atoms inside it, smallest distances above 1 A).  A condition on
the INPUTS, asserted from the oracle's edges for every case: no edge direction lies in the band around the pole threshold where
float32 and float64 could pick different frame branches.  No element of any comparison is left out.
[3P-UNVERIFIED] like the rest of the model path: fairchem's own periodic graph generation has not been compared."""
import importlib

import numpy as np
import pytest

from periodic_oracle import PeriodicOracle, assert_clear_of_the_pole_band, commensurate_atoms, lattice_translations, periodic_radius_graph
from pdb2reaction_amd import synth, weights as W

pytestmark = pytest.mark.gpu

TOL_E = 1e-4   # eV      (UMX_ENERGY_TOL_EV)
TOL_F = 1e-3   # eV / A  (UMX_FORCE_TOL_EV_PER_A)

CUBIC = np.eye(3) * 14.0
TRICLINIC = np.array([[5.0, 0.0, 0.0], [1.1, 6.0, 0.0], [0.7, -0.9, 7.0]])
SLAB = np.array([[8.6, 0.0, 0.0], [1.3, 8.2, 0.0], [0.0, 0.0, 6.5]])

CASES = {
    # name: (cell, pbc, grid, seed, faces)
    "cubic": (CUBIC, (True, True, True), (5, 5, 5), 11, None),            # 125 atoms, at most one image per pair (14 A > 2 x cutoff)
    "triclinic": (TRICLINIC, (True, True, True), (2, 2, 3), 5, (10, 1)),  # 12 atoms: several images per pair, self images, +-2 along a
    "slab": (SLAB, (True, True, False), (4, 4, 3), 7, None),              # 48 atoms, open along c
}


def make_case(name, k=1):
    """(z, images float32 [k,N,3], cell, pbc): image 0 is the jittered lattice, the others add N(0, 0.02 A) noise."""
    cell, pbc, grid, seed, faces = CASES[name]
    z, pos = commensurate_atoms(cell, grid, seed, faces=faces)
    imgs = [pos] + [pos + 0.02 * np.random.default_rng(seed + 100 + i).standard_normal(pos.shape) for i in range(1, k)]
    return z, np.asarray(imgs, dtype=np.float32), cell, pbc


def reference(orc, z, p32):
    """Oracle energy and forces of one float32 image, with the input condition asserted from the oracle's own edges."""
    p64 = np.asarray(p32, dtype=np.float64)
    src, dst, shift, _ = periodic_radius_graph(p64, orc.cell, orc.pbc, orc.cutoff, orc.max_neigh)
    assert_clear_of_the_pole_band(p64[src.numpy()] + shift.numpy() - p64[dst.numpy()])
    return orc.energy_forces(z, p64)


def check(engine, orc, z, p32, label=""):
    e, f = engine.energy_forces(p32)
    for k in range(len(p32)):
        e_ref, f_ref = reference(orc, z, p32[k])
        de, df = abs(e[k] - e_ref), float(np.abs(f[k] - f_ref).max())
        print(f"[periodic {label} image {k}] |dE| = {de:.3e} eV  max|dF| = {df:.3e} eV/A  shifts {engine.last_graph_shifts()}  (edges, maxdeg) {engine.graph_stats()}")
        assert de <= TOL_E, (label, k, e[k], e_ref)
        assert df <= TOL_F, (label, k, df)
    return e, f


@pytest.fixture()
def eng(weights):
    from pdb2reaction_amd.engine import Engine

    e = Engine(0)
    e.load_weights(weights)
    yield e
    e.close()


@pytest.mark.parametrize("name,shifts", [("cubic", 27), ("triclinic", 5 * 5 * 3), ("slab", 9)])
def test_engine_matches_the_periodic_oracle(eng, weights, name, shifts):
    z, p32, cell, pbc = make_case(name, k=2)
    orc = PeriodicOracle(weights, cell=cell, pbc=pbc)
    eng.set_system(z)
    eng.set_cell(cell, pbc)
    check(eng, orc, z, p32, name)
    assert eng.last_graph_shifts() == shifts
    if name == "triclinic":
        src, dst, _, tidx = periodic_radius_graph(p32[0].astype(np.float64), cell, pbc, W.CUTOFF)
        ints, _ = lattice_translations(cell, pbc, W.CUTOFF)
        assert (src == dst).any() and np.abs(ints[tidx.numpy()][:, 0]).max() == 2   # self-image edges and +-2 translations along a do occur
        pairs = np.stack([src.numpy(), dst.numpy()], 1)
        assert len(np.unique(pairs, axis=0)) < len(pairs)                       # several images per (source, target) pair


def test_positions_outside_the_cell_give_the_same_result(eng, weights):
    """The caller need not wrap: a rigid shift that carries atoms out of the cell, and single atoms moved by lattice vectors."""
    z, p32, cell, pbc = make_case("triclinic")
    orc = PeriodicOracle(weights, cell=cell, pbc=pbc)
    eng.set_system(z)
    eng.set_cell(cell, pbc)
    moved = (p32[0].astype(np.float64) + np.array([3.3, -7.1, 12.9]))
    moved[3] += 2 * cell[1] - cell[2]
    check(eng, orc, z, moved[None].astype(np.float32), "triclinic, unwrapped")


@pytest.mark.parametrize("max_neigh", [7, 20])
def test_max_neigh_keeps_the_nearest_over_all_images(eng, weights, max_neigh):
    """The captured edge list must be the oracle's graph exactly (rows in (source, translation) order), as test_max_neigh_truncation
    asks for open boundaries."""
    z, p32, cell, pbc = make_case("triclinic")
    orc = PeriodicOracle(weights, cell=cell, pbc=pbc, max_neigh=max_neigh)
    eng.set_system(z, max_neigh=max_neigh)
    eng.set_cell(cell, pbc)
    eng.debug_keep(True)
    try:
        eng.energy_forces(p32)
        p64 = p32[0].astype(np.float64)
        src, dst, shift, _ = periodic_radius_graph(p64, cell, pbc, W.CUTOFF, max_neigh)
        assert np.array_equal(eng.debug_fetch("src", np.int32), src.numpy()) and np.array_equal(eng.debug_fetch("dst", np.int32), dst.numpy())
        assert eng.graph_stats() == (max_neigh * len(z), max_neigh)
        evec = eng.debug_fetch("evec").reshape(-1, 4)
        vec = p64[src.numpy()] + shift.numpy() - p64[dst.numpy()]
        d = np.linalg.norm(vec, axis=1)
        # float32 arithmetic on coordinates of up to 10 A: a few ulp of the coordinates
        assert np.abs(evec[:, 3] - d).max() <= 1e-5 and np.abs(evec[:, :3] - vec / d[:, None]).max() <= 1e-5
    finally:
        eng.debug_keep(False)
    check(eng, orc, z, p32, f"triclinic, max_neigh {max_neigh}")


def test_a_large_cell_is_the_open_boundary_engine_bit_for_bit(eng):
    z, imgs, _ = synth.make_images(60, 2, seed=9)
    p32 = (imgs + 25.0).astype(np.float32)                                # inside the cell, 15 A and more from every face
    eng.set_system(z)
    e0, f0 = eng.energy_forces(p32)
    assert eng.last_graph_shifts() == 0
    eng.set_cell(np.eye(3) * 50.0, True)
    e1, f1 = eng.energy_forces(p32)
    assert eng.last_graph_shifts() == 27
    assert np.array_equal(e1, e0) and np.array_equal(f1.view(np.uint32), f0.view(np.uint32))
    eng.set_system(z)                                                       # the cell persists across set_system
    e2, f2 = eng.energy_forces(p32)
    assert eng.last_graph_shifts() == 27 and np.array_equal(e2, e0) and np.array_equal(f2.view(np.uint32), f0.view(np.uint32))
    for clear in ((None, None), (np.eye(3) * 50.0, False)):
        eng.set_cell(np.eye(3) * 50.0, True)
        eng.set_cell(*clear)
        e3, f3 = eng.energy_forces(p32)
        assert eng.last_graph_shifts() == 0 and np.array_equal(e3, e0) and np.array_equal(f3.view(np.uint32), f0.view(np.uint32))


def test_clearing_the_cell_restores_the_cluster(eng, oracle):
    """... also for a system on which the cell matters: with it the periodic result, without it the cluster's."""
    z, p32, cell, pbc = make_case("triclinic")
    eng.set_system(z)
    e_open, f_open = eng.energy_forces(p32)
    eng.set_cell(cell, pbc)
    e_per, _ = eng.energy_forces(p32)
    assert abs(e_per[0] - e_open[0]) > 100 * TOL_E
    eng.set_cell(None)
    e_again, f_again = eng.energy_forces(p32)
    assert np.array_equal(e_again, e_open) and np.array_equal(f_again.view(np.uint32), f_open.view(np.uint32))
    e_ref, f_ref = oracle.energy_forces(z, p32[0].astype(np.float64))
    assert abs(e_open[0] - e_ref) <= TOL_E and np.abs(f_open[0] - f_ref).max() <= TOL_F


@pytest.mark.parametrize("name", ["cubic", "triclinic"])
def test_a_batch_equals_its_singles_bitwise(eng, name):
    z, p32, cell, pbc = make_case(name, k=4)
    eng.set_system(z)
    eng.set_cell(cell, pbc)
    e, f = eng.energy_forces(p32)
    for k in range(len(p32)):
        e1, f1 = eng.energy_forces(p32[k])
        assert e1[0] == e[k] and np.array_equal(f1[0].view(np.uint32), f[k].view(np.uint32)), (name, k)
    e2, _ = eng.energy_forces(p32, forces=False)
    assert np.array_equal(e2, e)


@pytest.mark.parametrize("ff", ["spectral", "grid"])
@pytest.mark.parametrize("mode", ["fp32", "split", "split-bf16", "bf16x3"])
def test_every_precision_mode_and_feed_forward_form(mode, ff):
    from pdb2reaction_amd.engine import Engine

    w = W.make_synthetic_weights(0, **({"ff_type": "grid"} if ff == "grid" else {}))
    eng = Engine(0, precision=mode)
    try:
        eng.load_weights(w)
        for name in ("triclinic", "cubic"):
            z, p32, cell, pbc = make_case(name)
            eng.set_system(z)
            eng.set_cell(cell, pbc)
            check(eng, PeriodicOracle(w, cell=cell, pbc=pbc), z, p32, f"{name}, {mode}, {ff}")
    finally:
        eng.close()


@pytest.mark.parametrize("parts", [0, 2])
def test_partitions_and_recompute_plans(weights, parts, monkeypatch):
    """The stored plan against the recompute plan (mode 2), bitwise, in one piece and in two target-node partitions; the partitioned
    plan against the oracle (its float32 sums over the partitions run in another order than the plan in one piece)."""
    from pdb2reaction_amd.engine import Engine

    if parts:
        monkeypatch.setenv("UMX_FORCE_PARTS", str(parts))
    stored, replay = Engine(0, recompute=0), Engine(0, recompute=2)
    try:
        for e_ in (stored, replay):
            e_.load_weights(weights)
        for name in ("triclinic", "cubic"):
            z, p32, cell, pbc = make_case(name, k=2)
            for e_ in (stored, replay):
                e_.set_system(z)
                e_.set_cell(cell, pbc)
            e0, f0 = check(stored, PeriodicOracle(weights, cell=cell, pbc=pbc), z, p32, f"{name}, {parts} partitions")
            e1, f1 = replay.energy_forces(p32)
            assert stored.last_partitions() == parts and replay.last_partitions() == parts
            assert stored.last_recompute() == 0 and replay.last_recompute() == 1
            assert np.array_equal(e1, e0) and np.array_equal(f1.view(np.uint32), f0.view(np.uint32)), (name, parts)
    finally:
        stored.close()
        replay.close()


def test_a_pool_of_two_engines_on_one_device(weights, monkeypatch):
    """``UMX_LOCAL_DEVICES=0,0`` through the calculator facade: a batch bitwise as one engine, one image graph-parallel over the pool
    within the project tolerances; the facade hands cell and pbc of the images to every engine."""
    A = importlib.import_module("pdb2reaction_amd.ase_calculator")

    class Atoms:
        def __init__(self, z, pos, cell, pbc):
            self.numbers, self._pos, self.cell, self.pbc, self.info = z, np.asarray(pos, dtype=np.float64), cell, pbc, {}

        def get_positions(self):
            return self._pos

    z, p32, cell, pbc = make_case("triclinic", k=4)
    images = [Atoms(z, p, cell, pbc) for p in p32]
    orc = PeriodicOracle(weights, cell=cell, pbc=pbc)
    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    one = A.UMXCalculator(model="synthetic")
    try:
        e1, f1 = one.calculate_images(images)
        one.calculate(images[0])
        s1 = dict(one.results)
        e_ref, f_ref = reference(orc, z, p32[0])
        assert abs(s1["energy"] - e_ref) <= TOL_E and np.abs(s1["forces"] - f_ref).max() <= TOL_F     # the facade is periodic
        assert one._engine.last_graph_shifts() == 75
    finally:
        one.close()
    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,0")
    two = A.UMXCalculator(model="synthetic", workers=2)
    try:
        e2, f2 = two.calculate_images(images)
        pool = two._engine
        assert two.local_devices == [0, 0] and len(pool) == 2 and pool.last_route == "batch"
        assert np.array_equal(e2, e1) and np.array_equal(f2, f1)
        two.calculate(images[0])
        assert pool.last_route == "graph-parallel" and [e.last_graph_shifts() for e in pool.engines] == [75, 75]
        de, df = abs(two.results["energy"] - e_ref), float(np.abs(two.results["forces"] - f_ref).max())
        print(f"[periodic pool, graph-parallel] |dE| = {de:.3e} eV  max|dF| = {df:.3e} eV/A")
        assert de <= TOL_E and df <= TOL_F
        assert abs(two.results["energy"] - s1["energy"]) <= TOL_E and np.abs(two.results["forces"] - s1["forces"]).max() <= TOL_F
    finally:
        two.close()


def test_refusals(eng):
    from pdb2reaction_amd.engine import UmxError

    z, p32, cell, pbc = make_case("triclinic")
    eng.set_system(z)
    eng.set_cell(cell, pbc)
    e0, f0 = eng.energy_forces(p32)
    flat = cell.copy()
    flat[2] = 0.5 * cell[0] - 2.0 * cell[1]
    for bad, flags, what in ((flat, True, "volume"),
                             (np.array([[5.0, 0, 0], [0, 6.0, 0], [10.0, 0, 0]]), (True, False, True), "area"),
                             (np.array([[5.0, 0, 0], [0, 0, 0], [0, 0, 7.0]]), True, "zero length"),
                             (np.diag([1.4, 9.0, 9.0]), True, "lattice translations"),
                             (np.diag([np.nan, 9.0, 9.0]), True, "non-finite"),
                             (np.diag([9.0, 9.0, np.inf]), (True, True, False), "non-finite")):
        with pytest.raises(UmxError, match=what):
            eng.set_cell(bad, flags)
    # a refused call leaves the cell in place
    e1, f1 = eng.energy_forces(p32)
    assert np.array_equal(e1, e0) and np.array_equal(f1, f0)
    # a degenerate c vector is no obstacle when c is open; 1.6 A plane distance is inside the cap
    eng.set_cell(flat, (True, True, False))
    eng.set_cell(np.diag([1.6, 9.0, 9.0]), True)
    # the cap follows the cutoff that is bound
    eng.set_system(z, radius=7.0)
    with pytest.raises(UmxError, match="lattice translations"):
        eng.energy_forces(p32)
    eng.set_system(z)
    eng.set_cell(None)
    assert np.isfinite(eng.energy_forces(p32)[0]).all()
