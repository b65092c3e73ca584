"""Per-image cells on the GPU (``umx_set_cells``): one batch of images, each in its own periodic cell, through the C ABI and the Python
layers above it.

The yardstick is exact: image k of a per-image-cell batch is, in every bit of E (float64), F (float32) and W (float64), the single
evaluation of image k after ``set_cell(cell_k)`` -- in one piece, in chunks, on two lanes, in partitions and with the recompute plan,
with ``max_neigh`` binding, and over a pool of two engines.  On top of that every image of the family meets the project's tolerances
against the float64 periodic checker (|dE| <= 1e-4 eV, max|dF| <= 1e-3 eV/A, include/umx.h) and the virial rule of
tests/test_gpu_stress.py (max|dW| <= M_D32[mode] d32, the same constants, restated here), and the stress of image k refers to the
volume of cell k (the volumes differ by a factor of 4 across the family).

The cells (tests/cells_cases.py) have translation tables of 75, 27, 125, 75 (and 75) entries, the slab's 9 and 25; the counts are
computed with ``periodic_oracle.lattice_translations``.  Every image held to the checker satisfies ``assert_clear_of_the_pole_band``.
[3P-UNVERIFIED] like the rest of the periodic path: fairchem's own periodic graph generation and stress have not been compared."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from cells_cases import FAMILIES, assert_image_is_clear, family, table_entries
from periodic_oracle import PeriodicOracle
from stress_oracle import TRICLINIC, strain_derivative, voigt_stress
from test_gpu_periodic import TOL_E, TOL_F
from pdb2reaction_amd import synth

pytestmark = pytest.mark.gpu

# the rule of tests/test_gpu_stress.py: max|dW| <= m d32, d32 the checker's own float32 deviation on the case, m per precision mode
M_D32 = {"fp32": 1, "bf16x3": 2, "split-bf16": 16, "split": 16}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_efw(a, b):
    return a[0].dtype == np.float64 and a[1].dtype == np.float32 and a[2].dtype == np.float64 and all(same_bits(x, y) for x, y in zip(a, b))


def new_engine(weights, **kw):
    from pdb2reaction_amd.engine import Engine

    e = Engine(0, **kw)
    e.load_weights(weights)
    return e


@pytest.fixture()
def eng(weights):
    e = new_engine(weights)
    yield e
    e.close()


def singles(eng, p32, cells, pbc):
    """(E [K], F [K,N,3], W [K,3,3]) of the images one by one, each after ``set_cell`` with its own cell."""
    out = []
    for k in range(len(p32)):
        eng.set_cell(cells[k], pbc)
        out.append(eng.energy_forces_virial(p32[k]))
    return tuple(np.concatenate([o[i] for o in out]) for i in range(3))


# ---- 1. a batch equals its singles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("triclinic", 4), ("slab", 2)])
def test_a_batch_equals_its_singles_bitwise(eng, name, k):
    z, p32, cells, pbc = family(name, k)
    counts = [table_entries(c, pbc) for c in cells]
    assert len(set(counts)) > 1                                              # the tables do differ in size
    eng.set_system(z)
    eng.set_cells(cells, pbc)
    batch = eng.energy_forces_virial(p32)
    assert eng.last_graph_shifts() == max(counts)
    one = singles(eng, p32, cells, pbc)
    for i in range(k):
        assert same_efw([x[i] for x in batch], [x[i] for x in one]), (name, i)
    assert len({batch[0][i] for i in range(k)}) == k                         # the images differ: a wrong cell cannot pass
    eng.set_cells(cells, pbc)                                                # and again after the single cells
    assert same_efw(eng.energy_forces_virial(p32), batch)


# ---- 2. and 3. every image against the float64 checker --------------------------------------------------------------------------------
_batch, _ref = {}, {}
CELLS = [(name, i) for name in sorted(FAMILIES) for i in range(len(FAMILIES[name][2]) - (name == "triclinic"))]     # the six of the table


def batch_of(weights, name):
    """E, F, W and the stress (where there is a volume) of the whole family in one per-image-cell call, once per session."""
    if name not in _batch:
        z, p32, cells, pbc = family(name)
        e = new_engine(weights)
        try:
            e.set_system(z)
            e.set_cells(cells, pbc)
            _batch[name] = e.energy_forces_virial(p32) + (e.energy_forces_stress(p32)[2] if all(pbc) else None, e.precision_mode())
        finally:
            e.close()
    return _batch[name]


def checker(weights, name, i):
    """(orc, z, p64, graph) of image i of a family, the input condition asserted."""
    if (name, i) not in _ref:
        z, p32, cells, pbc = family(name)
        torch.set_num_threads(16)
        _ref[(name, i)] = (PeriodicOracle(weights, cell=cells[i], pbc=pbc), z, p32[i].astype(np.float64), assert_image_is_clear(p32[i], cells[i], pbc))
    return _ref[(name, i)]


@pytest.mark.parametrize("name,i", CELLS)
def test_every_image_matches_the_periodic_oracle(weights, name, i):
    e, f = batch_of(weights, name)[:2]
    orc, z, p64, _ = checker(weights, name, i)
    e_ref, f_ref = orc.energy_forces(z, p64)
    de, df = abs(e[i] - e_ref), float(np.abs(f[i] - f_ref).max())
    print(f"[cells oracle {name} image {i}] |dE| = {de:.3e} eV  max|dF| = {df:.3e} eV/A")
    assert de <= TOL_E, (name, i, e[i], e_ref)
    assert df <= TOL_F, (name, i, df)


@pytest.mark.parametrize("name,i", CELLS)
def test_every_virial_matches_the_strain_derivative(weights, name, i):
    _, _, w, stress, mode = batch_of(weights, name)
    orc, z, p64, graph = checker(weights, name, i)
    w64 = strain_derivative(orc, z, p64, graph=graph)
    d32 = float(np.abs(strain_derivative(orc, z, p64, torch.float32, graph=graph) - w64).max())
    dw = float(np.abs(w[i] - w64).max())
    print(f"[cells virial {name} image {i} {mode}] max|dW| = {dw:.3e} eV  d32 = {d32:.3e} eV  ratio = {dw / d32:.2f}  (m = {M_D32[mode]})")
    assert dw <= M_D32[mode] * d32, (name, i, dw, d32)
    if stress is not None:
        cells = family(name)[2]
        want = voigt_stress(w[i], cells[i])
        assert np.abs(stress[i] - want).max() <= 1e-12 * np.abs(want).max(), (name, i)


def test_the_volumes_differ_across_the_family(eng):
    z, p32, cells, pbc = family("triclinic", 4)
    eng.set_cells(cells, pbc)
    vols = eng.cell_volumes()
    assert vols.shape == (4,) and vols.dtype == np.float64 and vols.max() / vols.min() > 4.0
    assert np.allclose(vols, [abs(np.linalg.det(c)) for c in cells], rtol=1e-15, atol=0)
    eng.set_cell(cells[1], pbc)
    assert same_bits(eng.cell_volumes(), np.array([eng.cell_volume()]))
    eng.set_cells(cells, (True, True, False))
    with pytest.raises(ValueError, match="periodic along all three"):
        eng.cell_volumes()


# ---- 4. chunks and lanes, 5. partitions and recompute ----------------------------------------------------------------------------------
def test_chunks_and_lanes_read_the_cell_of_their_image(weights, monkeypatch):
    z, p32, cells, pbc = family("triclinic", 5)

    def run(env, lanes):
        for k_, v in env.items():
            monkeypatch.setenv(k_, v)
        e_ = new_engine(weights)
        try:
            e_.set_system(z)
            e_.set_cells(cells, pbc)
            out = e_.energy_forces_virial(p32)
            assert e_.last_lanes() == lanes and e_.last_partitions() == 0 and e_.last_graph_shifts() == 125
            return out
        finally:
            e_.close()
            for k_ in env:
                monkeypatch.delenv(k_)

    whole = run({}, 1)
    for env, lanes in (({"UMX_MAX_CHUNK_IMAGES": "1"}, 1), ({"UMX_MAX_CHUNK_IMAGES": "3"}, 1), ({"UMX_STREAMS": "2"}, 2)):
        assert same_efw(run(env, lanes), whole), env


@pytest.mark.parametrize("setting", ["parts2", "parts3", "recompute2"])
def test_partitions_and_recompute_read_the_cell_of_their_image(weights, monkeypatch, setting):
    z, p32, cells, pbc = family("triclinic", 3)
    if setting.startswith("parts"):
        monkeypatch.setenv("UMX_FORCE_PARTS", setting[-1])
    e_ = new_engine(weights, **({"recompute": 2} if setting == "recompute2" else {}))
    try:
        e_.set_system(z)
        e_.set_cells(cells, pbc)
        batch = e_.energy_forces_virial(p32)
        assert e_.last_partitions() == (int(setting[-1]) if setting.startswith("parts") else 0)
        assert e_.last_recompute() == (1 if setting == "recompute2" else 0)
        one = singles(e_, p32, cells, pbc)
        for i in range(3):
            assert same_efw([x[i] for x in batch], [x[i] for x in one]), (setting, i)
    finally:
        e_.close()


# ---- 6. max_neigh binds ------------------------------------------------------------------------------------------------------------------
def test_max_neigh_7_with_two_cells(eng, weights):
    z, p32, cells, pbc = family("triclinic", [0, 2])                         # 75 and 125 translations
    n = len(z)
    eng.set_system(z, max_neigh=7)
    eng.set_cells(cells, pbc)
    batch = eng.energy_forces_virial(p32)
    assert eng.graph_stats() == (2 * 7 * n, 7)
    one = singles(eng, p32, cells, pbc)
    for i in range(2):
        assert same_efw([x[i] for x in batch], [x[i] for x in one]), i
        orc = PeriodicOracle(weights, cell=cells[i], pbc=pbc, max_neigh=7)
        assert_image_is_clear(p32[i], cells[i], pbc, 7)
        e_ref, f_ref = orc.energy_forces(z, p32[i].astype(np.float64))
        de, df = abs(batch[0][i] - e_ref), float(np.abs(batch[1][i] - f_ref).max())
        print(f"[cells max_neigh 7 image {i}] |dE| = {de:.3e} eV  max|dF| = {df:.3e} eV/A")
        assert de <= TOL_E and df <= TOL_F, (i, de, df)


# ---- 7. equivalences -------------------------------------------------------------------------------------------------------------------
def test_identical_cells_are_set_cell(eng):
    z, p32, cells, pbc = family("triclinic", 4)
    eng.set_system(z)
    eng.set_cell(cells[2], pbc)
    shared = eng.energy_forces_virial(p32)
    one = eng.energy_forces_virial(p32[1])
    eng.set_cells(np.stack([cells[2]] * 4), pbc)
    assert same_efw(eng.energy_forces_virial(p32), shared) and eng.last_graph_shifts() == 125
    eng.set_cells(cells[2:3], pbc)                                           # K = 1
    assert same_efw(eng.energy_forces_virial(p32[1]), one)
    eng.set_cells(cells, pbc)
    per_image = eng.energy_forces_virial(p32)
    assert not same_bits(per_image[0], shared[0])
    eng.set_cell(cells[2], pbc)                                              # set_cell after set_cells replaces it
    assert same_efw(eng.energy_forces_virial(p32), shared)
    assert same_efw(eng.energy_forces_virial(p32[:2]), [x[:2] for x in shared])     # ... for any number of images again
    eng.set_system(z)                                                        # the cells persist across set_system
    eng.set_cells(cells, pbc)
    eng.set_system(z)
    assert same_efw(eng.energy_forces_virial(p32), per_image)


def test_no_flag_or_no_cells_is_the_cluster(eng):
    z, p32, cells, pbc = family("triclinic", 4)
    eng.set_system(z)
    cluster = eng.energy_forces_virial(p32)
    for clear in ((cells, False), (None, None)):
        eng.set_cells(cells, pbc)
        assert not same_bits(eng.energy_forces_virial(p32)[0], cluster[0])
        eng.set_cells(*clear)
        assert same_efw(eng.energy_forces_virial(p32), cluster) and eng.last_graph_shifts() == 0
        assert same_efw(eng.energy_forces_virial(p32[:3]), [x[:3] for x in cluster])      # no count is bound any more


def test_large_cells_are_the_open_boundary_engine_bit_for_bit(eng):
    z, imgs, _ = synth.make_images(60, 2, seed=9)
    p32 = (imgs + 25.0).astype(np.float32)                                   # 15 A and more from every face of the smaller cell
    eng.set_system(z)
    cluster = eng.energy_forces_virial(p32)
    eng.set_cells(np.stack([np.eye(3) * 50.0, np.eye(3) * 55.0]), True)
    out = eng.energy_forces_virial(p32)
    assert eng.last_graph_shifts() == 27 and same_bits(out[0], cluster[0]) and same_bits(out[1], cluster[1])
    # (W sums r (x) g over edges whose vectors carry no translation here: the cluster's bits as well)
    assert same_bits(out[2], cluster[2])


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(eng):
    from pdb2reaction_amd.engine import UmxError

    z, p32, cells, pbc = family("triclinic", 4)
    eng.set_system(z)
    eng.set_cells(cells, pbc)
    before = eng.energy_forces_virial(p32)
    five = np.concatenate([p32, p32[:1]])
    for call in (eng.energy_forces, eng.energy_forces_virial):
        with pytest.raises(UmxError, match=r"5 images.*4"):
            call(five)
    assert same_efw(eng.energy_forces_virial(p32), before)

    def refused(bad, match):
        with pytest.raises(UmxError, match=match):
            eng.set_cells(bad, pbc)
        assert same_efw(eng.energy_forces_virial(p32), before)                # the cells that were in force stay in force

    bad = cells.copy()
    bad[2, 1] = 2.0 * bad[2, 0]                                              # two parallel lattice vectors
    refused(bad, r"image 2.*degenerate")
    bad = cells.copy()
    bad[3, 1, 1] = np.inf
    refused(bad, r"image 3.*non-finite")
    bad = cells.copy()
    bad[1] = TRICLINIC * 0.2
    refused(bad, r"image 1.*more than the 4 lattice translations")
    # the C level: UMX_ERR_ARG = -1
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    bad = np.ascontiguousarray(cells.copy())
    bad[2] = 0.0
    flags = np.ones(3, dtype=np.intc)
    assert eng.lib.umx_set_cells(eng._h, 4, bad.ctypes.data_as(dp), flags.ctypes.data_as(ip)) == -1
    assert b"image 2" in eng.lib.umx_last_error(eng._h)
    assert eng.lib.umx_set_cells(eng._h, 0, bad.ctypes.data_as(dp), flags.ctypes.data_as(ip)) == -1
    assert same_efw(eng.energy_forces_virial(p32), before)


def test_gp_begin_takes_one_bound_cell_only(eng):
    from pdb2reaction_amd.engine import UmxError

    z, p32, cells, pbc = family("triclinic", 2)
    n = len(z)
    dev = torch.device("cuda", 0)
    eng.set_system(z)
    pos = torch.from_numpy(p32[0]).to(dev)
    e_t, f_t = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(n, 3, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    eng.set_cells(cells, pbc)
    with pytest.raises(UmxError, match=r"umx_gp_begin.*2 images"):
        eng.gp_begin(pos.data_ptr(), 0, n, e_t.data_ptr(), f_t.data_ptr())
    assert np.isfinite(eng.energy_forces(p32)[0]).all()                      # the engine stays usable

    def graph_parallel():                                                    # one rank owning every node: nothing to sum
        e_t.fill_(float("nan")); f_t.fill_(float("nan"))
        torch.cuda.synchronize(dev)
        eng.gp_begin(pos.data_ptr(), 0, n, e_t.data_ptr(), f_t.data_ptr())
        steps = 0
        while not eng.gp_step()[2]:
            steps += 1
        eng.synchronize()
        assert steps > 0
        return e_t.cpu().numpy(), f_t.cpu().numpy()

    eng.set_cell(cells[1], pbc)
    want = graph_parallel()
    eng.set_cells(cells[1:2], pbc)                                           # exactly one cell: as set_cell with it
    got = graph_parallel()
    assert np.isfinite(want[0]).all() and same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    eng.set_cell(cells[0], pbc)
    assert not same_bits(graph_parallel()[0], want[0])


# ---- 9. the pool, 10. the facade ---------------------------------------------------------------------------------------------------------
class _Atoms:
    def __init__(self, z, pos, cell, pbc):
        self.numbers, self._pos, self.cell, self.pbc, self.info = z, np.asarray(pos, dtype=np.float64), cell, pbc, {}

    def get_positions(self):
        return self._pos


def test_a_pool_of_two_engines_deals_the_cells_with_the_images(eng, weights):
    from pdb2reaction_amd.parallel import LocalEnginePool

    z, p32, cells, pbc = family("triclinic", 5)
    eng.set_system(z)
    eng.set_cells(cells, pbc)
    e0, f0, w0 = eng.energy_forces_virial(p32)
    s0 = eng.energy_forces_stress(p32)[2]
    eng.set_cell(cells[0], pbc)
    one = eng.energy_forces_virial(p32[0])
    with LocalEnginePool.create([0, 0], weights) as pool:
        pool.set_system(z)
        pool.set_cells(cells, pbc)
        e1, f1, s1 = pool.energy_forces_stress(p32)
        assert pool.last_route == "batch" and pool.last_blocks == [(0, 3), (3, 5)]
        assert same_bits(e1, e0) and same_bits(f1, f0) and same_bits(s1, s0)
        assert same_efw(pool.energy_forces_virial(p32), (e0, f0, w0))
        pool.set_cells(cells[:1], pbc)                                       # K = 1: set_cell(cells[0]) on the engines
        assert same_efw(pool.energy_forces_virial(p32[0]), one) and pool.last_route == "single"
        e2, f2 = pool.energy_forces(p32[0])                                  # ... also for the graph-parallel route
        assert pool.last_route == "graph-parallel" and abs(e2[0] - one[0][0]) <= TOL_E
        pool.set_cell(cells[0], pbc)
        e3, f3 = pool.energy_forces(p32[0])
        assert pool.last_route == "graph-parallel" and same_bits(e3, e2) and same_bits(f3, f2)
        pool.set_cells(cells, pbc)                                           # and back to the batch
        assert same_efw(pool.energy_forces_virial(p32), (e0, f0, w0))


def test_the_facade_with_per_image_cells(eng, monkeypatch):
    A = importlib.import_module("pdb2reaction_amd.ase_calculator")
    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    z, p32, cells, pbc = family("triclinic", 4)
    eng.set_system(z)
    eng.set_cells(cells, pbc)
    e0, f0, s0 = eng.energy_forces_stress(p32)
    calc = A.UMXCalculator(model="synthetic", stress=True)
    try:
        images = [_Atoms(z, p, c, pbc) for p, c in zip(p32, cells)]
        with pytest.raises(ValueError, match="share the cell"):
            calc.calculate_images(images, stress=True)                       # the default is one cell per call
        e1, f1, s1 = calc.calculate_images(images, stress=True, per_image_cells=True)
        assert same_bits(e1, e0) and same_bits(f1, f0.astype(np.float64)) and same_bits(s1, s0)
        assert calc.get_potential_energy(images[0]) == e0[0]                 # the single-image path binds its cell again
        assert same_bits(calc.get_stress(images[0]), s0[0])
        e2, f2 = calc.calculate_images(images, per_image_cells=True)
        assert same_bits(e2, e0) and same_bits(f2, f0.astype(np.float64))
    finally:
        calc.close()
