"""Pinned graphs per image on the GPU (``umx_pin_graphs`` / ``umx_pin_assign``): every image of a batch replays the edge set of its own
reference.

Yardsticks.  Exact: pinned at the references, a batch of the references is the unpinned batch in every bit of E, F, W and of the graph
buffers; image k of any batch, under any plan, is bitwise the evaluation of that image alone on an engine with ``pin_graph`` of its
reference.  Float64: ``PeriodicOracle.model_energy(graph=...)`` (tests/pinned_cases.py) at the project's bounds |dE| <= 1e-4 eV,
max|dF| <= 1e-3 eV/A.  The reference sets and their edge counts are those of tests/pinned_graphs_cases.py, which
tests/test_pinned_graphs_cpu.py holds to the checker.

Synthetic weights seed 0, default precision.  Every case is a handful of evaluations of at most 48 atoms."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import pinned_cases as PC
import pinned_graphs_cases as GC
from test_gpu_periodic import TOL_E, TOL_F
from pdb2reaction_amd.engine import UmxError

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_efw(a, b):
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


def image_of(out, k):
    """Image k of a batch result (E, F[, W]) as a batch of one."""
    return tuple(x[k: k + 1] for x in out)


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


def lib_pinned_graphs(e, capacity=8):
    """(references, edges of the first ``capacity`` of them, max degree) straight from ``umx_pinned_graphs``."""
    ne, md = (C.c_int64 * max(capacity, 1))(*([-1] * max(capacity, 1))), C.c_int32(-1)
    n = e.lib.umx_pinned_graphs(e._h, capacity, ne, C.byref(md))
    return n, tuple(int(ne[r]) for r in range(min(max(n, 0), capacity))), int(md.value)


def lib_pinned_total(e):
    ne, md = C.c_int64(-1), C.c_int32(-1)
    assert e.lib.umx_pinned_graph(e._h, C.byref(ne), C.byref(md)) == 0
    return int(ne.value), int(md.value)


def bind(e, case):
    z, refs, cell, pbc, max_neigh = case
    e.set_system(z, max_neigh=max_neigh)
    e.set_cell(cell, pbc)


# ---- 1. at the references ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double", [False, True], ids=["float", "double"])
@pytest.mark.parametrize("name", ["open12_capped", "open40", "triclinic_capped", "slab", "triclinic_mid"])
def test_pinned_at_the_references_is_the_unpinned_batch(eng, name, double):
    """Pinned at its references, the batch of the references is the unpinned batch in every bit of E, F, W and of the graph buffers, and
    every image of it is the unpinned evaluation of that reference ALONE.  ``triclinic_mid`` has its odd count (595) in the middle: the
    unpinned batch then has reference 2 at an odd row of its one chunk and differs from its own single evaluations by float32 rounding
    (pinned_graphs_cases.py), so there the pinned batch is held to the singles and to the unpinned batch within TOL_E / TOL_F."""
    case = GC.reference_set(name)
    z, refs = case[0], case[1]
    _, edges, maxdeg = GC.EXPECTED[name]
    if double:      # float64 positions that float32 does not hold: the double entry's own differences
        refs = refs.astype(np.float64) + 1e-6 * np.random.default_rng(1).standard_normal(refs.shape)
    kw = {"double_positions": True} if double else {}
    bind(eng, case)
    alone = [eng.energy_forces_virial(r, **kw) for r in refs]
    eng.debug_keep(True)

    def run():
        out = eng.energy_forces_virial(refs, **kw)
        return out, (eng.debug_fetch("src", np.int32), eng.debug_fetch("dst", np.int32), eng.debug_fetch("evec", np.float32)), eng.graph_stats()

    free, g_free, stats = run()
    assert eng.pinned_graphs() is None and lib_pinned_graphs(eng) == (0, (), 0)
    eng.pin_graphs(refs, **kw)
    counts, md = eng.pinned_graphs()
    print(f"[references {name} {'double' if double else 'float'}] edges per reference {counts}, largest in-degree {md}")
    assert len(set(counts)) > 1                                              # the references do differ in their graphs
    if not double:
        assert (counts, md) == (edges, maxdeg)                               # the counts the CPU test holds to the checker
    assert lib_pinned_graphs(eng) == (3, counts, md) and lib_pinned_total(eng) == (sum(counts), md)
    assert stats == (sum(counts), md)
    pinned, g_pin, stats_pin = run()
    assert stats_pin == stats and len(g_free[0]) == stats[0] and len(g_free[2]) == 4 * stats[0]
    for k in range(len(refs)):
        assert same_efw(image_of(pinned, k), alone[k]), (name, double, k)
    if GC.behind_odd(counts):
        de, df = np.abs(pinned[0] - free[0]).max(), np.abs(pinned[1] - free[1]).max()
        print(f"[references {name}] an image behind an odd count: pinned against the unpinned batch max|dE| = {de:.3e} eV  max|dF| = {df:.3e} eV/A")
        assert de <= TOL_E and df <= TOL_F
        assert same_efw(image_of(pinned, 0), image_of(free, 0)) and same_efw(image_of(pinned, 1), image_of(free, 1))
    else:
        assert same_efw(pinned, free), (name, double)
        for a, b, what in zip(g_pin, g_free, ("src", "dst", "evec")):
            assert same_bits(a, b), (what, name, double)
    eng.unpin_graph()
    assert eng.pinned_graphs() is None and lib_pinned_graphs(eng) == (0, (), 0) and lib_pinned_total(eng) == (0, 0)
    again, g_again, _ = run()
    assert same_efw(again, free) and all(same_bits(a, b) for a, b in zip(g_again, g_free))
    eng.debug_keep(False)


# ---- 2. image for image --------------------------------------------------------------------------------------------------------------------
def singles_of(weights, case, ys, assign, **engine_kw):
    """[(E, F, W) of ys[k] alone on an engine with ``pin_graph(refs[assign[k]])``], one engine for all of them."""
    e_ = new_engine(weights, **engine_kw)
    try:
        bind(e_, case)
        out = []
        for k, a in enumerate(assign):
            e_.pin_graph(case[1][a])
            out.append(e_.energy_forces_virial(ys[k]))
            stats = (e_.last_partitions(), e_.last_recompute(), e_.last_lanes())
        return out, stats
    finally:
        e_.close()


IMAGE_SETS = ("open12_even", "open40", "open12_capped", "triclinic_mid")


@pytest.fixture(scope="module")
def image_cases(weights):
    """name -> (case, Y, the single-pin results of every image in one piece): computed once, left unchanged."""
    out = {}
    for name in IMAGE_SETS:
        case = GC.reference_set(name)
        ys = GC.displaced(case[1], GC.ASSIGN)
        singles, stats = singles_of(weights, case, ys, GC.ASSIGN)
        assert stats == (0, 0, 1)
        out[name] = (case, ys, singles)
    return out


SETTINGS = {
    # name: (environment, engine keywords, (partitions, recompute, lanes) the batch must report)
    "plain": ({}, {}, (0, 0, 1)),
    "chunk2": ({"UMX_MAX_CHUNK_IMAGES": "2"}, {}, (0, 0, 1)),
    "chunk1": ({"UMX_MAX_CHUNK_IMAGES": "1"}, {}, (0, 0, 1)),              # the empty reference is then a chunk without edges
    "streams2": ({"UMX_STREAMS": "2"}, {}, (0, 0, 2)),
    "recompute2": ({}, {"recompute": 2}, (0, 1, 1)),
    "parts2": ({"UMX_FORCE_PARTS": "2"}, {}, (2, 0, 1)),
    "parts3": ({"UMX_FORCE_PARTS": "3"}, {}, (3, 0, 1)),
    "plain_rows": ({"UMX_ALT_ROWS": "0"}, {}, (0, 0, 1)),                  # without the sign-alternating operand rows (see the docstring)
}
SAME_ENV_SINGLES = ("parts2", "parts3", "plain_rows")                       # the single-pin evaluations under the setting's own environment


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", IMAGE_SETS)
def test_image_for_image(weights, image_cases, monkeypatch, name, setting):
    """Image k of the batch Y[0..4] with assignment [2, 0, 0, 1, 2] is bitwise (E, F, W) Y[k] alone on ``pin_graph(refs[a[k]])``.

    ``open12_capped`` and ``triclinic_mid`` put images behind an odd number of edges (47, 595).  The GEMM producers negate the operand
    rows of odd index and the epilogues restore the sign (umx_edge.h, "sign-alternating rows"; on by default), so the float32
    rounding of an edge depends on the parity of its row in the chunk; at an odd row the image would differ from the image alone by
    rounding (measured before the planner knew: max|dE| = 1.0e-06 eV, max|dF| = 3.6e-07 eV/A, max|dW| = 1.4e-06 eV,
    profiles/pinned_graphs.txt part 1).  With several references pinned the planner ends a chunk behind an odd count, so every image
    starts at an even row; ``plain_rows`` (UMX_ALT_ROWS=0) runs the same batches with the alternating rows off."""
    case, ys, singles = image_cases[name]
    env, engine_kw, want = SETTINGS[setting]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    edges = GC.EXPECTED[name][1]
    if setting in SAME_ENV_SINGLES:
        # partitions differ from one piece at float32 summation order: each image against the single-pin evaluation at the SAME count
        singles, stats = singles_of(weights, case, ys, GC.ASSIGN)
        assert stats == want
    e_ = new_engine(weights, **engine_kw)
    try:
        bind(e_, case)
        e_.pin_graphs(case[1], assign=GC.ASSIGN)
        assert e_.pinned_graphs() == (edges, GC.EXPECTED[name][2])
        out = e_.energy_forces_virial(ys)
        assert (e_.last_partitions(), e_.last_recompute(), e_.last_lanes()) == want, setting
        assert e_.graph_stats() == (sum(edges[a] for a in GC.ASSIGN), GC.EXPECTED[name][2])
        worst = [max(float(np.abs(np.asarray(out[q][k], dtype=np.float64) - np.asarray(singles[k][q][0], dtype=np.float64)).max())
                     for k in range(len(GC.ASSIGN))) for q in range(3)]
        print(f"[image for image {name} {setting}] against the single pins: max|dE| = {worst[0]:.3e} eV  max|dF| = {worst[1]:.3e} eV/A  max|dW| = {worst[2]:.3e} eV")
        for k in range(len(GC.ASSIGN)):
            assert same_efw(image_of(out, k), singles[k]), (name, setting, k)
        # the pin matters here: unpinned, some of the displaced images have other graphs (tests/test_pinned_graphs_cpu.py)
        e_.unpin_graph()
        free = e_.energy_forces_virial(ys)
        assert not same_bits(free[0], out[0])
    finally:
        e_.close()


# ---- 3. each image keeps its own graph -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def swaps(weights):
    out = {}
    for name in ("cluster", "triclinic"):
        if name == "cluster":
            z, orc, x0, xm = PC.cluster_swap(weights)[:4]
            cell = pbc = None
        else:
            z, orc, cell, pbc, x0, xm = PC.triclinic_swap(weights)[:6]
        g0, gm = PC.graph_of(orc, x0), PC.graph_of(orc, xm)
        out[name] = dict(z=z, cell=cell, pbc=pbc, x0=x0, xm=xm, g0=g0, gm=gm, on_start=PC.energy_forces_on(orc, z, xm, g0),
                         on_moved=PC.energy_forces_on(orc, z, xm, gm))
    return out


@pytest.mark.parametrize("name", ["cluster", "triclinic"])
def test_each_image_keeps_its_own_graph(eng, swaps, name):
    s = swaps[name]
    gap = abs(s["on_start"][0] - s["on_moved"][0])
    print(f"[own graph {name}] the checker at x_moved on the graph of x_start and on that of x_moved: |dE| = {gap:.4f} eV")
    assert not PC.same_graph(s["g0"], s["gm"]) and gap > 100 * TOL_E
    eng.set_system(s["z"], max_neigh=PC.MAX_NEIGH)
    eng.set_cell(s["cell"], s["pbc"])
    eng.pin_graphs(np.stack([s["x0"], s["xm"]]))
    assert eng.pinned_graphs() == ((len(s["g0"][0]), len(s["gm"][0])), PC.MAX_NEIGH)
    e, f = eng.energy_forces(np.stack([s["xm"], s["xm"]]))
    for k, ref in enumerate((s["on_start"], s["on_moved"])):
        de, df = abs(e[k] - ref[0]), float(np.abs(f[k] - ref[1]).max())
        print(f"[own graph {name}] image {k} against the checker on the graph of reference {k}: |dE| = {de:.3e} eV  max|dF| = {df:.3e} eV/A")
        assert de <= TOL_E and df <= TOL_F
    assert abs(e[0] - e[1]) > 50 * TOL_E                                     # the same geometry twice, two graphs, two energies


# ---- 4. cells after the pin ----------------------------------------------------------------------------------------------------------------
def test_cells_after_the_pin(eng, weights):
    case = GC.reference_set("triclinic_pair")            # (even edge counts: every image at an even offset, see pinned_graphs_cases.py)
    z, refs, cell, pbc, max_neigh = case
    assign = [0, 1, 0, 1]
    cells = GC.strained_cells(cell)
    ys = GC.displaced(refs, assign, seed=5)
    bind(eng, case)
    eng.pin_graphs(refs)
    counts = eng.pinned_graphs()[0]
    assert counts == GC.EXPECTED["triclinic_pair"][1] and counts[0] != counts[1]
    eng.set_cells(cells, pbc)                                                # the same flags: the pins stay, the translations follow the cells
    eng.pin_assign(assign)
    assert eng.pinned_graphs()[0] == counts
    out = eng.energy_forces_virial(ys)
    assert eng.graph_stats()[0] == sum(counts[a] for a in assign)
    one = new_engine(weights)
    try:
        bind(one, case)
        for k, a in enumerate(assign):
            one.set_cell(cell, pbc)
            one.pin_graph(refs[a])
            one.set_cell(cells[k], pbc)
            assert same_efw(image_of(out, k), one.energy_forces_virial(ys[k])), k
    finally:
        one.close()
    # the strained cells matter: in the cell of pin time image 0 is another number
    eng.set_cell(cell, pbc)
    eng.pin_assign([0])
    assert not same_bits(eng.energy_forces_virial(ys[0])[0], out[0][:1])


# ---- 5. one reference ----------------------------------------------------------------------------------------------------------------------
def test_one_reference_is_pin_graph(eng, weights):
    case = GC.reference_set("open12_capped")
    refs = case[1]
    x = refs[0]
    moved = GC.displaced(refs, [0] * 5, seed=7)
    bind(eng, case)
    free = [eng.energy_forces_virial(moved[:1]), eng.energy_forces_virial(moved)]
    eng.pin_graph(x)
    old = [eng.energy_forces_virial(moved[:1]), eng.energy_forces_virial(moved)]
    total, stats = lib_pinned_total(eng), eng.graph_stats()
    eng.pin_graphs(x[None])
    assert eng.pinned_graphs() == ((total[0],), total[1]) and lib_pinned_total(eng) == total
    new = [eng.energy_forces_virial(moved[:1]), eng.energy_forces_virial(moved)]
    assert eng.graph_stats() == stats == (5 * total[0], total[1])
    assert same_efw(new[0], old[0]) and same_efw(new[1], old[1])
    assert not same_bits(old[1][0], free[1][0])                              # (the moved images do have other graphs)
    eng.unpin_graph()
    assert same_efw(eng.energy_forces_virial(moved[:1]), free[0]) and same_efw(eng.energy_forces_virial(moved), free[1])


# ---- 6. rules ------------------------------------------------------------------------------------------------------------------------------
def refused(fn, match):
    with pytest.raises(UmxError, match=match) as ei:
        fn()
    assert ei.value.status == -1                                             # UMX_ERR_ARG


def test_the_rules(eng, weights):
    case = GC.reference_set("triclinic_capped")
    z, refs, cell, pbc, max_neigh = case
    two, ys = refs[:2], GC.displaced(refs, [0, 1, 1], seed=9)
    refused(lambda: eng.pin_graphs(np.zeros((2, 0, 3))), "bind a system first")
    bind(eng, case)
    refused(lambda: eng.pin_assign([0]), "nothing is pinned")
    eng.pin_graphs(two)
    n, counts, md = lib_pinned_graphs(eng)
    assert n == 2 and counts == GC.EXPECTED["triclinic_capped"][1][:2]
    assert lib_pinned_graphs(eng, capacity=1) == (2, counts[:1], md) and lib_pinned_graphs(eng, capacity=0)[0] == 2
    # the image count: the default of two references is two images ...
    refused(lambda: eng.energy_forces(ys), r"3 images.*2 graphs are pinned")
    default = eng.energy_forces_virial(ys[:2])
    # ... and an assignment holds for its own number of images
    eng.pin_assign([0, 1, 1])
    refused(lambda: eng.energy_forces(ys[:2]), r"2 images.*umx_pin_assign.*3")
    assigned = eng.energy_forces_virial(ys)
    assert same_efw(image_of(assigned, 0), image_of(default, 0)) and same_efw(image_of(assigned, 1), image_of(default, 1))
    # an entry out of range: refused, the old assignment stays in force
    refused(lambda: eng.pin_assign([0, 2, 0]), r"image 1 names reference 2")
    refused(lambda: eng.pin_assign([0, -1, 0]), r"image 1 names reference -1")
    refused(lambda: eng.energy_forces(ys[:2]), "2 images")
    assert same_efw(eng.energy_forces_virial(ys), assigned)
    # a non-finite coordinate in reference 1 of 2: the whole call is refused, it names the reference, the previous pin stays in force
    bad = two.copy()
    bad[1, 3, 1] = np.nan
    refused(lambda: eng.pin_graphs(bad), r"non-finite.*reference 1")
    refused(lambda: eng.pin_graphs(bad.astype(np.float64), double_positions=True), r"non-finite.*reference 1")
    assert lib_pinned_graphs(eng) == (2, counts, md) and same_efw(eng.energy_forces_virial(ys), assigned)
    # None restores the default
    eng.pin_assign(None)
    assert same_efw(eng.energy_forces_virial(ys[:2]), default)
    # re-pinning resets the assignment
    eng.pin_graphs(two, assign=[1, 1, 0])
    eng.energy_forces(ys)
    eng.pin_graphs(two)
    refused(lambda: eng.energy_forces(ys), "3 images")
    assert same_efw(eng.energy_forces_virial(ys[:2]), default)
    # per-image cells bound at pin time: several references are refused (and what was pinned stays); one reference, one cell is pin_graph
    eng.set_cells(np.stack([cell, cell * 1.01]), pbc)
    assert lib_pinned_graphs(eng) == (2, counts, md)                         # (same flags: the pins stay)
    refused(lambda: eng.pin_graphs(two), "per-image cells")
    assert lib_pinned_graphs(eng) == (2, counts, md)
    # a strained cell with the same flags keeps the pins; other flags unpin
    eng.set_cell(cell * 1.01, pbc)
    assert lib_pinned_graphs(eng) == (2, counts, md) and eng.pinned_graphs() is not None
    eng.set_cell(cell, pbc)
    assert same_efw(eng.energy_forces_virial(ys[:2]), default)
    eng.set_cell(cell, (True, True, False))
    assert lib_pinned_graphs(eng) == (0, (), 0) and eng.pinned_graphs() is None
    eng.set_cell(cell, pbc)
    free = eng.energy_forces_virial(ys[:2])
    assert not same_bits(free[0], default[0])
    # set_system unpins
    eng.pin_graphs(two, assign=[1, 0])
    eng.set_system(z, max_neigh=max_neigh)
    assert lib_pinned_graphs(eng) == (0, (), 0) and eng.pinned_graphs() is None and same_efw(eng.energy_forces_virial(ys[:2]), free)
    # the graph-parallel entry refuses while anything is pinned
    eng.pin_graphs(two)
    pos = torch.tensor(ys[0], device="cuda")
    e_t = torch.zeros(1, dtype=torch.float64, device="cuda")
    f_t = torch.zeros(len(z), 3, dtype=torch.float32, device="cuda")
    w_t = torch.zeros(9, dtype=torch.float64, device="cuda")
    refused(lambda: eng.gp_begin(pos.data_ptr(), 0, len(z), e_t.data_ptr(), f_t.data_ptr()), r"umx_gp_begin.*pinned")
    refused(lambda: eng.gp_begin(pos.data_ptr(), 0, len(z), e_t.data_ptr(), f_t.data_ptr(), d_virial=w_t.data_ptr()), r"umx_gp_begin.*pinned")
    # the with block unpins on an exception
    eng.unpin_graph()
    with pytest.raises(KeyError):
        with eng.pinned_each(two, assign=[1, 0, 1]):
            assert lib_pinned_graphs(eng) == (2, counts, md)
            eng.energy_forces(ys)
            raise KeyError("inside")
    assert lib_pinned_graphs(eng) == (0, (), 0) and eng.pinned_graphs() is None
    assert same_efw(eng.energy_forces_virial(ys[:2]), free)


# ---- 7. pool and facade --------------------------------------------------------------------------------------------------------------------
class _Atoms:
    def __init__(self, z, pos, cell, pbc):
        self.numbers, self._pos, self.cell, self.pbc, self.info = z, np.asarray(pos, dtype=np.float64), cell, pbc, {}

    def get_positions(self):
        return self._pos


def test_a_pool_of_two_engines_on_one_device(weights, image_cases, monkeypatch):
    from pdb2reaction_amd.engine import Engine
    from pdb2reaction_amd.parallel import LocalEnginePool, local_devices_for

    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,0")
    case, ys, singles = image_cases["open12_even"]
    edges = GC.EXPECTED["open12_even"][1]
    pool = LocalEnginePool.create(local_devices_for(2), weights, engine_factory=Engine)
    try:
        assert len(pool) == 2
        pool.set_system(case[0], max_neigh=case[4])
        with pool.pinned_each(case[1], assign=GC.ASSIGN):
            assert pool.pinned_graphs() == (edges, GC.EXPECTED["open12_even"][2])
            out = pool.energy_forces_virial(ys)
            assert pool.last_route == "batch" and pool.last_blocks == [(0, 3), (3, 5)]
            for k in range(len(GC.ASSIGN)):
                assert same_efw(image_of(out, k), singles[k]), k
            e, f = pool.energy_forces(ys)
            assert same_bits(e, out[0]) and same_bits(f, out[1])
            pool.pin_assign([GC.ASSIGN[3]])                                  # a single geometry: engine 0 alone, with its one entry
            e1, f1 = pool.energy_forces(ys[3])
            assert pool.last_route == "single" and same_bits(e1, singles[3][0]) and same_bits(f1, singles[3][1])
        assert pool.pinned_graphs() is None and all(lib_pinned_graphs(e_) == (0, (), 0) for e_ in pool.engines)
    finally:
        pool.close()


def test_the_facade_pins_every_image_at_its_own_geometry(eng, monkeypatch):
    case = GC.reference_set("triclinic_capped")
    z, refs, cell, pbc, max_neigh = case
    bind(eng, case)
    with eng.pinned_each(refs):
        want = eng.energy_forces(refs)
    moved = GC.displaced(refs, [0, 1, 2], seed=11)
    with eng.pinned_each(refs):
        want_moved = eng.energy_forces(moved)
    A = importlib.import_module("pdb2reaction_amd.ase_calculator")
    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    calc = A.UMXCalculator(model="synthetic", max_neigh=max_neigh)
    try:
        atoms = [_Atoms(z, p, cell, pbc) for p in refs]
        with calc.pinned_each(atoms):
            assert calc._engine.pinned_graphs()[0] == GC.EXPECTED["triclinic_capped"][1]
            e, f = calc.calculate_images(atoms)
            e2, f2 = calc.calculate_images([_Atoms(z, p, cell, pbc) for p in moved])
        assert same_bits(e, want[0]) and same_bits(f, want[1].astype(np.float64))
        assert same_bits(e2, want_moved[0]) and same_bits(f2, want_moved[1].astype(np.float64))
        assert lib_pinned_graphs(calc._engine) == (0, (), 0)
        with pytest.raises(ValueError, match="per_image_cells"):
            calc.pinned_each(atoms, per_image_cells=True)
    finally:
        calc.close()
