"""Pinned graphs per image without a GPU: the conditions of the cases (tests/pinned_graphs_cases.py) against the float64 checker, so that
no GPU test passes vacuously; the C ABI's declarations against the ctypes binding; and ``LocalEnginePool``'s dealing of assignment slices
over its blocks against stand-in engines that record what reaches them."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import pinned_cases as PC
import pinned_graphs_cases as GC
from test_gpu_periodic import TOL_E
from pdb2reaction_amd import parallel as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def test_the_edge_counts_of_the_issue_at_the_checkers_own_cutoff(weights):
    cutoff = PC.checker(weights).cutoff
    for (n, seed, scale, max_neigh), edges in GC.TABLE:
        _, x = GC.scaled_cluster(n, seed, scale)
        assert GC.checker_counts(x, None, None, max_neigh, cutoff)[0] == edges, (n, seed, scale, max_neigh)
    assert all(e > 256 and e % 64 for e in (1206, 764, 288))                 # an image's edges cross block and wave boundaries
    assert 48 + 0 + 47 < 256                                                 # several whole images in one 256-thread block


@pytest.mark.parametrize("name", sorted(GC.EXPECTED))
def test_the_reference_sets_have_unequal_graphs(weights, name):
    cutoff = PC.checker(weights).cutoff
    z, refs, cell, pbc, max_neigh = GC.reference_set(name)
    _, edges, maxdeg = GC.EXPECTED[name]
    got = [GC.checker_counts(r, cell, pbc, max_neigh, cutoff) for r in refs]
    assert tuple(g[0] for g in got) == edges and max(g[1] for g in got) == maxdeg
    assert len(set(edges)) > 1 and len(z) == refs.shape[1]
    if max_neigh is not None:
        assert maxdeg == max_neigh                                           # the cap binds
    if name in ("open12_capped", "open12_even"):
        assert edges[1] == 0 and edges[0] > 0 and edges[2] > 0               # the empty reference BETWEEN two non-empty ones
    # row parity (pinned_graphs_cases.py): the one set whose references, in their order, put an image behind an odd number of edges --
    # and the sets of test 2 that do so under its assignment
    assert GC.behind_odd(edges) == (name == "triclinic_mid")
    if len(refs) == 3:
        assert GC.behind_odd([edges[a] for a in GC.ASSIGN]) == (name in ("open12_capped", "triclinic_capped", "triclinic_mid"))
    if len(refs) < 3:
        return
    # the images of test 2 are other geometries than their references, and every reference is used
    y = GC.displaced(refs, GC.ASSIGN)
    assert len(GC.ASSIGN) != len(refs) and set(GC.ASSIGN) == set(range(len(refs))) and GC.ASSIGN != sorted(GC.ASSIGN)
    assert all(np.abs(y[k] - refs[a]).max() > 1e-3 for k, a in enumerate(GC.ASSIGN))
    # ... and at least one of them has another graph than its reference when it is rebuilt: there the pin matters
    def edge_set(pos):
        from periodic_oracle import periodic_radius_graph

        src, dst, _, tidx = periodic_radius_graph(np.asarray(pos, dtype=np.float64), cell, pbc, cutoff, max_neigh)
        return set(zip(src.tolist(), dst.tolist(), tidx.tolist()))

    assert any(edge_set(y[k]) != edge_set(refs[a]) for k, a in enumerate(GC.ASSIGN))


@pytest.mark.parametrize("name", ["cluster", "triclinic"])
def test_the_rank_swap_pair_has_two_graphs_that_matter(weights, name):
    """Test 3's precondition: on the graphs of ``x_start`` and of ``x_moved`` the checker's energies at ``x_moved`` differ by more than
    100 TOL_E (the condition of ``test_the_rank_swap``)."""
    if name == "cluster":
        z, orc, x0, xm = PC.cluster_swap(weights)[:4]
    else:
        z, orc, _, _, x0, xm = PC.triclinic_swap(weights)[:6]
    g0, gm = PC.graph_of(orc, x0), PC.graph_of(orc, xm)
    assert not PC.same_graph(g0, gm)
    de = abs(PC.energy_on(orc, z, xm, g0) - PC.energy_on(orc, z, xm, gm))
    print(f"[swap {name}] the checker on the two graphs at x_moved: |dE| = {de:.4f} eV")
    assert de > 100 * TOL_E


def test_the_strained_cells_are_four_other_cells():
    cell = GC.reference_set("triclinic_capped")[2]
    cells = GC.strained_cells(cell)
    assert cells.shape == (4, 3, 3) and all(np.abs(c - cell).max() > 1e-3 for c in cells)
    assert len({c.tobytes() for c in cells}) == 4


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_the_four_new_exports_and_their_ctypes_signatures():
    from pdb2reaction_amd import engine as E

    lib = E.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "umx.h")).read(), flags=re.S)
    vp, fp, dp, i32 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double), ctypes.c_int
    decl = {
        "umx_pin_graphs": r"int\s+umx_pin_graphs\s*\(\s*umx_engine\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*\)",
        "umx_pin_graphs_f64": r"int\s+umx_pin_graphs_f64\s*\(\s*umx_engine\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+double\s*\*\s*\w+\s*\)",
        "umx_pin_assign": r"int\s+umx_pin_assign\s*\(\s*umx_engine\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*\)",
        "umx_pinned_graphs": r"int\s+umx_pinned_graphs\s*\(\s*const\s+umx_engine\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int64_t\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)",
    }
    for sym, pattern in decl.items():
        assert re.search(pattern, txt), sym
        assert hasattr(lib, sym) and sym in (E.EXPORTED_SYMBOLS_F64 if sym.endswith("f64") else E.EXPORTED_SYMBOLS)
    assert lib.umx_abi_version() == 10                                       # additive: no version bump
    assert lib.umx_pin_graphs.argtypes == [vp, i32, fp] and lib.umx_pin_graphs_f64.argtypes == [vp, i32, dp]
    assert lib.umx_pin_assign.argtypes == [vp, i32, ctypes.POINTER(ctypes.c_int32)]
    assert lib.umx_pinned_graphs.argtypes == [vp, i32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)]
    # no engine: refused, not a crash
    assert lib.umx_pin_graphs(None, 2, None) != 0 and lib.umx_pin_graphs_f64(None, 2, None) != 0
    assert lib.umx_pin_assign(None, 0, None) != 0 and lib.umx_pinned_graphs(None, 0, None, None) < 0
    for name in ("pin_graphs", "pin_assign", "pinned_graphs", "pinned_each"):
        assert callable(getattr(E.Engine, name)) and callable(getattr(P.LocalEnginePool, name))
    full = open(os.path.join(ROOT, "include", "umx.h")).read()
    assert "one graph per image of a batch" not in full                      # no longer among what is not provided


# ---- LocalEnginePool: every image reaches its engine with the reference the caller gave -----------------------------------------------
class _Engine:
    """Stand-in engine: keeps its pins and its assignment by the engine's rules, and records (image tag, reference) of every image it
    evaluates.  Images carry their index within the call in coordinate [0, 0]."""

    def __init__(self, log, name, device, refuse_pin=False):
        self.log, self.name, self.device, self.natoms, self.widened, self.refuse_pin = log, name, device, 3, False, refuse_pin
        self.refs, self.assign = 0, None

    def set_system(self, z, **kw):
        self.natoms, self.refs, self.assign = len(z), 0, None

    def pin_graph(self, pos, **kw):
        self.refs, self.assign = 1, None

    def pin_graphs(self, refs, **kw):
        assert "assign" not in kw                                            # the pool deals the assignment itself
        if self.refuse_pin:
            raise RuntimeError("refused")
        self.refs, self.assign = len(refs), None

    def pin_assign(self, assign=None):
        assert self.refs > 0
        if assign is not None and any(a < 0 or a >= self.refs for a in assign):
            raise RuntimeError("out of range")
        self.assign = None if assign is None else tuple(assign)

    def unpin_graph(self):
        self.refs, self.assign = 0, None
        self.log.append((self.name, "unpin"))

    def _refs_of(self, k):
        if self.assign is not None:
            assert len(self.assign) == k, (self.name, self.assign, k)
            return self.assign
        assert self.refs == 1 or self.refs == k, (self.name, self.refs, k)
        return tuple(range(k)) if self.refs > 1 else (0,) * k

    def energy_forces(self, p, forces=True, **kw):
        for img, ref in zip(p, self._refs_of(len(p))):
            self.log.append((self.name, int(round(float(img[0, 0]))), ref))
        return np.zeros(len(p)), np.zeros(np.shape(p), np.float32)

    def energy_forces_virial(self, p, **kw):
        e, f = self.energy_forces(p)
        return e, f, np.zeros((len(p), 3, 3))

    def close(self):
        pass


def _pool(log, g=3, refuse_last=False):
    engines = [_Engine(log, f"e{r}", r, refuse_pin=refuse_last and r == g - 1) for r in range(g)]
    pool = P.LocalEnginePool(engines, gp=True, peer_sum=lambda *a: None, tensor_device=lambda e: torch.device("cpu"))
    pool.natoms = 3
    return pool


def _images(k):
    p = np.zeros((k, 3, 3), np.float32)
    p[:, 0, 0] = np.arange(k)
    return p


def _seen(log):
    return sorted((tag, ref) for _, tag, ref in (entry for entry in log if len(entry) == 3))


@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_the_pool_deals_the_slices_of_the_assignment_over_its_blocks(g):
    log = []
    pool = _pool(log, g)
    try:
        refs = np.zeros((3, 3, 3), np.float32)
        pool.pin_graphs(refs, assign=GC.ASSIGN)
        for call in (pool.energy_forces, pool.energy_forces_virial):
            del log[:]
            call(_images(5))
            assert pool.last_route == "batch" and _seen(log) == list(enumerate(GC.ASSIGN))
            by_engine = {name for name, _, _ in log}
            assert len(by_engine) == min(g, 5)                               # contiguous blocks over all engines, as without a pin
        # another assignment of the same length: every engine gets its new slice
        del log[:]
        pool.pin_assign([0, 1, 2, 2, 1])
        pool.energy_forces(_images(5))
        assert _seen(log) == list(enumerate([0, 1, 2, 2, 1]))
        # a wrong image count is refused before any engine evaluates; an out-of-range entry leaves the assignment in force
        del log[:]
        with pytest.raises(ValueError, match="4 images"):
            pool.energy_forces(_images(4))
        with pytest.raises(ValueError, match=r"\[0, 3\)"):
            pool.pin_assign([0, 3, 0, 0, 0])
        assert log == []
        pool.energy_forces(_images(5))
        assert _seen(log) == list(enumerate([0, 1, 2, 2, 1]))
        # the default with three references: image k replays reference k, whatever block it falls into
        del log[:]
        pool.pin_assign(None)
        pool.energy_forces(_images(3))
        assert _seen(log) == [(0, 0), (1, 1), (2, 2)]
        with pytest.raises(ValueError, match="5 images"):
            pool.energy_forces(_images(5))
        # a single geometry goes to engine 0 alone, with its one entry
        del log[:]
        pool.pin_assign([2])
        pool.energy_forces(_images(1)[0])
        assert pool.last_route == "single" and log == [("e0", 0, 2)]
        # pinning again resets the assignment; unpinning drops it
        pool.pin_graphs(refs)
        del log[:]
        pool.energy_forces(_images(3))
        assert _seen(log) == [(0, 0), (1, 1), (2, 2)]
        pool.unpin_graph()
        assert pool.pinned_graphs() is None
        with pytest.raises(ValueError, match="nothing is pinned"):
            pool.pin_assign([0])
    finally:
        pool.close()


def test_one_reference_with_an_assignment_and_back_to_the_default():
    log = []
    pool = _pool(log, 2)
    try:
        pool.pin_graphs(np.zeros((1, 3, 3), np.float32))
        pool.energy_forces(_images(4))                                       # one reference: every image of any batch
        assert _seen(log) == [(k, 0) for k in range(4)]
        pool.pin_assign([0, 0, 0])
        with pytest.raises(ValueError, match="4 images"):
            pool.energy_forces(_images(4))
        pool.energy_forces(_images(3))
        pool.pin_assign(None)                                                # the engines' own default again: any number of images
        assert all(e.assign is None for e in pool.engines)
        del log[:]
        pool.energy_forces(_images(6))
        assert _seen(log) == [(k, 0) for k in range(6)]
    finally:
        pool.close()


def test_a_refusing_engine_leaves_the_pool_unpinned_and_the_with_block_unpins():
    log = []
    pool = _pool(log, 3, refuse_last=True)
    try:
        with pytest.raises(RuntimeError, match="refused"):
            pool.pin_graphs(np.zeros((2, 3, 3), np.float32))
        assert log == [("e0", "unpin"), ("e1", "unpin")] and pool.pinned_graphs() is None
        assert all(e.refs == 0 for e in pool.engines[:2])
    finally:
        pool.close()
    log = []
    pool = _pool(log, 2)
    try:
        with pytest.raises(KeyError):
            with pool.pinned_each(np.zeros((2, 3, 3), np.float32), assign=[1, 1, 0]):
                pool.energy_forces(_images(3))
                assert _seen(log) == [(0, 1), (1, 1), (2, 0)]
                raise KeyError("inside")
        assert log[-2:] == [("e0", "unpin"), ("e1", "unpin")] and all(e.refs == 0 for e in pool.engines)
        # an assignment that names a reference that is not there: nothing stays pinned
        with pytest.raises(ValueError, match=r"\[0, 2\)"):
            pool.pin_graphs(np.zeros((2, 3, 3), np.float32), assign=[0, 2])
        assert all(e.refs == 0 for e in pool.engines)
    finally:
        pool.close()


# ---- the ASE facade ------------------------------------------------------------------------------------------------------------------
class _Atoms:
    def __init__(self, z, pos, cell, pbc):
        self.numbers, self._pos, self.cell, self.pbc, self.info = z, np.asarray(pos, dtype=np.float64), cell, pbc, {}

    def get_positions(self):
        return self._pos


def test_the_facade_refuses_per_image_cells_and_mixed_cells_at_pin_time():
    A = importlib.import_module("pdb2reaction_amd.ase_calculator")
    calc = A.UMXCalculator(model="synthetic")
    z, refs, cell, pbc, _ = GC.reference_set("triclinic_capped")
    atoms = [_Atoms(z, p, cell, pbc) for p in refs]
    with pytest.raises(ValueError, match="per_image_cells"):
        calc.pinned_each(atoms, per_image_cells=True)
    atoms[1].cell = cell * 1.01
    with pytest.raises(ValueError, match="share the cell"):
        calc.pinned_each(atoms)
    with pytest.raises(ValueError, match="empty"):
        calc.pinned_each([])
    assert calc._engine is None                                              # refused before an engine was built
