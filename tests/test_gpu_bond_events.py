"""``umx_bond_events`` on the GPU: the events of many pairs of geometries are, bit for bit, the non-zero entries of the matrix kernels
(``umx_bond_changes`` / ``umx_bond_changes_cell``) in row-major order; against the independent checkers; at the seams of the scan and of
the triangle; under every capacity; beyond the matrix entries' n*n <= 2^31; the refusals; and the Python layers above the engine.

Geometries: ``synth.make_cluster`` / ``synth.make_product`` as tests/test_gpu_bond_changes.py (open space), atoms inside the cells of
tests/periodic_path_cases.py (periodic).  Lengths in Angstrom throughout (``unit_scale = 1``) except in the layer tests (Bohr, as pysisyphus).
The seeds were chosen on the CPU with the checkers so that every case of test 2 holds a formed and a broken pair; the test asserts it."""
import ctypes as C
import types

import numpy as np
import pytest

import periodic_path_cases as PC
from oracle import bond_changes_oracle as O
from pdb2reaction_amd import bond_changes as B
from pdb2reaction_amd import synth
from pdb2reaction_amd.engine import BOND_EVENT_DTYPE, BondEvent, Engine, UmxError

pytestmark = pytest.mark.gpu

PAIRS = [(0, 1), (1, 2), (0, 2), (2, 0)]
BOUNDARIES = ["open", "sheared", "slab"]
SENTINEL = 0xAB


@pytest.fixture(scope="module")
def light():
    e = Engine(0)                  # no weights, no system: the bond entries need neither
    yield e
    e.close()


def stack_of_three(n, boundary, seed=5):
    """(geoms (3, n, 3), cov (n,), cell, pbc): three geometries of the same n atoms, Angstrom."""
    if boundary == "open":
        z, pos = synth.make_cluster(max(n, 8), seed)
        g1 = synth.make_product(pos, seed + 1)
        g2 = synth.make_product(g1, seed + 2, sigma=4.0, amp=1.2)
        atoms = [synth.SYMBOLS[int(a)] for a in z][:n]
        geoms, cell, pbc = np.stack([pos, g1, g2])[:, :n], None, None
    else:
        cell, pbc = PC.CELLS[boundary]
        seed = 100 * n + seed + BOUNDARIES.index(boundary)
        rng = np.random.default_rng(seed)
        r0 = PC.atoms_in_cell(n, cell, seed)
        r1 = r0 + rng.uniform(-0.4, 0.4, r0.shape)
        r2 = r1 + rng.uniform(-0.4, 0.4, r0.shape)
        atoms = [str(a) for a in rng.choice(["C", "H", "O", "N"], size=n)]
        geoms = np.stack([r0, r1, r2])
    return np.ascontiguousarray(geoms), B.element_radii(atoms, 1.0)[1], cell, pbc


def kw_of(cell, pbc):
    return {} if cell is None else {"cell": cell, "pbc": pbc}


def events_of_matrices(p, d1, d2, code):
    """What the matrix entry's outputs hold as events of pair p: the non-zero codes in row-major order."""
    ij = np.argwhere(code != 0)
    ev = np.zeros(len(ij), dtype=BOND_EVENT_DTYPE)
    ev["pair"], ev["i"], ev["j"] = p, ij[:, 0], ij[:, 1]
    ev["code"], ev["d1"], ev["d2"] = code[ij[:, 0], ij[:, 1]], d1[ij[:, 0], ij[:, 1]], d2[ij[:, 0], ij[:, 1]]
    return ev


def matrix_route(light, geoms, cov, pairs, cell=None, pbc=None):
    """(events, counts) from one ``Engine.bond_changes`` call per pair -- the existing kernels."""
    per = [events_of_matrices(p, *light.bond_changes(geoms[a], geoms[b], cov, **kw_of(cell, pbc))) for p, (a, b) in enumerate(pairs)]
    return np.concatenate(per), np.array([len(e) for e in per], dtype=np.int64)


def raw(light, geoms, cov, pairs, capacity, cell=None, pbc=None, guard=4, n_atoms=None, n_geoms=None, n_pairs=None, only_a=False):
    """``umx_bond_events`` straight through ctypes on pre-filled outputs: (status, event bytes incl. the guard records behind the buffer,
    n_events, per_pair).  The buffer is ``capacity + guard`` records of SENTINEL bytes; n_events starts at -7, per_pair at -9."""
    g, c = np.ascontiguousarray(geoms, dtype=np.float64), np.ascontiguousarray(cov, dtype=np.float64)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    buf = np.full((capacity + guard) * 32, SENTINEL, dtype=np.uint8)
    total = C.c_int64(-7)
    ga = gb = None
    if pairs is not None:
        pr = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        ga_, gb_ = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        ga, gb = ga_.ctypes.data_as(ip), None if only_a else gb_.ctypes.data_as(ip)
    np_ = (len(pairs) if pairs is not None else g.shape[0] - 1) if n_pairs is None else n_pairs
    per = np.full(max(np_, 1), -9, dtype=np.int64)
    lat = None if cell is None else np.ascontiguousarray(cell, dtype=np.float64)
    flg = None if pbc is None else np.ascontiguousarray(pbc, dtype=np.intc)
    st = light.lib.umx_bond_events(light._h, c.shape[0] if n_atoms is None else n_atoms, g.shape[0] if n_geoms is None else n_geoms, g.ctypes.data_as(dp), np_,
                                   ga, gb, c.ctypes.data_as(dp), None if lat is None else lat.ctypes.data_as(dp),
                                   None if flg is None else flg.ctypes.data_as(C.POINTER(C.c_int)), 1.2, 0.05, 0.05, capacity,
                                   buf.ctypes.data_as(C.POINTER(BondEvent)) if capacity else None, C.byref(total), per.ctypes.data_as(C.POINTER(C.c_int64)))
    return st, buf, int(total.value), per


def same_events(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. events == the existing kernels, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("n", [2, 63, 64, 65, 130])
def test_events_are_the_nonzero_entries_of_the_matrix_kernels_bit_for_bit(light, n, boundary):
    geoms, cov, cell, pbc = stack_of_three(n, boundary)
    want, counts = matrix_route(light, geoms, cov, PAIRS, cell, pbc)
    got, per = light.bond_events(geoms, cov, PAIRS, per_pair=True, **kw_of(cell, pbc))
    print(f"[bond events {boundary} n={n}] per pair {per.tolist()}")
    assert np.array_equal(per, counts) and len(got) == counts.sum()
    for f in ("pair", "i", "j", "code"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["d1"].view(np.uint64), want["d1"].view(np.uint64)) and np.array_equal(got["d2"].view(np.uint64), want["d2"].view(np.uint64))
    assert same_events(got, want)
    # pair (2, 0) is pair (0, 2) read backwards: formed <-> broken, d1 <-> d2, the same bits
    fwd, back = got[got["pair"] == 2], got[got["pair"] == 3]
    assert np.array_equal(fwd["i"], back["i"]) and np.array_equal(fwd["j"], back["j"]) and np.array_equal(fwd["code"], 3 - back["code"])
    assert fwd["d1"].tobytes() == back["d2"].tobytes() and fwd["d2"].tobytes() == back["d1"].tobytes()
    if n >= 63:
        assert counts[:3].min() > 0                                           # no case passes empty


# ---- 2. against the independent checkers ----------------------------------------------------------------------------------------------
def checker_events(geoms, cov, pairs, cell, pbc):
    """The events by NumPy: oracle/bond_changes_oracle.compare (open) or brute-force minimum images + classify (cell)."""
    out = []
    dist = {} if cell is None else {g: PC.brute_distances(geoms[g], cell, pbc) for g in sorted({g for p in pairs for g in p})}
    for p, (a, b) in enumerate(pairs):
        if cell is None:
            d1, d2, code = O.compare(geoms[a], geoms[b], cov)
        else:
            d1, d2 = dist[a], dist[b]
            code, T = PC.classify(d1, d2, cov)
            assert PC.clear_of_thresholds(d1, d2, T)                          # the condition on the inputs: no pair at a threshold
        out.append(events_of_matrices(p, d1, d2, code))
    return out


@pytest.mark.parametrize("boundary, n", [("open", 64), ("open", 130), ("sheared", 65), ("sheared", 130), ("slab", 63), ("slab", 130)])
def test_events_against_the_independent_checkers(light, boundary, n):
    geoms, cov, cell, pbc = stack_of_three(n, boundary)
    pairs = PAIRS[:3]
    want = checker_events(geoms, cov, pairs, cell, pbc)
    for w in want:
        assert (w["code"] == 1).any() and (w["code"] == 2).any()                 # a formed and a broken pair in every pair of geometries
    got = light.bond_events(geoms, cov, pairs, **kw_of(cell, pbc))
    want = np.concatenate(want)
    print(f"[bond events vs checker {boundary} n={n}] {len(want)} events  max|dD1| = {np.abs(got['d1'] - want['d1']).max():.3e}  "
          f"max|dD2| = {np.abs(got['d2'] - want['d2']).max():.3e}")
    for f in ("pair", "i", "j", "code"):
        assert np.array_equal(got[f], want[f]), f
    np.testing.assert_allclose(got["d1"], want["d1"], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(got["d2"], want["d2"], rtol=1e-13, atol=1e-13)


# ---- 3. seams -------------------------------------------------------------------------------------------------------------------------
def plant(geoms, cov, i, j, where, close_in):
    """Atoms i and j alone at ``where``: 0.9 (c_i + c_j) apart (bonded) in the geometries ``close_in``, 3 (c_i + c_j) in the others."""
    s = cov[i] + cov[j]
    for g in range(len(geoms)):
        geoms[g, i] = where
        geoms[g, j] = np.asarray(where) + np.array([(0.9 if g in close_in else 3.0) * s, 0.0, 0.0])


def test_seams_of_the_scan_and_of_the_triangle(light):
    n = 130
    geoms, cov, _, _ = stack_of_three(n, "open")
    plant(geoms, cov, 0, 77, (60.0, 0.0, 0.0), {1})                            # an event in row 0 ...
    plant(geoms, cov, n - 2, n - 1, (-60.0, 5.0, 0.0), {1})                    # ... and one in the last possible cell (n - 2, n - 1)
    pairs = [(0, 1), (1, 2), (0, 2), (1, 1), (2, 0), (2, 1), (1, 0), (0, 1)]    # 8 x 130 = 1040 rows: past one 1024-row scan block;
    want, counts = matrix_route(light, geoms, cov, pairs)                      # (1, 1): identical geometries in the middle of the list
    got, per = light.bond_events(geoms, cov, pairs, per_pair=True)
    assert same_events(got, want) and np.array_equal(per, counts)
    assert counts[3] == 0 and counts[4] > 0
    keys = {(int(e["pair"]), int(e["i"]), int(e["j"])): int(e["code"]) for e in got}
    for p, code in ((0, 1), (1, 2), (5, 1), (6, 2), (7, 1)):
        assert keys[(p, 0, 77)] == code and keys[(p, n - 2, n - 1)] == code
    assert 7 * n + (n - 2) >= 1024                                            # the last event's row lies in the second scan block
    # consecutive pairs by default: NULL, NULL
    got01 = light.bond_events(geoms, cov)
    assert same_events(got01, got[got["pair"] <= 1])


def test_two_atoms_with_and_without_an_event(light):
    cov = B.element_radii(["C", "O"], 1.0)[1]
    s = cov.sum()
    geoms = np.zeros((2, 2, 3))
    geoms[0, 1, 0], geoms[1, 1, 0] = 3.0 * s, 0.9 * s
    got, per = light.bond_events(geoms, cov, [(0, 1), (0, 0), (1, 0)], per_pair=True)
    assert per.tolist() == [1, 0, 1]
    assert got.tolist() == [(0, 0, 1, 1, 3.0 * s, 0.9 * s), (2, 0, 1, 2, 0.9 * s, 3.0 * s)]


# ---- 4. capacity ----------------------------------------------------------------------------------------------------------------------
def test_every_capacity_writes_the_prefix_and_reports_the_total(light):
    geoms, cov, _, _ = stack_of_three(65, "open")
    full = light.bond_events(geoms, cov, PAIRS)
    T = len(full)
    assert T >= 3
    for cap in (0, 1, T - 1, T, T + 5):
        st, buf, total, per = raw(light, geoms, cov, PAIRS, cap)
        m = min(cap, T)
        assert st == 0 and total == T and per[:4].sum() == T, cap
        assert buf[:m * 32].tobytes() == full[:m].tobytes(), cap
        assert (buf[m * 32:] == SENTINEL).all(), cap                            # the rest of the buffer and the guard behind it
    # the wrapper repeats the call once when its buffer was too small
    assert same_events(light.bond_events(geoms, cov, PAIRS, capacity=1), full) and len(light.bond_events(geoms, cov, PAIRS, capacity=0)) == T


# ---- 5. order and repeatability -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", ["open", "sheared"])
def test_order_is_strict_and_two_calls_give_the_same_bytes(light, boundary):
    geoms, cov, cell, pbc = stack_of_three(130, boundary)
    a = light.bond_events(geoms, cov, PAIRS, **kw_of(cell, pbc))
    b = light.bond_events(geoms, cov, PAIRS, **kw_of(cell, pbc))
    assert len(a) and a.tobytes() == b.tobytes()
    n = 130
    key = (a["pair"].astype(np.int64) * n + a["i"]) * n + a["j"]
    assert (np.diff(key) > 0).all() and (a["i"] < a["j"]).all() and np.isin(a["code"], (1, 2)).all()


# ---- 6. beyond n * n <= 2^31 ----------------------------------------------------------------------------------------------------------
def test_fifty_thousand_atoms_beyond_the_matrix_limit(light):
    n, a = 50000, 3.0
    g = np.arange(37, dtype=np.float64) * a
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[:n]
    cov = B.element_radii(["H"] * n, 1.0)[1]                                   # T = 0.744 A: nothing on the 3 A lattice is bonded
    planted = [(0, 49999), (1, 2), (63, 64), (65, 129), (777, 30000), (12345, 40000), (25000, 25001), (49997, 49998)]
    back = [(63, 64), (12345, 40000)]
    geoms = np.stack([lattice, lattice, lattice])
    for i, j in planted:
        geoms[1, j] = geoms[1, i] + np.array([0.36, 0.48, 0.0])                # 0.6 A from its partner
        if (i, j) not in back:
            geoms[2, j] = geoms[1, j]
    got, per = light.bond_events(geoms, cov, per_pair=True)                    # consecutive: (0, 1), (1, 2)
    assert per.tolist() == [len(planted), len(back)]
    assert [(int(e["pair"]), int(e["i"]), int(e["j"]), int(e["code"])) for e in got] == [(0, i, j, 1) for i, j in sorted(planted)] + [(1, i, j, 2) for i, j in sorted(back)]
    for e in got:
        ga, gb = (geoms[0], geoms[1]) if e["pair"] == 0 else (geoms[1], geoms[2])
        want = [np.sqrt(((x[e["i"]] - x[e["j"]]) ** 2).sum()) for x in (ga, gb)]
        np.testing.assert_allclose([e["d1"], e["d2"]], want, rtol=1e-13, atol=1e-13)
    with pytest.raises(UmxError, match=r"n\*n exceeds 2\^31 pairs"):            # the matrix entry keeps its limit
        light.bond_changes(geoms[0], geoms[1], cov, distances=False)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_offender_and_leave_the_outputs_untouched(light):
    geoms, cov, _, _ = stack_of_three(5, "open")
    cell, pbc = PC.CELLS["ortho"]
    nan_geom = geoms.copy()
    nan_geom[2, 3, 1] = np.nan
    inf_cov = cov.copy()
    inf_cov[4] = np.inf
    nan_cell = cell.copy()
    nan_cell[1, 2] = np.nan
    flat = np.array([[5.0, 0, 0], [10.0, 0, 0], [0, 0, 8.0]])
    cases = [(dict(n_atoms=0), "n_atoms = 0"), (dict(n_geoms=0), "n_geoms = 0"), (dict(n_pairs=0), "n_pairs = 0"), (dict(n_pairs=-2), "n_pairs = -2"),
             (dict(only_a=True), "only one of geom_a / geom_b"),
             (dict(pairs=[(0, 1), (1, 3)]), "pair 1 names geometry 3"), (dict(pairs=[(-1, 1)]), "pair 0 names geometry -1"),
             (dict(geoms=nan_geom), "non-finite coordinate in geometry 2"), (dict(cov=inf_cov), "non-finite radius of atom 4"),
             (dict(cell=flat, pbc=(1, 1, 1)), "degenerate cell: the periodic lattice vectors span no volume"),
             (dict(cell=nan_cell, pbc=(1, 1, 1)), "non-finite cell entry"),
             (dict(cell=np.array([[5.0, 0, 0], [9.5, 1.0, 0], [0, 0, 8.0]]), pbc=(1, 1, 1)), "more than the 4 lattice translations")]
    for kw, why in cases:
        args = {"geoms": geoms, "cov": cov, "pairs": PAIRS, "capacity": 8, **kw}
        st, buf, total, per = raw(light, **args)
        msg = light.lib.umx_last_error(light._h).decode()
        assert st == -1 and msg.startswith("umx_bond_events: ") and why in msg, (why, msg)
        assert (buf == SENTINEL).all() and total == -7 and (per == -9).all(), why
    # a single geometry has no consecutive pair; an open axis makes the flat cell harmless
    st, buf, total, per = raw(light, geoms[:1], cov, None, 8)
    assert st == -1 and "consecutive pairs need at least two geometries" in light.lib.umx_last_error(light._h).decode() and total == -7
    assert raw(light, geoms, cov, PAIRS, 8, cell=flat, pbc=(1, 0, 1))[0] == 0
    with pytest.raises(UmxError, match="pair 0 names geometry 7"):
        light.bond_events(geoms, cov, [(7, 0)])


# ---- 8. the layers above the engine ---------------------------------------------------------------------------------------------------
def _bohr_geoms(n, k, seed=5):
    """k images of a straight interpolation cluster -> product, as pysisyphus-like geometries in Bohr."""
    from pdb2reaction_amd.uma_pysis import ANG2BOHR

    z, pos = synth.make_cluster(n, seed)
    prod = synth.make_product(pos, seed + 1)
    atoms = [synth.SYMBOLS[int(a)] for a in z]
    return [types.SimpleNamespace(atoms=atoms, coords3d=(pos + (prod - pos) * t) * ANG2BOHR) for t in np.linspace(0.0, 1.0, k)]


def test_compare_structures_without_matrices_and_compare_path(light):
    geoms = _bohr_geoms(65, 5)
    full = B.compare_structures(geoms[0], geoms[-1], engine=light)
    lean = B.compare_structures(geoms[0], geoms[-1], engine=light, matrices=False)
    assert full.formed_covalent and full.broken_covalent
    assert lean.formed_covalent == full.formed_covalent and lean.broken_covalent == full.broken_covalent
    assert lean.distances_1 is None and lean.distances_2 is None and full.lengths is None
    assert all(lean.lengths[p] == (full.distances_1[p], full.distances_2[p]) for p in lean.lengths)
    assert B.summarize_changes(geoms[-1], lean) == B.summarize_changes(geoms[-1], full)
    path = B.compare_path(geoms, "consecutive", engine=light)
    assert len(path) == 4
    for k, r in enumerate(path):
        one = B.compare_structures(geoms[k], geoms[k + 1], engine=light)
        assert r.formed_covalent == one.formed_covalent and r.broken_covalent == one.broken_covalent
        assert B.summarize_changes(geoms[k + 1], r) == B.summarize_changes(geoms[k + 1], one)
    assert any(r.formed_covalent or r.broken_covalent for r in path)
    # in a cell: the minimum-image entry
    cell, pbc = PC.CELLS["sheared"]
    r0 = PC.atoms_in_cell(65, cell, 3)
    r1 = r0 + np.random.default_rng(4).uniform(-0.4, 0.4, r0.shape)
    atoms = [str(a) for a in np.random.default_rng(5).choice(["C", "H", "O", "N"], size=65)]
    g0, g1 = types.SimpleNamespace(atoms=atoms, coords3d=r0), types.SimpleNamespace(atoms=atoms, coords3d=r1)
    kw = dict(engine=light, unit_scale=1.0, cell=cell, pbc=pbc)
    full, lean = B.compare_structures(g0, g1, **kw), B.compare_structures(g0, g1, matrices=False, **kw)
    assert full.formed_covalent | full.broken_covalent and lean.formed_covalent == full.formed_covalent and lean.broken_covalent == full.broken_covalent
    assert B.summarize_changes(g1, lean) == B.summarize_changes(g1, full)


def test_optimize_path_gsm_reports_the_bond_changes_of_its_final_images(light):
    from pdb2reaction_amd.path_opt import optimize_path_gsm
    from pdb2reaction_amd.uma_pysis import ANG2BOHR

    z, imgs, _ = synth.make_images(14, 4, seed=21)                              # the system of tests/test_gpu_calculator.py
    elem = [synth.SYMBOLS[int(v)] for v in z]
    cov = B.element_radii(elem, 1.0)[1]
    # that system's endpoints differ in no bond: in the product H4 (atom 3) is drawn onto N11 (atom 10), its nearest non-bonded partner
    prod = imgs[3].copy()
    u = prod[10] - prod[3]
    prod[10] = prod[3] + 0.9 * (cov[3] + cov[10]) * u / np.linalg.norm(u)
    kw = dict(calc_kw={"model": "synthetic"}, max_nodes=4, max_cycles=3, gs_kw={"perp_thresh": 1e3, "climb": False}, stopt_kw={"max_step": 0.05}, align=False,
              fix_ends=True)
    plain = optimize_path_gsm(elem, imgs[0], prod, **kw)
    res = optimize_path_gsm(elem, imgs[0], prod, bond_changes=True, bond_engine=light, **kw)
    assert "bond_changes" not in plain and set(res) == set(plain) | {"bond_changes"}
    blk, k = res["bond_changes"], len(res["images_ang"])
    geoms = [types.SimpleNamespace(atoms=elem, coords3d=x * ANG2BOHR) for x in res["images_ang"]]
    ends = B.compare_structures(geoms[0], geoms[-1], engine=light)
    assert ends.formed_covalent == {(3, 10)} and not ends.broken_covalent       # the ends are fixed, so this is the planted change
    assert blk["endpoints"] == B.summarize_changes(geoms[-1], ends) and blk["endpoints"].startswith("Bond formed (1):\n  - H4-N11 : 1.407 Å --> 0.918 Å")
    assert [s["images"] for s in blk["segments"]] == [[a, a + 1] for a in range(k - 1)] and k == 6
    # every segment is the comparison of its two images, and each of its pairs changes its bonded state (D <= 1.14 (c_i + c_j), by NumPy)
    # between them in the direction it is reported in
    x = np.asarray(res["images_ang"])
    bonded = np.sqrt(((x[:, :, None, :] - x[:, None, :, :]) ** 2).sum(-1)) <= (1.2 - 0.05 * 1.2) * (cov[:, None] + cov[None, :])
    formed, broken, net = set(), set(), np.zeros((len(z), len(z)), dtype=int)
    for s in blk["segments"]:
        a, b = s["images"]
        one = B.compare_structures(geoms[a], geoms[b], engine=light)
        assert s["formed"] == [list(p) for p in sorted(one.formed_covalent)] and s["broken"] == [list(p) for p in sorted(one.broken_covalent)]
        assert all(not bonded[a][i, j] and bonded[b][i, j] for i, j in s["formed"]) and all(bonded[a][i, j] and not bonded[b][i, j] for i, j in s["broken"])
        formed |= one.formed_covalent
        broken |= one.broken_covalent
        for sign, pairs in ((1, s["formed"]), (-1, s["broken"])):
            for i, j in pairs:
                net[i, j] += sign
    print(f"[path bond changes] endpoints: {blk['endpoints']!r}; formed in some segment: {sorted(formed)}; broken in some segment: {sorted(broken)}")
    # The segments against the endpoint result.  A change of state is in no segment only when the length moves by less than
    # delta_fraction * T = 0.061 A within it; where every change of state of a pair is reported, formed minus broken over the segments is
    # its change of state between the ends.
    flips = np.abs(np.diff(bonded.astype(int), axis=0)).sum(0)
    for i, j in formed | broken:
        if flips[i, j] == sum([i, j] in s["formed"] or [i, j] in s["broken"] for s in blk["segments"]):
            assert net[i, j] == int(bonded[-1][i, j]) - int(bonded[0][i, j])
    # Here: H4-N11 closes from 1.407 A to 0.918 A over five segments between fixed ends -- on the straight path 0.19 and 0.16 A in the
    # first two, crossing 1.163 A in the second, 0.056 A and 0.103 A away from its two images -- so it is formed in some segment; no other
    # pair comes within 0.1 A of its threshold before the last image, so nothing else forms and nothing breaks.
    assert formed == ends.formed_covalent == {(3, 10)} and broken == ends.broken_covalent == set()
