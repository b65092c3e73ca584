"""The checker of tests/test_gpu_graph_links.py on the CPU (no GPU): every case of tests/graph_cases.py meets the input conditions it was
built for (the tie at the cap, the pair at exactly the cutoff, the candidate count above 1024 ...), so a later edit of a geometry cannot
quietly lose them; captures synthesised from the reference -- the edge vectors from a numpy float32 restatement of the formula -- pass the
checker; and five mutations of such captures are rejected, each for its own reason."""
import functools

import numpy as np
import pytest

import graph_cases as G
from periodic_oracle import lattice_translations


@functools.lru_cache(maxsize=None)
def _open(name):
    z, pos, radius, max_neigh = G.open_case(name)
    return pos, radius, max_neigh, G.candidates_open(pos, radius), G.reference_open(pos, radius, max_neigh)


@functools.lru_cache(maxsize=None)
def _cell(name, max_neigh):
    z, pos, cell, pbc, radius = G.cell_case(name)
    d2c, shifts = G.candidates_cell(pos, cell, pbc, radius)
    return pos, cell, pbc, radius, d2c, shifts, G.reference_cell(pos, cell, pbc, radius, max_neigh)


def _degrees(ref, nn):
    return np.bincount(ref["dst"], minlength=nn), np.bincount(ref["src"], minlength=nn)


# ---- 1. the input conditions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.OPEN))
def test_open_cases_meet_their_conditions(name):
    pos, radius, max_neigh, d2c, ref = _open(name)
    exp = G.OPEN_EXPECT[name]
    f = G.cap_facts(d2c, radius, max_neigh)
    indeg, outdeg = _degrees(ref, len(pos))
    assert G.is_dyadic(pos) and ref["exact"]
    assert len(ref["src"]) == exp["edges"] and f["trunc_rows"] == exp["trunc_rows"]
    for key in ("tie_rows", "at_cutoff", "rows_at_cap"):
        if key in exp:
            assert f[key] == exp[key], (key, f[key])
    if "cand" in exp:
        assert (int(f["cand"].min()), int(f["cand"].max())) == exp["cand"]
    if "outdeg" in exp:
        assert (int(outdeg.min()), int(outdeg.max())) == exp["outdeg"]
    if name in ("G10", "G26", "G53", "G124", "Gfree"):
        # edges AT the cutoff survive into the graph where the cap leaves room for them (G53: the three of each corner row)
        d2 = (ref["vec"] ** 2).sum(1)
        assert (d2 == radius * radius).sum() == {"G10": 0, "G26": 0, "G53": 24, "G124": 150, "Gfree": 150}[name]
    if name == "G53":          # the 8 corner rows have exactly max_neigh candidates, every other row truncates
        corners = np.nonzero(f["cand"] == 53)[0]
        assert sorted(corners.tolist()) == sorted(int(a * 25 + b * 5 + c) for a in (0, 4) for b in (0, 4) for c in (0, 4))
    if name == "G124":         # the largest candidate count IS the cap: the host sees maxdeg >= max_neigh, no row truncates
        assert int(f["cand"].max()) == max_neigh == int(indeg.max())
    if name == "Gfree":        # 64 < out-degree <= 320 occurs (the five-register rank sort), and so does <= 64
        assert (outdeg > 64).any() and (outdeg <= 64).any()
    if name == "S1236":        # both truncating forms in one launch; k_scan with 3 nodes per thread
        assert int((f["cand"] > 1024).sum()) == exp["cand_over_1024"] and int(f["cand"].max()) == exp["cand_max"]
        assert int((f["cand"] <= 1024).sum()) == 2050 and len(pos) == 2197 and -(-len(pos) // 1024) == 3 and (indeg == 12).all()
    if name == "D400":         # both branches of the out-edge sort, in-degree at the cap
        assert (outdeg > 320).any() and ((outdeg > 64) & (outdeg <= 320)).any() and int(indeg.max()) == exp["indeg_max"]


@pytest.mark.parametrize("name", list(G.CELLS))
def test_cell_cases_meet_their_conditions(name):
    exp = G.CELL_EXPECT[name]
    pos, cell, pbc, radius, d2c, shifts, ref = _cell(name, 20)
    ints, _ = lattice_translations(cell, pbc, radius)
    assert shifts == len(ints) == exp["shifts"]
    assert G.is_dyadic(pos, cell) and ref["exact"]
    frac = pos @ np.linalg.inv(cell)
    assert ((frac > 0) & (frac < 1)).all()                                       # strictly inside the cell: the wrap is the identity
    inv = np.linalg.inv(cell)
    assert np.array_equal(inv * 16, np.round(inv * 16))                          # dyadic dual vectors: float32 and float64 wrap alike
    f = G.cap_facts(d2c, radius, 20)
    assert (f["cand"] == exp["cand"]).all()
    indeg, outdeg = _degrees(ref, len(pos))
    if name != "Cap":
        assert f["at_cutoff"] == exp["at_cutoff"] and f["tie_rows"] == len(pos) == f["trunc_rows"]
        assert (indeg == 20).all()
        free = G.cap_facts(d2c, radius, None)
        assert free["trunc_rows"] == 0
    if name == "Sh":           # a cap makes the graph asymmetric
        assert (int(outdeg.min()), int(outdeg.max())) == exp["outdeg20"]
    if name == "One":          # every edge is a self image; the table is full
        assert len(pos) == 1 and (ref["src"] == ref["dst"]).all() and shifts == 729
    if name == "Cap":          # more candidates than the truncating fill ranks: refused while the cap binds, accepted when it does not
        assert exp["cand"] > 1024 and G.cap_facts(d2c, radius, 50)["trunc_rows"] == 64 and G.cap_facts(d2c, radius, 2000)["trunc_rows"] == 0
        full = _cell(name, 2000)[-1]
        ind, outd = _degrees(full, 64)
        assert len(full["src"]) == 64 * 1188 and (ind == 1188).all() and (outd == 1188).all()


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_seam_cases_are_clear_of_their_thresholds(n):
    z, pos = G.seam_case(n)
    assert len(z) == n
    for cap in (8, None):
        f = G.random_facts(pos[None], 6.0, cap)
        assert f["cutoff_gap"] > G.CLEAR and f["cap_gap"] > G.CLEAR
        assert (f["trunc_rows"] > 0) == (cap == 8)


@pytest.mark.parametrize("n,k", [(205, 5), (129, 9)])
def test_batch_cases_are_clear_of_their_thresholds(n, k):
    z, imgs = G.batch_case(n, k)
    assert imgs.shape == (k, n, 3) and k * n > 1024 and (k * n) % -(-(k * n) // 1024) != 0      # past one node per thread, a ragged last chunk
    f = G.random_facts(imgs, 6.0, 20)
    assert f["cutoff_gap"] > G.CLEAR and f["cap_gap"] > G.CLEAR and f["trunc_rows"] > 0


# ---- 2. the checker passes on captures synthesised from the reference --------------------------------------------------------------------
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("name", list(G.OPEN))
def test_checker_accepts_open_lattices(name, double):
    pos, radius, max_neigh, _, ref = _open(name)
    p = pos if double else pos.astype(np.float32)
    cap = G.captures_of(ref, p, len(pos))
    indeg, _ = _degrees(ref, len(pos))
    G.check_graph(cap, ref, len(pos), stats=(len(ref["src"]), int(indeg.max())))


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("max_neigh", [20, None])
@pytest.mark.parametrize("name", ["C4", "Sh", "One", "Slab"])
def test_checker_accepts_cells(name, max_neigh, double):
    z, pos, cell, pbc, radius = G.cell_case(name)
    both = np.stack([pos, pos])                                                   # two images of the same cell
    ref = G.reference_cell(both, cell, pbc, radius, max_neigh, double_positions=double)
    cap = G.captures_of(ref, both if double else both.astype(np.float32), 2 * len(pos))
    G.check_graph(cap, ref, 2 * len(pos))
    assert (ref["absd"] is None) == double


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("n", [63, 129])
def test_checker_accepts_random_clusters(n, double):
    z, pos = G.seam_case(n)
    for cap_ in (8, None):
        ref = G.reference_open(pos, 6.0, cap_, double_positions=double)
        assert not ref["exact"]
        rd, rn = G.check_graph(G.captures_of(ref, pos if double else pos.astype(np.float32), n), ref, n)
        assert 0 < rd <= 1 and 0 < rn <= 1


def test_checker_accepts_a_batch_and_a_partition():
    z, imgs = G.batch_case(129, 9)
    ref = G.reference_open(imgs, 6.0, 20)
    assert ref["dst"].max() == 9 * 129 - 1 and (np.diff(ref["dst"]) >= 0).all()
    G.check_graph(G.captures_of(ref, imgs.astype(np.float32), 9 * 129), ref, 9 * 129)
    pos, radius, max_neigh, _, full = _open("G10")
    n = len(pos)
    part = G.restrict(full, n * 2 // 3, n)
    assert 0 < len(part["src"]) < len(full["src"]) and part["dst"].min() == n * 2 // 3
    cap = G.captures_of(part, pos.astype(np.float32), n)
    assert (np.diff(cap["row_ptr"])[: n * 2 // 3] == 0).all()
    G.check_graph(cap, part, n, stats=(1250, 10), expect_stats=(1250, 10))
    with pytest.raises(G.GraphMismatch, match="edge list"):
        G.check_graph(cap, full, n)


# ---- 3. mutations the checker must reject -------------------------------------------------------------------------------------------------
def test_rejects_a_tie_broken_towards_the_higher_source():
    pos, radius, max_neigh, d2c, ref = _open("G10")
    wrong = G.break_tie_upwards(ref, pos, d2c, max_neigh)
    assert len(wrong["src"]) == len(ref["src"]) and (wrong["src"] != ref["src"]).sum() >= 1
    G.check_graph(G.captures_of(wrong, pos.astype(np.float32), len(pos)), wrong, len(pos))        # self-consistent, just another graph
    with pytest.raises(G.GraphMismatch, match="edge list"):
        G.check_graph(G.captures_of(wrong, pos.astype(np.float32), len(pos)), ref, len(pos))


def test_rejects_a_tie_broken_towards_the_higher_translation():
    pos, cell, pbc, radius, d2c, shifts, ref = _cell("One", 20)
    ints, _ = lattice_translations(cell, pbc, radius)
    wrong = G.break_tie_upwards(ref, pos, d2c, 20, tv=ints.astype(np.float64) @ cell)
    # one atom: every source is atom 0, so the two graphs differ in a translation only -- the integer arrays cannot see it
    assert np.array_equal(wrong["src"], ref["src"]) and not np.array_equal(wrong["tidx"], ref["tidx"])
    with pytest.raises(G.GraphMismatch, match="evec"):
        G.check_graph(G.captures_of(wrong, pos.astype(np.float32), 1), ref, 1)
    pos, cell, pbc, radius, d2c, shifts, ref = _cell("C4", 20)
    ints, _ = lattice_translations(cell, pbc, radius)
    wrong = G.break_tie_upwards(ref, pos, d2c, 20, tv=ints.astype(np.float64) @ cell)
    with pytest.raises(G.GraphMismatch, match="edge list|evec"):
        G.check_graph(G.captures_of(wrong, pos.astype(np.float32), len(pos)), ref, len(pos))


@pytest.mark.parametrize("case", ["Gfree", "C4"])
def test_rejects_a_dropped_edge_at_the_cutoff(case):
    if case == "Gfree":
        pos, radius, _, _, ref = _open(case)
    else:
        pos, _, _, radius, _, _, ref = _cell(case, None)
    at = np.nonzero((ref["vec"] ** 2).sum(1) == radius * radius)[0]
    assert len(at)
    wrong = G.drop_edge(ref, int(at[len(at) // 2]))
    with pytest.raises(G.GraphMismatch, match="edge list"):
        G.check_graph(G.captures_of(wrong, pos.astype(np.float32), len(pos)), ref, len(pos))


@pytest.mark.parametrize("case", ["Gfree", "D400"])
def test_rejects_two_swapped_out_edges(case):
    pos, radius, max_neigh, _, ref = _open(case)
    cap = G.captures_of(ref, pos.astype(np.float32), len(pos))
    row = int(np.argmax(np.diff(cap["out_ptr"])))                                # the longest list; swap its last two entries
    b = int(cap["out_ptr"][row + 1])
    assert b - int(cap["out_ptr"][row]) > (320 if case == "D400" else 64)
    cap["out_edge"][[b - 2, b - 1]] = cap["out_edge"][[b - 1, b - 2]]
    with pytest.raises(G.GraphMismatch, match=f"out_edge.*source {row}"):
        G.check_graph(cap, ref, len(pos))


def test_rejects_a_row_ptr_shifted_behind_node_1024():
    pos, radius, max_neigh, _, ref = _open("S1236")
    cap = G.captures_of(ref, pos.astype(np.float32), len(pos))
    cap["row_ptr"][1024:] += 1
    with pytest.raises(G.GraphMismatch, match="row_ptr.*node 1024"):
        G.check_graph(cap, ref, len(pos))


@pytest.mark.parametrize("case", ["G10", "seam"])
def test_rejects_a_distance_off_by_8_ulp(case):
    if case == "G10":
        pos, radius, max_neigh, _, ref = _open(case)
    else:
        z, pos = G.seam_case(65)
        ref = G.reference_open(pos, 6.0, 8)
    cap = G.captures_of(ref, pos.astype(np.float32), len(pos))
    G.check_graph(cap, ref, len(pos))
    e = len(ref["src"]) // 2
    d = cap["evec"][e, 3]
    for _ in range(8):
        d = np.nextafter(d, np.float32(np.inf))
    cap["evec"][e, 3] = d
    with pytest.raises(G.GraphMismatch, match=f"evec distance: edge {e} "):
        G.check_graph(cap, ref, len(pos))
