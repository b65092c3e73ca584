"""The neighbour-graph kernels (K1), link by link, against the float64 graph -- at ties, caps and seams.

Every other link file takes the graph from the engine's captures as given.  Here the captured graph itself (row_ptr, src, dst, out_ptr,
out_edge, evec) is compared with the oracle's: ``oracle.escn_md_oracle.radius_graph`` for open boundaries,
``periodic_oracle.periodic_radius_graph`` for cells, on the float64 values of the positions the engine was given.  The integer arrays must
be EQUAL; evec holds per element (bounds derived in tests/graph_cases.py: K_D = 4, K_N = 7 u, the periodic float path with its absolute
term; on the dyadic lattices d is bit-equal to float32(sqrt(d^2))).  The energy must be finite; E and F are the parity files' business.
tests/test_graph_links_cpu.py asserts the input conditions of every case from the oracle and holds the checker itself.

    kernel          branch                                                       cases
    k_graph_count   open, float | double                                         every open case | G10, Gfree, seams (double)
                    periodic one cell | per-image cells, float | double          C4, Sh, One, Slab (all four combinations)
                    cand > max_neigh && cand > GF_MAXC -> flag bit 2             Cap at max_neigh 50 (refused), 2000 (accepted)
                    d2 == rc2 kept                                               G*, C4, Sh, One, Slab (pairs at exactly the cutoff)
                    rows outside [lo, hi) zeroed                                 parts
    k_scan          n <= 1024 (one node per thread)                              G*, D400, seams, cells
                    n > 1024: chunk 2 with a ragged end | chunk 3                batch (1025, 1161 nodes) | S1236 (2197)
                    zeros carried over unowned rows                              parts
    k_graph_fill    TRUNC = false                                                Gfree, seams at the default cap, cells at the default cap
                    TRUNC, no row truncates (maxdeg == max_neigh)                G124
                    TRUNC, LDS rank, ties across the cap                         G10, G26, D400 (in-degree 400), S1236 (2050 rows)
                    TRUNC, rows with cand == max_neigh next to truncating ones   G53
                    TRUNC, slow form (cand > GF_MAXC), its own tie rule          S1236 (147 rows, 1025 .. 1236 candidates)
                    ballot compaction across wave seams                          seams (63, 64, 65, 129 atoms), batch (base = image offset)
                    PBC truncating: key (d2, translation index * N + source)     C4, Sh, One (self images only, 729 table entries), Slab
                    PBC not truncating, > GF_MAXC candidates                     Cap at max_neigh 2000
                    PBC pruning (pbc_active_shifts) with an image AT the cutoff  C4, Sh, One, Slab
                    owned rows [lo, hi) only                                     parts
    k_out_count / k_out_fill / k_out_sort
                    d <= 64 | 64 < d <= 320 | d > 320 (insertion sort)           G10 | Gfree, G124, D400 | D400 (.. 511), Cap (1188)
                    empty rows                                                   parts; asymmetric lists: G10 (3 .. 20), Sh (19 .. 21)
    k_wrap_cell     identity on atoms strictly inside the cell                   every cell case

Measured on the MI355X (53 cases, 10 s in all, the largest evaluation -- D400, 203864 edges -- well under a second; energies only: the
graph is built alike with and without forces, and the force assembly is the edge-link file's): every integer array equal in every case; max
|err| / bound of (d, n): dyadic lattices 0.19 / 0.16 .. 0.29 (d is the correctly rounded root of an exact d^2: its error is the root's one
rounding), random clusters and batches 0.42 .. 0.61 / 0.35 .. 0.51, cells 0.05 .. 0.15 / 0.03 .. 0.09 (their bound carries the absolute
term), Cap at max_neigh 2000 0.13 / 0.10; the batches of 1025 and 1161 nodes ran as one chunk.  No kernel finding.  One host finding, fixed
with this file: with captures on, UMX_FORCE_PARTS came back as UMX_ERR_CAPACITY with an empty text (NOTES.md section 12, item 17).
"""
import numpy as np
import pytest

import graph_cases as G
from periodic_oracle import lattice_translations

pytestmark = pytest.mark.gpu

UMX_ERR_CAPACITY = -4          # include/umx.h


@pytest.fixture(scope="module")
def geng(weights):
    """one engine for the cases that need no fresh one; it leaves no cell and no captures behind"""
    from pdb2reaction_amd.engine import Engine

    e = Engine(0)
    e.load_weights(weights)
    yield e
    e.close()


def capture(eng, z, pos, radius, max_neigh, monkeypatch, double=False, cell=None, cells=None, pbc=None, forces=False):
    """one evaluation with the graph captures kept: (captures, graph_stats, last_graph_shifts, energies)"""
    monkeypatch.setenv("UMX_DEBUG_ONLY", G.NAMES)
    eng.set_system(z, radius=radius, max_neigh=max_neigh)
    if cells is not None:
        eng.set_cells(cells, pbc)
    else:
        eng.set_cell(cell, pbc)
    eng.debug_keep(True)
    try:
        e, _ = eng.energy_forces(pos, forces=forces, double_positions=double)     # (the graph is built alike with and without forces)
        cap = {n: eng.debug_fetch(n, np.int32) for n in ("row_ptr", "src", "dst", "out_ptr", "out_edge")}
        cap["evec"] = eng.debug_fetch("evec").reshape(-1, 4)
        return cap, eng.graph_stats(), eng.last_graph_shifts(), e
    finally:
        eng.debug_keep(False)
        eng.set_cell(None)


def held(tag, cap, ref, nn, stats, e, expect_stats=None):
    rd, rn = G.check_graph(cap, ref, nn, stats=stats, expect_stats=expect_stats)
    print(f"  [{tag}] {len(ref['src'])} edges, stats {stats}: max |err| / bound  d {rd:.3f}  n {rn:.3f}")
    assert np.isfinite(e).all(), e


# ---- open boundaries ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,double", [(n, False) for n in G.OPEN] + [("G10", True), ("Gfree", True)])
def test_open_lattices(geng, name, double, monkeypatch):
    """the double entry on G10 and Gfree (the float64 values are the same: the graph must be identical)"""
    z, pos, radius, max_neigh = G.open_case(name)
    ref = G.reference_open(pos, radius, max_neigh, double_positions=double)
    exp = G.OPEN_EXPECT[name]
    assert len(ref["src"]) == exp["edges"] and ref["exact"]
    cap, stats, shifts, e = capture(geng, z, pos, radius, max_neigh, monkeypatch, double=double)
    assert shifts == 0
    held(f"{name}{' f64' if double else ''}", cap, ref, len(z), stats, e)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("max_neigh", [8, None])
@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_wave_seams(geng, n, max_neigh, double, monkeypatch):
    z, pos = G.seam_case(n)
    f = G.random_facts(pos[None], 6.0, max_neigh)
    assert f["cutoff_gap"] > G.CLEAR and f["cap_gap"] > G.CLEAR
    ref = G.reference_open(pos, 6.0, max_neigh, double_positions=double)
    cap, stats, _, e = capture(geng, z, pos, 6.0, max_neigh, monkeypatch, double=double)
    held(f"seam {n} / {max_neigh}{' f64' if double else ''}", cap, ref, n, stats, e)


@pytest.mark.parametrize("n,k", [(205, 5), (129, 9)])
def test_batches_past_the_scan_seam(weights, n, k, monkeypatch):
    from pdb2reaction_amd.engine import Engine

    z, imgs = G.batch_case(n, k)
    f = G.random_facts(imgs, 6.0, 20)
    assert f["cutoff_gap"] > G.CLEAR and f["cap_gap"] > G.CLEAR and f["trunc_rows"] > 0
    ref = G.reference_open(imgs, 6.0, 20)
    monkeypatch.setenv("UMX_STREAMS", "1")
    eng = Engine(0)
    try:
        eng.load_weights(weights)
        cap, stats, _, e = capture(eng, z, imgs, 6.0, 20, monkeypatch)
    finally:
        eng.close()
    if len(cap["row_ptr"]) != k * n + 1:
        pytest.skip(f"the batch ran in several chunks: the captured row_ptr has {len(cap['row_ptr'])} entries, one chunk has {k * n + 1}")
    held(f"batch {k} x {n}", cap, ref, k * n, stats, e)


def test_partitions_own_their_target_range(weights, monkeypatch):
    """UMX_FORCE_PARTS=3: the captures are the last partition's -- the reference rows of its targets, empty rows elsewhere, out-lists
    built from those edges; the counts the host reports are the whole image's"""
    from pdb2reaction_amd.engine import Engine

    z, pos, radius, max_neigh = G.open_case("G10")
    n = len(z)
    full = G.reference_open(pos, radius, max_neigh)
    part = G.restrict(full, n * 2 // 3, n)
    monkeypatch.setenv("UMX_FORCE_PARTS", "3")
    eng = Engine(0)
    try:
        eng.load_weights(weights)
        cap, stats, _, e = capture(eng, z, pos, radius, max_neigh, monkeypatch, forces=True)
        assert eng.last_partitions() == 3
    finally:
        eng.close()
    held("G10 in 3 partitions", cap, part, n, stats, e, expect_stats=(len(full["src"]), max_neigh))


# ---- cells --------------------------------------------------------------------------------------------------------------------------------
CELL_RUNS = [("C4", 20), ("C4", None), ("Sh", 20), ("One", 20), ("One", None), ("Slab", 20)]


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("name,max_neigh", CELL_RUNS)
def test_cells(geng, name, max_neigh, per_image, double, monkeypatch):
    z, pos, cell, pbc, radius = G.cell_case(name)
    p = np.stack([pos, pos]) if per_image else pos[None]
    ref = G.reference_cell(p, cell, pbc, radius, max_neigh, double_positions=double)
    assert ref["exact"] and len(lattice_translations(cell, pbc, radius)[0]) == G.CELL_EXPECT[name]["shifts"]
    kw = dict(cells=np.stack([cell, cell]), pbc=pbc) if per_image else dict(cell=cell, pbc=pbc)
    cap, stats, shifts, e = capture(geng, z, p, radius, max_neigh, monkeypatch, double=double, **kw)
    assert shifts == G.CELL_EXPECT[name]["shifts"]
    held(f"{name} / {max_neigh}{' per image' if per_image else ''}{' f64' if double else ''}", cap, ref, len(p) * len(z), stats, e)


def test_more_candidates_than_the_truncating_fill_ranks(geng, monkeypatch):
    """Cap: 1188 candidates per row.  While max_neigh binds the evaluation is refused (capacity, the candidate-count message) and the
    engine works on; with max_neigh above the count the same geometry is accepted and its graph is the reference's"""
    from pdb2reaction_amd.engine import UmxError

    z, pos, cell, pbc, radius = G.cell_case("Cap")
    with pytest.raises(UmxError, match="candidates") as err:
        capture(geng, z, pos, radius, 50, monkeypatch, cell=cell, pbc=pbc)
    assert err.value.status == UMX_ERR_CAPACITY
    ref = G.reference_cell(pos, cell, pbc, radius, 2000)
    assert len(ref["src"]) == 64 * 1188
    cap, stats, shifts, e = capture(geng, z, pos, radius, 2000, monkeypatch, cell=cell, pbc=pbc)
    assert shifts == 125 and stats == (64 * 1188, 1188)
    held("Cap / 2000", cap, ref, 64, stats, e)
