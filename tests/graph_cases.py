"""Geometries, float64 references and the checker of the neighbour-graph links -- a helper, not a test.

tests/test_gpu_graph_links.py runs the checker on the engine's captures, tests/test_graph_links_cpu.py on captures synthesised from
the reference (and on mutations of them, which it must reject).  The reference is ``oracle.escn_md_oracle.radius_graph`` for open
boundaries and ``periodic_oracle.periodic_radius_graph`` for cells, on the float64 values of the positions the engine was given;
nothing here is transcribed from a kernel.

Lattice cases have dyadic coordinates (multiples of 1/4 A, below 32 A): every coordinate difference, every translation and every d^2
is exact in float32 and in float64 alike, so ties and pairs at exactly the cutoff are the same facts on both sides.  Random cases
assert that no decision is closer than 1e-5 relative in d^2 (the cutoff, the pair that decides the cap).
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import escn_md_oracle as O
from oracle import tables as OT
from periodic_oracle import lattice_translations, periodic_radius_graph
from pdb2reaction_amd import synth

U = 2.0 ** -24
DEFAULT_MAX_NEIGH = OT.MAX_NEIGHBORS          # what set_system(max_neigh=None) binds
NAMES = "row_ptr,src,dst,out_ptr,out_edge,evec"
CLEAR = 1e-5                                  # random cases: relative distance in d^2 every decision keeps from its threshold

# evec, per element, first order in u (every factor below is (1 + delta), |delta| <= u; the slack to the next integer covers u^2):
#   open float path    dx = fl(x_j - x_i)                                        1 rounding, relative to |dx|
#                      d2 = fma(dz, dz, fma(dy, dy, fl(dx dx)))                  squares of the components: 2; three roundings on a sum of
#                                                                                positive terms: 3                  -> (1 + u)^5
#                      d = sqrtf(d2)                                             5 / 2 + 1 = 3.5                    -> K_D = 4
#                      n_c = fl(dx_c fl(1 / d))                                  1 (dx_c) + 3.5 + 1 (1 / d) + 1     = 6.5 -> K_N = 7
#   double path        dx = (float)(x_j [+ t] - x_i in float64): the one float32 rounding of the open path, and 2^-53 per float64
#                      operation against the 1/2 u of slack above -> the same constants
#   periodic float     dx = fl(fl(x_j - x_i) + t32), t32 = the float32 table entry of t: absolute a_c = u (|x_j - x_i| + |t| + |vec|)
#                      per component instead of the relative u |dx|; | |v + a| - |v| | <= |a|_2, so
#                      |d - d64| <= K_D u d64 + |a|_2,  |n_c - n64_c| <= K_N u |n64_c| + (a_c + |n64_c| |a|_2) / d64
K_D, K_N = 4, 7


class GraphMismatch(AssertionError):
    pass


def _fail(what, detail=""):
    raise GraphMismatch(f"{what}{': ' if detail else ''}{detail}")


# ---- geometries ---------------------------------------------------------------------------------------------------------------------------
def species(n):
    """two elements, alternating"""
    return np.where(np.arange(n) % 2 == 0, 6, 8).astype(np.int32)


def cubic_lattice(m, spacing=1.5):
    """m x m x m simple cubic points, the last index running fastest"""
    g = np.arange(m, dtype=np.float64) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def cell_atoms(cell, m, offset):
    """m x m x m atoms at the fractional coordinates (k + offset) / m of the cell"""
    k = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return ((k + offset) / m) @ np.asarray(cell, dtype=np.float64)


# open boundaries: name -> (lattice points per axis, radius, max_neigh)
OPEN = {
    "G10": (5, 6.0, 10), "G26": (5, 6.0, 26), "G53": (5, 6.0, 53), "G124": (5, 6.0, 124), "Gfree": (5, 6.0, None),
    "S1236": (13, 10.0, 12), "D400": (8, 12.0, 400),
}
# what the oracle gives for them (measured once on the CPU, asserted by open_facts consumers): edges, rows that truncate, rows with a tie
# across the cap, ordered pairs at exactly the cutoff among the candidates, candidate range, out-degree range
OPEN_EXPECT = {
    "G10": dict(edges=1250, trunc_rows=125, tie_rows=117, at_cutoff=150, cand=(53, 124), outdeg=(3, 20)),
    "G26": dict(edges=3250, trunc_rows=125, tie_rows=98, at_cutoff=150, cand=(53, 124)),
    "G53": dict(edges=6625, trunc_rows=117, tie_rows=109, at_cutoff=150, cand=(53, 124), rows_at_cap=8),
    "G124": dict(edges=10784, trunc_rows=0, at_cutoff=150, cand=(53, 124), rows_at_cap=1),
    "Gfree": dict(edges=10784, trunc_rows=0, at_cutoff=150, cand=(53, 124), outdeg=(53, 124)),
    "S1236": dict(edges=26364, trunc_rows=2197, tie_rows=2197, cand_over_1024=147, cand_max=1236),
    "D400": dict(edges=203864, trunc_rows=480, tie_rows=360, cand=(340, 511), outdeg=(209, 511), indeg_max=400),
}

C4_CELL = np.eye(3) * 4.0
SH_CELL = np.array([[4.0, 0.0, 0.0], [2.0, 4.0, 0.0], [0.0, 2.0, 4.0]])
ONE_CELL = np.eye(3) * 2.0
SLAB_CELL = np.array([[4.0, 0.0, 0.0], [2.0, 4.0, 0.0], [0.0, 0.0, 4.0]])
# cells: name -> (cell, pbc, atoms per axis, fractional offset, radius)
CELLS = {
    "C4": (C4_CELL, (True, True, True), 2, 0.25, 6.0),
    "Sh": (SH_CELL, (True, True, True), 2, 0.25, 6.0),
    "One": (ONE_CELL, (True, True, True), 1, 0.25, 6.0),
    "Slab": (SLAB_CELL, (True, True, False), 2, 0.25, 6.0),
    "Cap": (C4_CELL, (True, True, True), 4, 0.5, 6.5),
}
CELL_EXPECT = {
    "C4": dict(shifts=125, cand=122, at_cutoff=240),
    "Sh": dict(shifts=125, cand=114, at_cutoff=80, outdeg20=(19, 21)),
    "One": dict(shifts=729, cand=122, at_cutoff=30),
    "Slab": dict(shifts=25, cand=55, at_cutoff=48),
    "Cap": dict(shifts=125, cand=1188),
}


def open_case(name):
    m, radius, max_neigh = OPEN[name]
    pos = cubic_lattice(m)
    return species(len(pos)), pos, radius, max_neigh


def cell_case(name):
    cell, pbc, m, offset, radius = CELLS[name]
    pos = cell_atoms(cell, m, offset)
    return species(len(pos)), pos, cell, pbc, radius


def is_dyadic(pos, *more):
    """every coordinate (and every entry of `more`) is a multiple of 1/4 below 32: differences, translations and d^2 are exact in float32"""
    return all(bool(np.all(np.asarray(a) * 4 == np.round(np.asarray(a) * 4)) and np.abs(a).max() < 32.0) for a in (pos,) + more)


# ---- references ---------------------------------------------------------------------------------------------------------------------------
def _cap(max_neigh):
    return DEFAULT_MAX_NEIGH if max_neigh is None else int(max_neigh)


def candidates_open(p64, radius):
    """d2 [N, N] float64 with inf where (j -> i) is no candidate"""
    d2 = ((p64[:, None, :] - p64[None, :, :]) ** 2).sum(-1)
    ok = (d2 <= radius * radius) & ~np.eye(len(p64), dtype=bool)
    return np.where(ok, d2, np.inf)


def candidates_cell(p64, cell, pbc, radius):
    """d2 [N, T * N] float64 (candidate index = translation index * N + source) with inf where there is no candidate"""
    ints, _ = lattice_translations(cell, pbc, radius)
    tv = ints.astype(np.float64) @ np.asarray(cell, dtype=np.float64)
    d2 = (((p64[None, None, :, :] + tv[None, :, None, :]) - p64[:, None, None, :]) ** 2).sum(-1)
    ok = (d2 <= radius * radius) & (d2 > 0.0)
    return np.where(ok, d2, np.inf).reshape(len(p64), -1), len(ints)


def cap_facts(d2c, radius, max_neigh):
    """what the candidate table says about the cap and the cutoff: input conditions of a case"""
    m = _cap(max_neigh)
    cand = np.isfinite(d2c).sum(1)
    s = np.sort(d2c, axis=1)
    trunc = cand > m
    tie = np.zeros(len(cand), dtype=bool)
    gap = np.full(len(cand), np.inf)
    if m < d2c.shape[1]:
        tie = trunc & (s[:, m - 1] == s[:, m])
        with np.errstate(invalid="ignore"):
            gap = np.where(trunc, (s[:, m] - s[:, m - 1]) / s[:, m], np.inf)
    fin = d2c[np.isfinite(d2c)]
    return dict(cand=cand, trunc_rows=int(trunc.sum()), tie_rows=int(tie.sum()), at_cutoff=int((fin == radius * radius).sum()),
                rows_at_cap=int((cand == m).sum()), cap_gap=float(gap.min()),
                cutoff_gap=float(np.abs(fin / (radius * radius) - 1.0).min()) if len(fin) else np.inf)


def _edges(src, dst, vec, absd=None, abst=None, exact=False, shift=None, tidx=None):
    """a reference graph: per edge the source, the target, r_j + t - r_i; the translation t and its index (cells); |r_j - r_i| and |t| per
    component where the engine's path forms the vector in two float32 steps; exact: d^2 of every edge is a float32 number"""
    src = np.asarray(src, dtype=np.int64)
    return dict(src=src, dst=np.asarray(dst, dtype=np.int64), vec=np.asarray(vec, dtype=np.float64), absd=absd, abst=abst, exact=exact,
                shift=shift, tidx=np.zeros(len(src), dtype=np.int64) if tidx is None else np.asarray(tidx, dtype=np.int64))


def reference_open(pos, radius, max_neigh, double_positions=False):
    """The oracle's graph of every image of pos [K, N, 3] (or [N, 3]), node offset k N, on the float64 values of the positions the
    engine reads (rounded to float32 unless double_positions)."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, np.shape(pos)[-2], 3)
    p = pos if double_positions else pos.astype(np.float32).astype(np.float64)
    n = p.shape[1]
    src, dst, vec = [], [], []
    for k, pk in enumerate(p):
        s, d = O.radius_graph(torch.as_tensor(pk), radius, _cap(max_neigh))
        s, d = s.numpy(), d.numpy()
        src.append(s + k * n), dst.append(d + k * n), vec.append(pk[s] - pk[d])
    return _edges(np.concatenate(src), np.concatenate(dst), np.concatenate(vec), exact=is_dyadic(p))


def reference_cell(pos, cell, pbc, radius, max_neigh, double_positions=False):
    """As reference_open with a cell (the same for every image): rows in (source, translation index) order."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, np.shape(pos)[-2], 3)
    p = pos if double_positions else pos.astype(np.float32).astype(np.float64)
    n = p.shape[1]
    src, dst, vec, absd, abst, shift, tidx = [], [], [], [], [], [], []
    for k, pk in enumerate(p):
        s, d, sh, ti = periodic_radius_graph(pk, cell, pbc, radius, _cap(max_neigh))
        s, d, sh = s.numpy(), d.numpy(), sh.numpy()
        src.append(s + k * n), dst.append(d + k * n), vec.append(pk[s] + sh - pk[d]), shift.append(sh), tidx.append(ti.numpy())
        absd.append(np.abs(pk[s] - pk[d])), abst.append(np.abs(sh))
    periodic_float = not double_positions
    return _edges(np.concatenate(src), np.concatenate(dst), np.concatenate(vec), np.concatenate(absd) if periodic_float else None,
                  np.concatenate(abst) if periodic_float else None, exact=is_dyadic(p, np.asarray(cell)), shift=np.concatenate(shift),
                  tidx=np.concatenate(tidx))


def restrict(ref, lo, hi):
    """the reference rows of the targets [lo, hi) only: what one target-node partition builds"""
    keep = (ref["dst"] >= lo) & (ref["dst"] < hi)
    return {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in ref.items()}


# ---- the checker --------------------------------------------------------------------------------------------------------------------------
def check_graph(cap, ref, nn, stats=None, expect_stats=None):
    """cap: the captures row_ptr, src, dst, out_ptr, out_edge (int) and evec (float32 [E, 4]) of one evaluation; ref: a reference_*
    result; nn: nodes.  Raises GraphMismatch naming the first row that differs.  Returns the largest |error| / bound of (d, n)."""
    src, dst = np.asarray(cap["src"], dtype=np.int64), np.asarray(cap["dst"], dtype=np.int64)
    row_ptr, out_ptr = np.asarray(cap["row_ptr"], dtype=np.int64), np.asarray(cap["out_ptr"], dtype=np.int64)
    out_edge = np.asarray(cap["out_edge"], dtype=np.int64)
    rs, rd = ref["src"], ref["dst"]
    ne = len(rs)
    # 1. the edge list
    if not (np.array_equal(dst, rd) and np.array_equal(src, rs)):
        both = min(len(src), ne)
        bad = np.nonzero((src[:both] != rs[:both]) | (dst[:both] != rd[:both]))[0]
        t = int(rd[bad[0]]) if len(bad) else int(rd[both]) if both < ne else int(dst[both])
        _fail("edge list", f"{len(src)} edges against {ne}; first difference in the row of target {t}: sources {src[dst == t].tolist()} "
                           f"against the reference's {rs[rd == t].tolist()}")
    # 2. in-degree rows
    indeg = np.bincount(rd, minlength=nn)
    want = np.concatenate([[0], np.cumsum(indeg)])
    if not np.array_equal(row_ptr, want):
        bad = np.nonzero(row_ptr[: len(want)] != want[: len(row_ptr)])[0]
        _fail("row_ptr", f"{len(row_ptr)} entries against {len(want)}, first difference at node {int(bad[0]) if len(bad) else -1}")
    # 3. the counts the host read back
    if stats is not None:
        exp = expect_stats if expect_stats is not None else (ne, int(indeg.max()) if ne else 0)
        if tuple(stats) != tuple(exp):
            _fail("graph_stats", f"{tuple(stats)} against {tuple(exp)}")
    # 4. out-edge lists, every row, the empty ones too
    outdeg = np.bincount(rs, minlength=nn)
    want = np.concatenate([[0], np.cumsum(outdeg)])
    if not np.array_equal(out_ptr, want):
        bad = np.nonzero(out_ptr[: len(want)] != want[: len(out_ptr)])[0]
        _fail("out_ptr", f"{len(out_ptr)} entries against {len(want)}, first difference at node {int(bad[0]) if len(bad) else -1}")
    want_edges = np.argsort(rs, kind="stable")                      # ascending edge ids within every source's row
    if not np.array_equal(out_edge, want_edges):
        bad = np.nonzero(out_edge[: ne] != want_edges[: len(out_edge)])[0]
        n = int(np.searchsorted(want, bad[0], side="right") - 1) if len(bad) else -1
        _fail("out_edge", f"first difference in the row of source {n}: {out_edge[want[n]: want[n + 1]].tolist() if n >= 0 else len(out_edge)}")
    # 5. edge vectors, per element
    evec = np.asarray(cap["evec"], dtype=np.float32).reshape(-1, 4)
    if evec.shape[0] != ne:
        _fail("evec", f"{evec.shape[0]} rows against {ne}")
    if ne == 0:
        return 0.0, 0.0
    if not np.isfinite(evec).all():
        _fail("evec", "non-finite entry")
    vec = ref["vec"]
    d64 = np.sqrt((vec * vec).sum(1))
    n64 = vec / d64[:, None]
    b_d, b_n = K_D * U * d64, K_N * U * np.abs(n64)
    if ref["absd"] is not None:                                      # periodic float path
        a = U * (ref["absd"] + ref["abst"] + np.abs(vec)) * (1.0 + 8 * U)
        a2 = np.sqrt((a * a).sum(1))
        b_d = b_d + a2
        b_n = b_n + (a + np.abs(n64) * a2[:, None]) / d64[:, None]
    e_d, e_n = np.abs(evec[:, 3].astype(np.float64) - d64), np.abs(evec[:, :3].astype(np.float64) - n64)
    if (e_d > b_d).any():
        e = int(np.argmax(e_d - b_d))
        _fail("evec distance", f"edge {e} ({int(rs[e])} -> {int(rd[e])}): {evec[e, 3]!r} against {d64[e]!r}, bound {b_d[e]:.3e}")
    if (e_n > b_n).any():
        e = int(np.argmax((e_n - b_n).max(1)))
        _fail("evec direction", f"edge {e} ({int(rs[e])} -> {int(rd[e])}): {evec[e, :3]!r} against {n64[e]!r}, bound {b_n[e]!r}")
    if ref["exact"]:                                                 # d^2 is exact in float32: the distance is its correctly rounded root
        d2 = (vec * vec).sum(1)
        if not np.array_equal(d2.astype(np.float32).astype(np.float64), d2):
            _fail("input condition", "d^2 of a dyadic lattice is not a float32 number")
        if not np.array_equal(evec[:, 3], np.sqrt(d2.astype(np.float32))):
            e = int(np.nonzero(evec[:, 3] != np.sqrt(d2.astype(np.float32)))[0][0])
            _fail("evec distance bits", f"edge {e}: {evec[e, 3]!r} against float32(sqrt({d2[e]!r}))")
    live = b_n > 0
    if (e_n[~live] != 0).any():
        _fail("evec direction", "a component that is exactly zero in float64 is not zero")
    return float((e_d / b_d).max()), float((e_n[live] / b_n[live]).max()) if live.any() else 0.0


# ---- captures synthesised from a reference (the CPU file; also what a mutation starts from) -------------------------------------------
def _fma32(a, b, c):
    """float32 fma through float64: the product of two float32 numbers is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def evec_float32(ps, pd, shift=None):
    """a numpy float32 restatement of the edge vector: difference (plus the float32 translation), fma chain, root, reciprocal, product;
    ps / pd: the positions of source and target [E, 3] (float32, or float64 for the double entry: one rounding of the float64 value)"""
    if ps.dtype == np.float64:
        dv = (ps + (0.0 if shift is None else shift) - pd).astype(np.float32)
    else:
        dv = ps - pd
        if shift is not None:
            dv = dv + shift.astype(np.float32)
    d2 = _fma32(dv[:, 2], dv[:, 2], _fma32(dv[:, 1], dv[:, 1], dv[:, 0] * dv[:, 0]))
    d = np.sqrt(d2)
    inv = np.float32(1.0) / d
    return np.concatenate([dv * inv[:, None], d[:, None]], axis=1).astype(np.float32)


def synth_captures(src, dst, evec, nn):
    """the five integer arrays a correct engine would capture for this edge list (sorted by target), with the given evec"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    return dict(src=src.astype(np.int32), dst=dst.astype(np.int32), evec=np.asarray(evec, dtype=np.float32).reshape(-1, 4),
                row_ptr=np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=nn))]).astype(np.int32),
                out_ptr=np.concatenate([[0], np.cumsum(np.bincount(src, minlength=nn))]).astype(np.int32),
                out_edge=np.argsort(src, kind="stable").astype(np.int32))


def captures_of(ref, pos, nn):
    """what a correct engine would capture for the reference graph: pos [K, N, 3] in the dtype the engine reads (float32 or float64)"""
    p = np.asarray(pos).reshape(-1, 3)
    return synth_captures(ref["src"], ref["dst"], evec_float32(p[ref["src"]], p[ref["dst"]], ref["shift"]), nn)


# ---- random geometries --------------------------------------------------------------------------------------------------------------------
def random_facts(pos, radius, max_neigh):
    """the smallest relative distance in d^2 of any pair from the cutoff, and of any cap-deciding pair of candidates from each other, over
    the images of pos [K, N, 3] (the float64 values of the float32 positions)"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, np.shape(pos)[-2], 3).astype(np.float32).astype(np.float64)
    cut, capg, trunc = np.inf, np.inf, 0
    for pk in pos:
        d2 = ((pk[:, None, :] - pk[None, :, :]) ** 2).sum(-1)
        off = d2[~np.eye(len(pk), dtype=bool)]
        cut = min(cut, float(np.abs(off / (radius * radius) - 1.0).min()))
        f = cap_facts(candidates_open(pk, radius), radius, max_neigh)
        capg, trunc = min(capg, f["cap_gap"]), trunc + f["trunc_rows"]
    return dict(cutoff_gap=cut, cap_gap=capg, trunc_rows=trunc)


def is_clear(pos, radius, caps):
    return all(min(f["cutoff_gap"], f["cap_gap"]) > CLEAR for f in (random_facts(pos, radius, m) for m in caps))


def seam_case(n, caps=(8, None), radius=6.0):
    """synth.make_cluster(n) with the first seed from the default on whose decisions are clear of their thresholds"""
    for seed in range(synth.DEFAULT_SEED, synth.DEFAULT_SEED + 20):
        z, pos = synth.make_cluster(n, seed)
        if is_clear(pos[None], radius, caps):
            return z, pos
    raise AssertionError("no clear seed")


def batch_case(n, k, caps=(20,), radius=6.0):
    for seed in range(synth.DEFAULT_SEED, synth.DEFAULT_SEED + 20):
        z, imgs, _ = synth.make_images(n, k, seed=seed)
        if is_clear(imgs, radius, caps):
            return z, imgs
    raise AssertionError("no clear seed")


# ---- mutations the checker must reject ----------------------------------------------------------------------------------------------------
def break_tie_upwards(ref, p64, d2c, max_neigh, tv=None):
    """The reference graph of ONE image with one tie at the cap decided the other way: in the first row whose candidates of rank
    max_neigh - 1 and max_neigh are equidistant, the kept one (lower source / translation index) is replaced by the dropped one.
    d2c: the candidate table [N, T N]; tv [T, 3]: the translations (None: open boundaries)."""
    n, m = len(p64), _cap(max_neigh)
    s = np.sort(d2c, axis=1)
    i = int(np.nonzero(np.isfinite(s[:, m]) & (s[:, m - 1] == s[:, m]))[0][0])
    order = np.argsort(d2c[i], kind="stable")
    out_c, in_c = int(order[m - 1]), int(order[m])
    assert in_c > out_c and d2c[i, in_c] == d2c[i, out_c]
    row = np.nonzero(ref["dst"] == i)[0]
    code = ref["tidx"][row] * n + ref["src"][row]
    at = row[np.nonzero(code == out_c)[0][0]]
    src, tidx, vec = ref["src"].copy(), ref["tidx"].copy(), ref["vec"].copy()
    shift = None if ref["shift"] is None else ref["shift"].copy()
    src[at], tidx[at] = in_c % n, in_c // n
    t = np.zeros(3) if tv is None else tv[in_c // n]
    vec[at] = p64[in_c % n] + t - p64[i]
    if shift is not None:
        shift[at] = t
    perm = np.arange(len(src))
    perm[row] = row[np.lexsort((tidx[row], src[row]))]                # the row back in (source, translation index) order
    return _edges(src[perm], ref["dst"], vec[perm], exact=ref["exact"], shift=None if shift is None else shift[perm], tidx=tidx[perm])


def drop_edge(ref, e):
    keep = np.ones(len(ref["src"]), dtype=bool)
    keep[e] = False
    return {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
