"""The gate-reverse epilogue of the conv-2^T products (umx_gemm_q.h EP = 1) against the two links it replaces.

In the bf16x3 reverse pass conv 2^T can apply gate^T to its finished elements and write g_hg, conv 1^T's quad-row operand, itself
(`UMX_GATE_EPI`: 0 never, 1 unless debug captures are on or the chunk has fewer than 16 257 edges, 2 always) instead of storing g_hid for k_gate_edge_bwd_q3<3> to read back.  The
epilogue performs the same float32 operations in the same order, so everything must come out bit for bit: the operand `ghgq.i` of every
layer, and energies and forces.

What can go wrong is the row tiling and the padding of the last row group, so the systems are chosen by their directed-edge count `ne`
(`synth.make_images` clusters; a neighbour cap makes the graph asymmetric, which is the only way to an odd `ne`):

    atoms  cap    ne
       7     3    21   < 64, ne % 4 = 1
       7     5    35   < 64, ne % 4 = 3
       8     -    56   < 64, ne % 4 = 0
      10     -    90   between 64 and 128: a partial half-height complex tile; ne % 4 = 2
      14     -   182   between 128 and 256
      18     -   298   above 256, no multiple of 256
     600     -  37 k   >= 32 768: `fills` holds for both complex products, which take their wide forms
    2 x 7    -  42 + 40  a batch whose second image starts inside a row group, at edge 42; the whole batch also goes through the operand
                        and launch checks

The batch's second image starts at an EVEN edge on purpose.  Every producer of a split-mode GEMM operand negates the rows of odd edge index
and the GEMM epilogue restores the sign (`row_sign(e, odd_sign)` in umx_edge.h, `GemmPL::odd_sign`: e is the edge's index in the CHUNK), so
that the matrix core's one-sided rounding alternates in sign from row to row.  An image whose first edge is odd in the batch therefore has
every one of its rows rounded the other way than when it is evaluated alone: its last bits differ between the two, in the unfused path as
in the fused one (the existing batch-independence tests all start their second image at an even edge: 78, 156).  Only an even start can
be held to "identical alone and in a batch", and 42 % 4 = 2 is the one even start inside a row group.

`test_sizes_cover_the_tile_cases` holds the table to what the engine's graph reports.  Every size runs with `UMX_GEMM_HALF` 0 and 3, so
both heights of every form are launched.
"""
import os

import numpy as np
import pytest
import torch

from pdb2reaction_amd import synth
from pdb2reaction_amd import weights as W

pytestmark = pytest.mark.gpu

H = W.HIDDEN_CHANNELS
HG = 2 * H + 9 * H                  # columns of g_hg: [gate l = 1 | gate l = 2 | the nine m-primary rows of g_hpre]
CASES = [(7, 3, 1), (7, 5, 1), (8, None, 1), (10, None, 1), (14, None, 1), (18, None, 1), (600, None, 1), (7, None, 2)]      # (atoms, neighbour cap, images)
HALVES = ("0", "3")
CONV2T = {("384", "384"), ("256", "256"), ("128", "128")}       # (N, K) of conv 2^T's three products; no other reverse product has them
GHG = [f"ghgq.{i}" for i in range(W.NUM_LAYERS)]


def _make_engines():
    """engines[half][epi] for UMX_GEMM_HALF in HALVES and UMX_GATE_EPI in 0, 1, 2 (both are read when an engine is created)."""
    from pdb2reaction_amd.engine import Engine

    w = W.make_synthetic_weights(0)
    old = {k: os.environ.get(k) for k in ("UMX_GEMM_HALF", "UMX_GATE_EPI", "UMX_DEBUG_ONLY")}
    made = {}
    try:
        os.environ["UMX_DEBUG_ONLY"] = "ghgq."          # (read at every capture: the 37 k-edge case would hold gigabytes of the other buffers)
        for half in HALVES:
            for epi in (0, 1, 2):
                os.environ["UMX_GEMM_HALF"], os.environ["UMX_GATE_EPI"] = half, str(epi)
                eng = Engine(0, precision="bf16x3")
                made[half, epi] = eng
                eng.load_weights(w)
        yield made
    finally:
        for eng in made.values():
            eng.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines():
    yield from _make_engines()


def _system(n, images=1):
    z, pos, _ = synth.make_images(n, images)
    return z, pos.astype(np.float32)


def _evaluate(eng, z, pos, cap, captures):
    """E, F (and with captures ghgq.i of every layer and the launch log) of one evaluation; the edge count of its graph."""
    eng.debug_keep(captures)
    try:
        eng.set_system(z, max_neigh=cap)
        e, f = eng.energy_forces(pos)
        out = {"E": e.copy(), "F": f.copy()}
        ne = eng.graph_stats()[0]
        if captures:
            for name in GHG:
                out[name] = eng.debug_fetch(name).copy()
            out["launches"] = eng.debug_fetch("gemm:launches", dtype=np.uint8).tobytes().decode().splitlines()
    finally:
        eng.debug_keep(False)
    return out, ne


def _rows(quad, ne):
    """A captured float32 quad-row operand (blocks of 4 rows x 16 columns) as the bit patterns of its rows: (rows < ne, the padding rows)."""
    groups = (ne + 3) // 4
    assert quad.size == groups * 4 * HG, f"ghgq holds {quad.size} floats, not {groups} row groups of 4 x {HG}"
    rows = quad.view(np.uint32).reshape(groups, HG // 16, 4, 16).transpose(0, 2, 1, 3).reshape(groups * 4, HG)
    return rows[:ne], rows[ne:]


def _same(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)), torch.from_numpy(np.ascontiguousarray(b).view(np.uint8)))


def _operand_differences(ref, fused, ne):
    """The layers whose g_hg operand differs in some bit of its rows < ne, or holds a non-finite value in the last group's padding."""
    bad = []
    for name in GHG:
        want, _ = _rows(ref[name], ne)
        got, pad = _rows(fused[name], ne)
        if not _same(want, got):
            bad.append(name)
        elif not np.isfinite(pad.view(np.float32)).all():
            bad.append(name + " (padding)")
    return bad


@pytest.fixture(scope="module")
def results(engines):
    """Per case and tile height: the unfused and the fused evaluation with captures, and both without -- computed once, shared by the tests."""
    memo = {}

    def get(n, cap, images, half):
        key = (n, cap, images, half)
        if key not in memo:
            z, pos = _system(n, images)
            ref, ne0 = _evaluate(engines[half, 0], z, pos, cap, True)
            fused, ne2 = _evaluate(engines[half, 2], z, pos, cap, True)
            plain0, _ = _evaluate(engines[half, 0], z, pos, cap, False)
            plain1, ne1 = _evaluate(engines[half, 1], z, pos, cap, False)
            assert ne0 == ne1 == ne2
            memo[key] = {"ne": ne0, "ref": ref, "fused": fused, "plain0": plain0, "plain1": plain1, "bad": _operand_differences(ref, fused, ne0)}
            if ne0 > 4096:                          # compared; the large case's operands are not kept (0.2 GB per layer)
                for name in GHG:
                    del ref[name], fused[name]
        return memo[key]

    return get


def test_sizes_cover_the_tile_cases(results, engines):
    counts = [results(n, cap, images, "0")["ne"] for n, cap, images in CASES if images == 1]
    assert {ne % 4 for ne in counts} == {0, 1, 2, 3}, counts
    assert any(ne < 64 for ne in counts), counts
    assert any(64 < ne < 128 for ne in counts), counts
    assert any(128 < ne < 256 for ne in counts), counts
    assert any(ne > 256 and ne % 256 != 0 and ne < 32768 for ne in counts), counts
    assert any(ne >= 32768 for ne in counts), counts
    z, pos = _system(7, images=2)
    _, both = _evaluate(engines["0", 1], z, pos, None, False)
    _, first = _evaluate(engines["0", 1], z, pos[:1], None, False)
    assert first % 4 == 2 and both > first, f"the second image of the batch starts at edge {first}: not inside a row group at an even edge"


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("n,cap,images", CASES)
def test_fused_operand_bit_for_bit(results, n, cap, images, half):
    r = results(n, cap, images, half)
    bad = r["bad"]
    assert not bad, f"ne = {r['ne']}, UMX_GEMM_HALF = {half}: conv 2^T's gate epilogue writes another g_hg than k_gate_edge_bwd_q3 in {bad}"
    assert _same(r["ref"]["E"], r["fused"]["E"]) and _same(r["ref"]["F"], r["fused"]["F"])


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("n,cap,images", CASES)
def test_fused_energy_forces_bit_for_bit(results, n, cap, images, half):
    r = results(n, cap, images, half)
    assert np.isfinite(r["plain0"]["E"]).all() and np.isfinite(r["plain0"]["F"]).all()
    assert _same(r["plain0"]["E"], r["plain1"]["E"]), f"ne = {r['ne']}: energies differ between UMX_GATE_EPI = 0 and 1"
    assert _same(r["plain0"]["F"], r["plain1"]["F"]), f"ne = {r['ne']}: forces differ between UMX_GATE_EPI = 0 and 1"
    # (UMX_GATE_EPI = 1 applies the epilogue from 16 257 edges on -- the 600-atom case; below, the fused evaluation is the one with captures)
    assert _same(r["plain0"]["E"], r["fused"]["E"]) and _same(r["plain0"]["F"], r["fused"]["F"]), f"ne = {r['ne']}: UMX_GATE_EPI = 2 differs"


@pytest.mark.parametrize("half", HALVES)
def test_fused_batch_independence(engines, half):
    """An image evaluated alone and as the second image of a batch (42 + 40 edges: it starts inside a row group), UMX_GATE_EPI = 1."""
    eng = engines[half, 1]
    z, pos = _system(7, images=2)
    both, _ = _evaluate(eng, z, pos, None, False)
    alone, _ = _evaluate(eng, z, pos[1:2], None, False)
    assert _same(alone["E"][0], both["E"][1]) and _same(alone["F"][0], both["F"][1])
    unfused, _ = _evaluate(engines[half, 0], z, pos, None, False)
    assert _same(unfused["E"], both["E"]) and _same(unfused["F"], both["F"])
    # UMX_GATE_EPI = 1 leaves so small a chunk to the unfused links: the same again with the epilogue forced on
    forced, _ = _evaluate(engines[half, 2], z, pos, None, False)
    forced_alone, _ = _evaluate(engines[half, 2], z, pos[1:2], None, False)
    assert _same(forced_alone["E"][0], forced["E"][1]) and _same(forced_alone["F"][0], forced["F"][1])
    assert _same(unfused["E"], forced["E"]) and _same(unfused["F"], forced["F"])


def _table(eng, name):
    return eng.debug_fetch(name, dtype=np.uint8).tobytes().decode().splitlines()


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("n,cap,images", CASES)
def test_fused_launches_keep_their_tile_form(engines, results, n, cap, images, half):
    """"gemm:table" keeps its 39 rows, the fused kernels have a table of their own, and with UMX_GATE_EPI = 2 exactly the conv-2^T launches
    move to it -- with the wide / half fields the unfused product has at that size."""
    assert len(_table(engines[half, 2], "gemm:table")) == 39
    gate = _table(engines[half, 2], "gemm:table_gate")
    assert len(gate) == 6 and len(set(gate)) == 6 and all(row.split()[0] == "Q_BF16_GATE" for row in gate)
    r = results(n, cap, images, half)
    ref, fused = r["ref"]["launches"], r["fused"]["launches"]
    assert len(ref) == len(fused) and ref
    moved = 0
    for a, b in zip(ref, fused):
        fa, fb = a.split(), b.split()
        assert len(fa) == len(fb) == 11
        if fa[0] == "rev" and (fa[8], fa[9]) in CONV2T:
            assert fa[1] == "Q_BF16" and fb[1] == "Q_BF16_GATE" and fa[2:] == fb[2:], (a, b)
            assert " ".join(fb[1:7]) in gate, b
            moved += 1
        else:
            assert a == b
    assert moved == 3 * W.NUM_LAYERS
    if r["ne"] >= 32768:
        assert all(b.split()[3] == "1" for b in fused if b.split()[1] == "Q_BF16_GATE" and b.split()[2] == "1"), "the complex products run wide here"


def test_comparison_rejects_swapped_gate_columns(results):
    """The comparison itself: with the gradients of the two gates exchanged in a copy of the fused capture it must report every layer."""
    r = results(18, None, 1, "0")
    ne = r["ne"]
    mutant = dict(r["fused"])
    for name in GHG:
        quad = r["fused"][name].copy()
        blocks = quad.reshape((ne + 3) // 4, HG // 16, 4, 16)
        blocks[:, : H // 16], blocks[:, H // 16: 2 * H // 16] = blocks[:, H // 16: 2 * H // 16].copy(), blocks[:, : H // 16].copy()
        mutant[name] = quad
    assert _operand_differences(r["ref"], r["fused"], ne) == []
    assert _operand_differences(r["ref"], mutant, ne) == GHG
