"""The strain derivative of a graph-parallel evaluation (``umx_gp_begin_virial``): every engine's share of W, their sum in engine / rank
order, and the layers above -- all engines on device 0, as tests/test_gpu_local_pool.py (more than one physical device has never run).

1. Every engine's share against the float64 sum of ``vec_e (x) gvec_e`` over the edges THAT engine captured, times rmsd, per component
   within ``(n + 8) 2^-53 rmsd sum|terms|`` (the bound of tests/test_gpu_stress.py); the engines' edge lists, put one after another in
   engine order, are the single-engine edge list exactly; an engine without target nodes writes nine zeros.  Pools of 2 and 3 engines;
   triclinic (self-image edges, repeated pairs), slab, open cluster, ``max_neigh``-truncated rows.
2. E and F of the evaluation with the virial are bitwise those without it, under the same split.
3. The sum over the engines against the float64 checker (tests/stress_oracle.py) in every precision mode and both feed-forward forms,
   in units of the checker's own float32 deviation ``d32``: ``max|dW| <= m d32``, m per mode the smallest power of two at or above twice
   the worst ratio measured over the cases and pool sizes of this file (profiles/gp_stress.txt), capped at the one-GPU test's caps.  The
   yardstick is the checker, never the single-engine W -- that one is printed for information (graph-parallel forces differ from the
   single-engine ones at float32 summation order, and so does W).
4. Two runs give the same bits; the pool's W is its ``last_partials`` added by hand in engine order.
5. Two gloo ranks on the one GPU: ``GraphParallelEvaluator(virial=True)`` ends with the same W bits on both ranks, within bound 3.
6. ``UMXCalculator(stress=True, workers=2, gp_stress=True)``: sym(W) / V in Voigt order over the graph-parallel route; ``gp_stress=False``
   keeps engine 0 alone.

[3P-UNVERIFIED]: fairchem's own stress has not been compared."""
import importlib
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from stress_oracle import make_case, voigt_stress
from test_gpu_stress import M_CAP, reference, same_bits
from pdb2reaction_amd import synth, weights as W

pytestmark = pytest.mark.gpu

# m per precision mode (see 3. above).  Worst ratios max|dW| / d32 over {spectral, grid} x {triclinic, slab} x {2, 3 engines} and the
# two-rank run, one MI355X (profiles/gp_stress.txt): fp32 0.26, bf16x3 0.40, split-bf16 4.14, split 4.03 -- twice that, rounded up to a
# power of two:
M_GP = {"fp32": 1, "bf16x3": 1, "split-bf16": 16, "split": 16}
CASES = ("triclinic", "slab")
KEEP = "row_ptr,src,dst,evec,gvec"          # the captures this file reads (UMX_DEBUG_ONLY)


def make_pool(g, z, weights, cell=None, pbc=None, precision=None, **system_kw):
    from pdb2reaction_amd.parallel import LocalEnginePool

    pool = LocalEnginePool.create([0] * g, weights, precision=precision)
    pool.set_system(z, **system_kw)
    pool.set_cell(cell, pbc)
    return pool


def single_edges(weights, z, p32, cell, pbc, **system_kw):
    """(src, dst, evec) of the one-engine evaluation, and its W."""
    from pdb2reaction_amd.engine import Engine

    eng = Engine(0)
    try:
        eng.load_weights(weights)
        eng.set_system(z, **system_kw)
        eng.set_cell(cell, pbc)
        eng.debug_keep(True)
        w = eng.energy_forces_virial(p32)[2][0]
        return eng.debug_fetch("src", np.int32), eng.debug_fetch("dst", np.int32), eng.debug_fetch("evec"), w
    finally:
        eng.close()


# ---- 1. the shares, link by link ---------------------------------------------------------------------------------------------------------
def shares_check(pool, weights, p32, label):
    """Every engine's share against the float64 sum over its own captured edges; returns the captures per engine."""
    rmsd = float(np.asarray(weights["normalizer.rmsd"]).reshape(-1)[0])
    assert rmsd == 1.5                                                    # (the synthetic sets: a dropped factor shows)
    n = pool.natoms
    for eng in pool.engines:
        eng.debug_keep(True)
    try:
        e, f, w = pool.energy_forces_virial(p32, graph_parallel=True)
        caps = [(eng.debug_fetch("row_ptr", np.int32), eng.debug_fetch("src", np.int32), eng.debug_fetch("dst", np.int32),
                 eng.debug_fetch("evec").reshape(-1, 4), eng.debug_fetch("gvec").reshape(-1, 4)) for eng in pool.engines]
    finally:
        for eng in pool.engines:
            eng.debug_keep(False)
    assert pool.last_route == "graph-parallel" and pool.n_exchanges == 10 and len(pool.last_partials) == len(pool.engines)
    assert w.shape == (1, 3, 3) and w.dtype == np.float64
    for r, (row_ptr, src, dst, evec, gvec) in enumerate(caps):
        lo, hi = pool.last_blocks[r]
        part = pool.last_partials[r]
        assert part.shape == (9,) and part.dtype == np.float64
        assert len(row_ptr) == n + 1 and row_ptr[-1] == len(evec) == len(gvec) == len(src) == len(dst)
        deg = np.diff(row_ptr)
        assert (deg[:lo] == 0).all() and (deg[hi:] == 0).all()            # only the targets the engine owns have rows
        assert pool.engines[r].graph_stats()[0] == len(evec)
        if len(evec) == 0:
            assert same_bits(part, np.zeros(9)), (label, r, part)
            print(f"[gp virial link {label} engine {r}/{len(caps)}] targets [{lo}, {hi}): no edges, nine zeros")
            continue
        vec = evec[:, :3].astype(np.float64) * evec[:, 3:4].astype(np.float64)
        g64 = gvec.astype(np.float64)
        worst = 0.0
        for a in range(3):
            for b in range(3):
                terms = vec[:, a] * g64[:, b]
                host = rmsd * math.fsum(terms)
                bound = (len(terms) + 8) * 2.0 ** -53 * rmsd * float(np.abs(terms).sum())
                d = abs(part[3 * a + b] - host)
                worst = max(worst, d / bound if bound > 0 else (0.0 if d == 0 else np.inf))
                assert d <= bound, (label, r, a, b, part[3 * a + b], host, bound)
        print(f"[gp virial link {label} engine {r}/{len(caps)}] targets [{lo}, {hi}): {len(evec)} edges  worst |W_r - host| / bound = {worst:.3f}  "
              f"W_r,xx = {part[0]:+.6f} eV")
    return caps, w[0]


def union_is_the_single_engine_list(caps, single):
    src1, dst1, evec1, _ = single
    assert np.array_equal(np.concatenate([c[1] for c in caps]), src1)
    assert np.array_equal(np.concatenate([c[2] for c in caps]), dst1)
    assert same_bits(np.concatenate([c[3].reshape(-1) for c in caps]), evec1)


@pytest.mark.parametrize("g", [2, 3])
@pytest.mark.parametrize("name", ["triclinic", "slab", "triclinic max_neigh 7", "cluster"])
def test_shares_link_by_link(weights, monkeypatch, name, g):
    monkeypatch.setenv("UMX_DEBUG_ONLY", KEEP)
    kw = {}
    if name == "cluster":
        z, pos = synth.make_cluster(40, seed=4)
        p32, cell, pbc = pos.astype(np.float32)[None], None, None
    else:
        z, p32, cell, pbc = make_case(name.split()[0])
        if "max_neigh" in name:
            kw["max_neigh"] = 7
    single = single_edges(weights, z, p32, cell, pbc, **kw)
    with make_pool(g, z, weights, cell, pbc, **kw) as pool:
        caps, w = shares_check(pool, weights, p32[0], f"{name}, {g} engines")
    union_is_the_single_engine_list(caps, single)
    assert all(len(c[3]) > 0 for c in caps)
    assert np.abs(w).max() > (0.0 if "max_neigh" in name else 1.0)       # (seven neighbours per atom: a smaller W, not an empty one)
    if "max_neigh" in name:
        assert sum(len(c[3]) for c in caps) == 7 * len(z)
    if name == "triclinic":
        src, dst = np.concatenate([c[1] for c in caps]), np.concatenate([c[2] for c in caps])
        pairs = np.stack([src, dst], 1)
        assert (src == dst).any() and len(np.unique(pairs, axis=0)) < len(pairs)      # self-image edges and repeated pairs
    print(f"[gp virial link {name}, {g} engines] max|W - W(one engine)| = {np.abs(w - single[3]).max():.3e} eV (for information)")


def test_an_engine_without_target_nodes_writes_nine_zeros(weights, monkeypatch):
    """Two atoms over three engines: engine 2 owns [2, 2), has no edge and reads no edge buffer; its share is nine zeros."""
    monkeypatch.setenv("UMX_DEBUG_ONLY", KEEP)
    z = np.array([8, 1], dtype=np.int32)
    p32 = np.array([[[0.0, 0.0, 0.0], [0.7, 0.5, 0.4]]], dtype=np.float32)
    single = single_edges(weights, z, p32, None, None)
    with make_pool(3, z, weights) as pool:
        caps, w = shares_check(pool, weights, p32[0], "two atoms, 3 engines")
        assert pool.last_blocks[2] == (2, 2) and [len(c[3]) for c in caps] == [1, 1, 0]
        assert same_bits(pool.last_partials[2], np.zeros(9)) and np.abs(w).max() > 0
    union_is_the_single_engine_list(caps, single)


# ---- 2. E and F do not know about the virial ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [2, 3])
def test_energy_and_forces_are_those_without_the_virial(weights, g):
    for name in CASES:
        z, p32, cell, pbc = make_case(name)
        with make_pool(g, z, weights, cell, pbc) as pool:
            e0, f0 = pool.energy_forces(p32)
            assert pool.last_route == "graph-parallel" and pool.last_partials is None
            all0 = pool.last_all
            e1, f1, w1 = pool.energy_forces_virial(p32, graph_parallel=True)
            assert pool.last_route == "graph-parallel" and pool.n_exchanges == 10
            assert same_bits(e1, e0) and same_bits(f1, f0), (name, g)
            for r in range(g):                                              # on every engine, not only on engine 0
                assert same_bits(pool.last_all[r][0], all0[r][0]) and same_bits(pool.last_all[r][1], all0[r][1]), (name, g, r)
            e2, f2 = pool.energy_forces(p32)                                # and the plain route is its old self afterwards
            assert same_bits(e2, e0) and same_bits(f2, f0) and pool.last_partials is None


# ---- 3. against the float64 checker -------------------------------------------------------------------------------------------------------
def ratio_to_checker(w, ff, name, mode, label, w_single=None):
    z, p32, cell, pbc, w64, d32 = reference(ff, name)
    dw = float(np.abs(w - w64).max())
    info = "" if w_single is None else f"  [one engine: max|dW| = {np.abs(w_single - w64).max():.3e}, |W - W(one engine)| = {np.abs(w - w_single).max():.3e}]"
    print(f"[gp virial oracle {label} {ff} {name} {mode}] max|dW| = {dw:.3e} eV  d32 = {d32:.3e} eV  ratio = {dw / d32:.2f}  (m = {M_GP[mode]}){info}")
    return dw / d32


@pytest.mark.parametrize("ff", ["spectral", "grid"])
@pytest.mark.parametrize("mode", ["fp32", "split", "split-bf16", "bf16x3"])
def test_summed_virial_against_the_float64_checker(mode, ff):
    from pdb2reaction_amd.engine import Engine

    assert M_GP[mode] <= M_CAP[mode]
    w = W.make_synthetic_weights(0, **({"ff_type": "grid"} if ff == "grid" else {}))
    ratios = {}
    one = Engine(0, precision=mode)
    try:
        one.load_weights(w)
        singles = {}
        for name in CASES:
            z, p32, cell, pbc, _, _ = reference(ff, name)
            one.set_system(z)
            one.set_cell(cell, pbc)
            singles[name] = one.energy_forces_virial(p32)[2][0]
    finally:
        one.close()
    for g in (2, 3):
        for name in CASES:
            z, p32, cell, pbc, _, _ = reference(ff, name)
            with make_pool(g, z, w, cell, pbc, precision=mode) as pool:
                assert pool.precision_mode() == {"split": "split-f16"}.get(mode, mode)
                wg = pool.energy_forces_virial(p32, graph_parallel=True)[2][0]
                assert pool.last_route == "graph-parallel"
            ratios[(name, g)] = ratio_to_checker(wg, ff, name, mode, f"{g} engines", singles[name])
    assert max(ratios.values()) <= M_GP[mode], (mode, ff, ratios)


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [2, 3])
def test_two_runs_give_the_same_bits_and_the_sum_is_taken_in_engine_order(weights, g):
    z, p32, cell, pbc = make_case("slab")
    with make_pool(g, z, weights, cell, pbc) as pool:
        e0, f0, w0 = pool.energy_forces_virial(p32, graph_parallel=True)
        parts0 = [p.copy() for p in pool.last_partials]
        by_hand = parts0[0].copy()
        for part in parts0[1:]:
            by_hand = np.add(by_hand, part)
        assert same_bits(w0[0], by_hand.reshape(3, 3))
        pool.energy_forces(np.stack([p32[0], p32[0]]))                      # something else in between
        e1, f1, w1 = pool.energy_forces_virial(p32, graph_parallel=True)
        assert same_bits(w1, w0) and same_bits(e1, e0) and same_bits(f1, f0)
        assert all(same_bits(a, b) for a, b in zip(pool.last_partials, parts0))
    with make_pool(g, z, weights, cell, pbc) as again:                      # and on fresh engines
        assert same_bits(again.energy_forces_virial(p32, graph_parallel=True)[2], w0)


def test_stress_of_the_pool_and_the_refusal_with_recompute_mode_two(weights):
    z, p32, cell, pbc = make_case("triclinic")
    with make_pool(2, z, weights, cell, pbc) as pool:
        e, f, w = pool.energy_forces_virial(p32, graph_parallel=True)
        e2, f2, s = pool.energy_forces_stress(p32, graph_parallel=True)
        assert pool.last_route == "graph-parallel" and same_bits(s[0], voigt_stress(w[0], cell)) and same_bits(e2, e) and same_bits(f2, f)
        e1, f1, w1 = pool.energy_forces_virial(p32)                         # the default: engine 0 alone
        assert pool.last_route == "single"
        print(f"[gp virial pool] max|W(graph-parallel) - W(engine 0)| = {np.abs(w - w1).max():.3e} eV (for information)")
        pool.set_recompute(2)
        with pytest.raises(ValueError, match="recompute mode 2"):
            pool.energy_forces_virial(p32, graph_parallel=True)
        assert same_bits(pool.energy_forces_virial(p32)[2], w1) and pool.last_route == "single"
        pool.set_recompute(0)
        assert same_bits(pool.energy_forces_virial(p32, graph_parallel=True)[2], w)


# ---- 5. two ranks ----------------------------------------------------------------------------------------------------------------------------
def _rank(rank, world, port, name, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pdb2reaction_amd.engine import Engine
        from pdb2reaction_amd.parallel import GraphParallelEvaluator

        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        z, p32, cell, pbc = make_case(name)
        eng = Engine(0)
        eng.load_weights(W.make_synthetic_weights(0))
        eng.set_system(z)
        eng.set_cell(cell, pbc)
        pos = torch.as_tensor(p32[0], dtype=torch.float32, device=dev)
        plain = GraphParallelEvaluator(eng, len(z), dev)
        e0, f0 = plain(pos)
        gp = GraphParallelEvaluator(eng, len(z), dev, virial=True)
        e, f, w = gp(pos)
        e2, f2, w2 = gp(pos)
        out[rank] = (float(e[0]), f.cpu().numpy(), w.cpu().numpy(), gp.last_partials.cpu().numpy(), gp.n_exchanges, (gp.lo, gp.hi),
                     bool(torch.equal(e, e0) and torch.equal(f, f0)), bool(torch.equal(w2, w) and torch.equal(f2, f)))
        eng.close()
    finally:
        dist.destroy_process_group()


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_two_gloo_ranks_hold_the_same_virial():
    name, world = "triclinic", 2
    mgr = mp.get_context("spawn").Manager()   # (never FORK a process that has initialised the GPU)
    out = mgr.dict()
    mp.spawn(_rank, args=(world, _port(), name, out), nprocs=world, join=True)
    assert sorted(out.keys()) == [0, 1]
    e0, f0, w0, parts0, nx0, _, ef_same0, again0 = out[0]
    for r in range(world):
        e, f, w, parts, nx, (lo, hi), ef_same, again = out[r]
        assert w.shape == (3, 3) and w.dtype == np.float64 and parts.shape == (world, 9) and nx == 10
        assert ef_same and again                                           # E, F as without the virial; a second call: same bits
        assert same_bits(w, w0) and same_bits(parts, parts0) and e == e0 and same_bits(f, f0)      # identical on all ranks
        assert same_bits(w.reshape(-1), np.add(parts[0], parts[1]))        # the gathered shares, added in rank order
    assert np.abs(parts0[0]).max() > 0 and np.abs(parts0[1]).max() > 0 and not same_bits(parts0[0], parts0[1])
    ratio = ratio_to_checker(w0, "spectral", name, "bf16x3", "2 gloo ranks")
    assert ratio <= M_GP["bf16x3"], ratio


# ---- 6. the facade --------------------------------------------------------------------------------------------------------------------------
class _Atoms:
    def __init__(self, z, pos, cell, pbc):
        self.numbers, self._pos, self.cell, self.pbc, self.info = z, np.asarray(pos, dtype=np.float64), cell, pbc, {}

    def get_positions(self):
        return self._pos


def test_the_facade_sends_single_images_over_the_pool(weights, monkeypatch):
    A = importlib.import_module("pdb2reaction_amd.ase_calculator")
    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,0")
    z, p32, cell, pbc = make_case("triclinic")
    at = _Atoms(z, p32[0], cell, pbc)
    with make_pool(2, z, weights, cell, pbc) as pool:
        e0, f0, w0 = pool.energy_forces_virial(p32, graph_parallel=True)
        w_single = pool.energy_forces_virial(p32)[2]
    on = A.UMXCalculator(model="synthetic", stress=True, workers=2, gp_stress=True)
    try:
        s = on.get_stress(at)
        assert on.local_devices == [0, 0] and on._engine.last_route == "graph-parallel" and on._engine.n_exchanges == 10
        assert s.shape == (6,) and same_bits(s, voigt_stress(w0[0], cell))
        sym = 0.5 * (w0[0] + w0[0].T) / abs(np.linalg.det(cell))
        assert np.allclose(s, [sym[0, 0], sym[1, 1], sym[2, 2], sym[1, 2], sym[0, 2], sym[0, 1]], rtol=0, atol=1e-15)
        assert on.get_potential_energy(at) == e0[0] and same_bits(on.get_forces(at), f0[0].astype(np.float64))
    finally:
        on.close()
    off = A.UMXCalculator(model="synthetic", stress=True, workers=2, gp_stress=False)
    try:
        s = off.get_stress(at)
        assert off._engine.last_route == "single" and same_bits(s, voigt_stress(w_single[0], cell))
    finally:
        off.close()
