"""Recompute plans on the GPU (``umx_set_recompute``): the replay issues the stored plan's forward kernels again on the same inputs, so a
recompute plan must give the stored plan's bits -- in one piece and in partitions, in every precision mode, with both feed-forward forms
-- and it must move the capacity wall: an image no stored plan holds within a workspace limit evaluates with mode 1."""
import importlib

import numpy as np
import pytest

from pdb2reaction_amd import synth, weights as W
from pdb2reaction_amd.engine import Engine, UmxError, workspace_bytes

pytestmark = pytest.mark.gpu

TOL_E = 1e-4   # eV
TOL_F = 1e-3   # eV/Angstrom


def make(weights, recompute=None):
    eng = Engine(0, recompute=recompute)
    eng.load_weights(weights)
    return eng


def pair(weights, z, monkeypatch, parts=0, precision=None):
    """(stored, recompute-always) engines with the same partitioning and precision mode, system bound."""
    if parts:
        monkeypatch.setenv("UMX_FORCE_PARTS", str(parts))
    if precision:
        monkeypatch.setenv("UMX_PRECISION", precision)
    a, b = make(weights, 0), make(weights, 2)
    for e_ in (a, b):
        e_.set_system(z)
    return a, b


def same_bits(a, b, imgs, parts):
    e0, f0 = a.energy_forces(imgs)
    e1, f1 = b.energy_forces(imgs)
    print(f"parts={parts} images={len(imgs)}: max|dE| = {np.abs(e1 - e0).max():.3e} eV  max|dF| = {np.abs(f1 - f0).max():.3e} eV/A")
    assert a.last_recompute() == 0 and b.last_recompute() == 1
    assert a.last_partitions() == parts and b.last_partitions() == parts
    assert np.array_equal(e1, e0) and np.array_equal(f1, f0)
    eo0, _ = a.energy_forces(imgs, forces=False)             # energy only: nothing is replayed, the forward is the stored plan's
    eo1, none = b.energy_forces(imgs, forces=False)
    assert none is None and np.array_equal(eo1, eo0) and np.array_equal(eo1, e0)
    e2, f2 = b.energy_forces(imgs)                           # and again after the energy-only call, on the same workspace
    assert np.array_equal(e2, e0) and np.array_equal(f2, f0)
    return e1, f1


@pytest.mark.parametrize("n,k,seed", [(97, 3, 11), (300, 2, 4)])
@pytest.mark.parametrize("parts", [0, 2, 3, 5])
def test_recompute_is_the_stored_plan_bit_for_bit(weights, monkeypatch, parts, n, k, seed):
    z, imgs, _ = synth.make_images(n, k, seed=seed)
    a, b = pair(weights, z, monkeypatch, parts)
    try:
        same_bits(a, b, imgs, parts)
        if n == 97:
            # the dilute system of test_one_image_in_target_node_partitions: partitions without edges, an isolated atom
            zd = np.array([8, 1, 1, 6, 7, 1], dtype=np.int32)
            pd = np.array([[[0, 0, 0], [0.96, 0, 0], [-0.3, 0.9, 0], [30, 0, 0], [31.2, 0.4, 0.1], [90.0, 0, 0]]], np.float32)
            for e_ in (a, b):
                e_.set_system(zd)
            _, fd = same_bits(a, b, pd, parts)
            assert np.all(fd[0, 5] == 0.0)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("mode", ["bf16x3", "split", "split-bf16", "fp32"])
@pytest.mark.parametrize("parts", [0, 3])
def test_every_precision_mode(weights, monkeypatch, mode, parts):
    z, imgs, _ = synth.make_images(150, 2, seed=13)
    a, b = pair(weights, z, monkeypatch, parts, precision=mode)
    try:
        assert b.precision_mode() == {"split": "split-f16"}.get(mode, mode)
        same_bits(a, b, imgs, parts)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("parts", [0, 2, 5])
def test_grid_feed_forward(monkeypatch, parts):
    w = W.make_synthetic_weights(0, ff_type="grid", chg_spin_emb_type="pos_emb")
    z, imgs, _ = synth.make_images(97, 2, seed=11)
    a, b = pair(w, z, monkeypatch, parts)
    try:
        assert "ff=grid" in b.model_variant()
        same_bits(a, b, imgs, parts)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("env", [{"UMX_STREAMS": "2"}, {"UMX_MAX_CHUNK_IMAGES": "1"}], ids=["two-lanes", "one-image-chunks"])
def test_chunks_and_lanes(weights, monkeypatch, env):
    """Several chunks reuse one slot one after another; two lanes have a workspace -- and a slot -- each."""
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    z, imgs, _ = synth.make_images(97, 4, seed=11)
    a, b = pair(weights, z, monkeypatch)
    try:
        same_bits(a, b, imgs, 0)
        assert b.last_lanes() == (2 if "UMX_STREAMS" in env else 1)
    finally:
        a.close()
        b.close()


def test_recompute_against_the_float64_oracle(weights, oracle, monkeypatch):
    z, imgs, _ = synth.make_images(97, 2, seed=11)
    monkeypatch.setenv("UMX_RECOMPUTE", "2")                 # the environment form of the switch, read at umx_create
    one = make(weights)
    monkeypatch.setenv("UMX_FORCE_PARTS", "3")
    three = make(weights)
    try:
        for eng, parts in ((one, 0), (three, 3)):
            eng.set_system(z)
            e, f = eng.energy_forces(imgs)
            assert eng.last_recompute() == 1 and eng.last_partitions() == parts
            for k in range(len(imgs)):
                e_ref, f_ref = oracle.energy_forces(z, imgs[k].astype(np.float32).astype(np.float64))
                print(f"parts={parts} image {k}: |dE| = {abs(e[k] - e_ref):.3e} eV  max|dF| = {np.abs(f[k] - f_ref).max():.3e} eV/A")
                assert abs(e[k] - e_ref) <= TOL_E and np.abs(f[k] - f_ref).max() <= TOL_F
    finally:
        one.close()
        three.close()


def wall_limit(eng, n, ne):
    """A workspace limit from the planner's own arithmetic (umx_workspace_bytes), not from trying the engine: half of what a recompute
    plan of the image needs in ONE piece.  No stored plan fits it -- a stored plan in equal partitions is a lower bound of the real
    (uneven) ones -- and a recompute plan fits it only in partitions, with room for partitions 1.4x the even size."""
    limit = workspace_bytes(n, ne, 0, 1, engine=eng) // 2
    stored = [workspace_bytes(n, ne, p, 0, engine=eng) for p in [0] + list(range(2, 17))]
    rc = [workspace_bytes(n, ne, p, 1, engine=eng) for p in range(2, 17)]
    print(f"limit {limit >> 20} MiB; stored plans need >= {min(stored) >> 20} MiB; recompute in one piece {2 * limit >> 20} MiB, "
          f"in equal partitions >= {min(rc) >> 20} MiB (P = {2 + int(np.argmin(rc))})")
    assert min(stored) > limit and 1.4 * min(rc) <= limit
    return limit


def test_the_wall_moves(weights):
    z, imgs, _ = synth.make_images(300, 1, seed=4)
    ref, eng = make(weights), make(weights)
    try:
        ref.set_system(z)
        e0, f0 = ref.energy_forces(imgs)                     # unconstrained, stored, one piece
        assert ref.last_partitions() == 0 and ref.last_recompute() == 0
        ne, _ = ref.graph_stats()
        limit = wall_limit(eng, 300, ne)
        eng.set_system(z)
        eng.set_workspace_limit(limit)
        with pytest.raises(UmxError, match=r"one image \(300 atoms, \d+ directed edges\) needs \d+ MiB.*16 partitions.*UMX_RECOMPUTE") as ei:
            eng.energy_forces(imgs)                          # mode 0: today's wall
        assert ei.value.status == -4
        eng.set_recompute(1)
        e, f = eng.energy_forces(imgs)
        print(f"mode 1: {eng.last_partitions()} partitions, workspace {eng.workspace_stats()[0] >> 20} MiB, "
              f"max|dE| = {np.abs(e - e0).max():.3e} eV  max|dF| = {np.abs(f - f0).max():.3e} eV/A")
        assert eng.last_recompute() != 0
        assert 2 <= eng.last_partitions() <= 16
        assert 0 < eng.workspace_stats()[0] <= limit
        assert np.abs(e - e0).max() <= 2e-5 and np.abs(f - f0).max() <= 2e-5          # partition sums reorder float32 adds
        eng.set_workspace_limit(0)                           # the image fits again: mode 1 goes back to the stored plan, bitwise
        e2, f2 = eng.energy_forces(imgs)
        assert eng.last_recompute() == 0 and eng.last_partitions() == 0 and np.array_equal(e2, e0) and np.array_equal(f2, f0)
        eng.set_recompute(2)                                 # ... and a change of plan kind on a live engine re-carves the workspace
        e3, f3 = eng.energy_forces(imgs)
        assert eng.last_recompute() == 1 and np.array_equal(e3, e0) and np.array_equal(f3, f0)
        eng.set_recompute(0)
        e4, f4 = eng.energy_forces(imgs)
        assert eng.last_recompute() == 0 and np.array_equal(e4, e0) and np.array_equal(f4, f0)
    finally:
        ref.close()
        eng.close()


def test_mode_1_is_inert_when_the_image_fits(weights):
    z, imgs, _ = synth.make_images(97, 3, seed=11)
    a, b = make(weights, 0), make(weights, 1)
    try:
        for e_ in (a, b):
            e_.set_system(z)
        e0, f0 = a.energy_forces(imgs)
        e1, f1 = b.energy_forces(imgs)
        assert np.array_equal(e1, e0) and np.array_equal(f1, f0)
        assert b.last_recompute() == 0 and b.last_partitions() == 0
        assert b.workspace_stats() == a.workspace_stats()
    finally:
        a.close()
        b.close()


def test_graph_parallel_entry_refuses_mode_2(weights):
    import torch

    z, imgs, _ = synth.make_images(20, 1, seed=1)
    eng = make(weights, 2)
    try:
        eng.set_system(z)
        pos = torch.tensor(np.asarray(imgs[0], np.float32), device="cuda")
        e = torch.zeros(1, dtype=torch.float64, device="cuda")
        f = torch.zeros(20, 3, dtype=torch.float32, device="cuda")
        with pytest.raises(UmxError, match=r"umx_gp_begin.*recompute mode 2") as ei:
            eng.gp_begin(pos.data_ptr(), 0, 20, e.data_ptr(), f.data_ptr())
        assert ei.value.status == -1                     # UMX_ERR_ARG
        with pytest.raises(UmxError, match="mode must be 0"):
            eng.set_recompute(3)
    finally:
        eng.close()


def test_the_local_pool_evaluates_a_batch_no_stored_plan_holds(monkeypatch):
    """Two engines on ONE device divide its workspace cap (UMX_WS_GB=1: 512 MiB each): 240-atom images, whose stored plans need more
    than that however they are partitioned, evaluate as a batch with recompute=1."""
    U = importlib.import_module("pdb2reaction_amd.uma_pysis")
    n = 240
    z, imgs, _ = synth.make_images(n, 2, seed=4)
    p64 = np.asarray(imgs, dtype=np.float64)
    symbols = [synth.SYMBOLS[int(q)] for q in z]
    ref = U.UMAcore(symbols, model="synthetic")
    try:
        r0 = ref.compute_batch(p64)
        ne = ref.engine.graph_stats()[0] // 2                                    # per image (the two differ by a few edges)
        half = (1 << 30) // 2
        stored = [workspace_bytes(n, int(ne * 0.98), p, 0, engine=ref.engine) for p in [0] + list(range(2, 17))]
        rc = [workspace_bytes(n, int(ne * 1.02), p, 1, engine=ref.engine) for p in range(2, 17)]
        print(f"{ne} edges per image: stored plans need >= {min(stored) >> 20} MiB, recompute in equal partitions >= {min(rc) >> 20} MiB, each engine has {half >> 20} MiB")
        assert min(stored) > half and 1.4 * min(rc) <= half
    finally:
        ref.close()
    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,0")
    monkeypatch.setenv("UMX_WS_GB", "1")
    off = U.UMAcore(symbols, model="synthetic", workers=2)
    try:
        with pytest.raises(UmxError, match="16 partitions") as ei:
            off.compute_batch(p64)
        assert ei.value.status == -4
    finally:
        off.close()
    core = U.UMAcore(symbols, model="synthetic", workers=2, recompute=1)
    try:
        assert core.local_devices == [0, 0] and len(core._pool.engines) == 2
        r = core.compute_batch(p64)
        assert core._pool.last_route == "batch" and [e.last_recompute() for e in core._pool.engines] == [1, 1]
        assert all(2 <= e.last_partitions() <= 16 and e.workspace_stats()[0] <= half for e in core._pool.engines)
        de = np.abs(np.asarray(r["energy"]) - np.asarray(r0["energy"])).max()
        df = np.abs(np.asarray(r["forces"]) - np.asarray(r0["forces"])).max()
        print(f"pool, recompute=1: partitions {[e.last_partitions() for e in core._pool.engines]}  max|dE| = {de:.3e}  max|dF| = {df:.3e}")
        assert de <= 2e-5 and df <= 2e-5
    finally:
        core.close()
