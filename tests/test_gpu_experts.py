"""Expert-form weights on the GPU: ``umx_set_expert_coefficients`` merges the Mixture-of-Linear-Experts
stacks of the 24 SO(2) weights and rebuilds their reverse-pass and plane copies on the device.

The yardstick everywhere is the HOST loader -- code this feature does not change -- fed with the blob merged on the host by
``checkpoint.merge_mole_ordered`` with the same coefficients.  Every comparison is bit for bit: no tolerance, no element left out.

The float32 arena ``weights:w`` of an expert-form engine also holds the routing tensors, which a merged blob does not carry, so the
two arenas are compared tensor by tensor through the engines' tensor tables (``weights:table``), every tensor of the merged engine;
``weights:dw`` and ``weights:bw`` are compared as raw bytes.  The plane records' fp16 scale has no fetch of its own: a wrong scale
changes the energies of the ``split`` mode, which are compared bit for bit below."""
import importlib
import os
import time

import numpy as np
import pytest

from pdb2reaction_amd import synth, weights as W

CK = importlib.import_module("pdb2reaction_amd.checkpoint")
pytestmark = pytest.mark.gpu

SYS_A = dict(charge=0, spin=1, task="omol")
SYS_B = dict(charge=-1, spin=2, task="omol")
VARIANTS = {"spectral": {}, "grid": dict(ff_type="grid", chg_spin_emb_type="pos_emb")}


@pytest.fixture(scope="module")
def experts():
    return {k: W.make_synthetic_experts(4, seed=5, **kw) for k, kw in VARIANTS.items()}


def host_merged(ws, z, charge=0, spin=1, task="omol"):
    alpha = CK.expert_coefficients(ws, z, charge, spin, task)
    return CK.merge_expert_set(ws, alpha, merged_for=W.system_record(z, charge, spin, task)), alpha


def table(eng):
    rows = [ln.split() for ln in eng.debug_fetch("weights:table", np.uint8).tobytes().decode().splitlines()]
    return {r[0]: (int(r[1]), int(r[2])) for r in rows}


def arenas(eng):
    return {n: eng.debug_fetch("weights:" + n, dt) for n, dt in (("w", np.uint32), ("dw", np.uint32), ("bw", np.uint16))}


def assert_same_arenas(dev, host):
    """dev: expert-form engine after set_system; host: engine that loaded the host-merged blob."""
    a, b = arenas(dev), arenas(host)
    assert a["dw"].size == b["dw"].size and np.array_equal(a["dw"], b["dw"]), "derived float32 weights (d_dw) differ"
    assert a["bw"].size == b["bw"].size and np.array_equal(a["bw"], b["bw"]), "plane copies (d_bw) differ"
    ta, tb = table(dev), table(host)
    assert set(tb) <= set(ta) and all(W.is_routing_tensor(k) for k in set(ta) - set(tb))
    for name, (off, cnt) in tb.items():
        o2, c2 = ta[name]
        assert c2 == cnt and np.array_equal(a["w"][o2:o2 + c2], b["w"][off:off + cnt]), f"{name} differs in d_w"
    # the engine lays its compact data section out as the merged blob's (routing tensors last): the shared prefix is the same bytes too
    assert np.array_equal(a["w"][: b["w"].size], b["w"])


def pair(ws, z, precision, sysk=SYS_A):
    """(expert-form engine, host-merged engine), both bound to the system."""
    from pdb2reaction_amd.engine import Engine

    merged, alpha = host_merged(ws, z, **sysk)
    dev, host = Engine(0, precision=precision), Engine(0, precision=precision)
    dev.load_weights(ws)
    assert dev.n_experts == 4 and dev.lib.umx_expert_count(dev._h) == 4
    dev.set_system(z, **sysk)
    assert np.array_equal(dev.expert_coefficients, alpha)
    host.load_weights(merged)
    assert host.n_experts == 0 and host.lib.umx_expert_count(host._h) == 0
    host.set_system(z, **sysk)
    return dev, host


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("align", ["2", "0"])
@pytest.mark.parametrize("precision", ["bf16x3", "split", "split-bf16", "fp32"])
def test_arenas_equal_host_loader(experts, precision, align, variant, monkeypatch):
    monkeypatch.setenv("UMX_ALIGN_PLANES", align)
    z, _, _ = synth.make_images(40, 1, seed=2)
    dev, host = pair(experts[variant], z, precision)
    try:
        assert dev.precision_mode() == host.precision_mode()
        assert_same_arenas(dev, host)
    finally:
        dev.close(); host.close()


@pytest.mark.parametrize("precision", ["bf16x3", "split", "split-bf16", "fp32"])
def test_energies_and_forces_equal_host_merged(experts, precision):
    for n_atoms, k in ((40, 3), (700, 2)):
        z, imgs, _ = synth.make_images(n_atoms, k, seed=2)
        dev, host = pair(experts["spectral"], z, precision)
        try:
            e0, f0 = host.energy_forces(imgs)
            e, f = dev.energy_forces(imgs)                                   # batched
            assert np.isfinite(e0).all() and np.array_equal(e, e0) and np.array_equal(f, f0)
            e1, f1 = dev.energy_forces(imgs[0])                              # single
            h1, g1 = host.energy_forces(imgs[0])
            assert np.array_equal(e1, h1) and np.array_equal(f1, g1)
        finally:
            dev.close(); host.close()


def _systems():
    za, ia, _ = synth.make_images(40, 2, seed=2)
    zb, ib, _ = synth.make_images(33, 2, seed=9)
    assert sorted(set(za.tolist())) != sorted(set(zb.tolist())) or len(za) != len(zb)
    return (za, ia, SYS_A), (zb, ib, SYS_B)


def _fresh_host(ws, z, imgs, sysk, precision=None):
    from pdb2reaction_amd.engine import Engine

    merged, _ = host_merged(ws, z, **sysk)
    host = Engine(0, precision=precision)
    try:
        host.load_weights(merged)
        host.set_system(z, **sysk)
        return host.energy_forces(imgs)
    finally:
        host.close()


def test_rebinding_one_engine(experts):
    from pdb2reaction_amd.engine import Engine

    ws = experts["spectral"]
    (za, ia, ka), (zb, ib, kb) = _systems()
    want_a, want_b = _fresh_host(ws, za, ia, ka), _fresh_host(ws, zb, ib, kb)
    eng = Engine(0)
    try:
        eng.load_weights(ws)
        eng.set_system(za, **ka)
        alpha_a = eng.expert_coefficients.copy()
        a1 = eng.energy_forces(ia)
        eng.set_system(zb, **kb)
        assert np.abs(eng.expert_coefficients - alpha_a).max() > 1e-6
        b1 = eng.energy_forces(ib)
        eng.set_system(za, **ka)
        a2 = eng.energy_forces(ia)
    finally:
        eng.close()
    for got, want in ((a1, want_a), (b1, want_b), (a2, want_a), (a2, a1)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(want_a[0], want_b[0][: len(want_a[0])])


def test_calculator_binds_two_systems_from_one_file(experts, tmp_path):
    U = importlib.import_module("pdb2reaction_amd.uma_pysis")
    ws = experts["spectral"]
    path = str(tmp_path / "experts.umxw")
    W.save_weights(path, ws)
    sym = {v: k for k, v in synth.Z_OF_SYMBOL.items()}
    for (z, imgs, sysk) in _systems():
        elem = [sym[int(v)] for v in z]
        x = (imgs[0] * U.ANG2BOHR).reshape(-1)
        merged, _ = host_merged(ws, z, **sysk)
        mpath = str(tmp_path / f"merged_{len(z)}.umxw")
        W.save_weights(mpath, merged)
        got = U.uma_pysis(model=path, charge=sysk["charge"], spin=sysk["spin"], task_name=sysk["task"])
        want = U.uma_pysis(model=mpath, charge=sysk["charge"], spin=sysk["spin"], task_name=sysk["task"])
        try:
            r, r0 = got.get_forces(elem, x), want.get_forces(elem, x)
            assert r["energy"] == r0["energy"] and np.array_equal(r["forces"], r0["forces"])
        finally:
            got.close(); want.close()


def test_local_pool_of_two_engines(experts):
    from pdb2reaction_amd.parallel import LocalEnginePool

    ws = experts["spectral"]
    for (z, imgs, sysk) in _systems():
        want = _fresh_host(ws, z, imgs, sysk)
        with LocalEnginePool.create([0, 0], ws) as pool:
            pool.set_system(z, **sysk)
            e, f = pool.energy_forces(imgs)                      # two images: one per engine
            assert np.array_equal(e, want[0]) and np.array_equal(f, want[1])
            pool.set_system(z, **sysk)                           # binding again merges again: same bits
            e2, f2 = pool.energy_forces(imgs)
            assert np.array_equal(e2, e) and np.array_equal(f2, f)


def test_widening_keeps_the_merged_weights(experts, monkeypatch):
    """An expert-form engine in ``split`` driven beyond the fp16 operand range (UMX_ERR_RANGE: a status code, the way
    tests/test_gpu_parity.py::test_fp16_operand_range_is_guarded does it) ends in ``split-bf16`` with the merged weights intact."""
    from pdb2reaction_amd.engine import Engine

    big = W.WeightSet(experts["spectral"], meta=experts["spectral"].meta)
    key = "blocks.0.edge_wise.so2_conv_1.rad_func.fc3.weight"
    big[key] = (np.asarray(big[key]) * 3e4).astype(np.float32)
    z, imgs, _ = synth.make_images(40, 1, seed=2)
    merged, _ = host_merged(big, z)
    ref, eng = Engine(0, precision="split-bf16"), Engine(0, precision="split")
    try:
        ref.load_weights(merged)
        ref.set_system(z)
        e0, f0 = ref.energy_forces(imgs)
        assert np.isfinite(e0).all() and np.isfinite(f0).all()
        eng.load_weights(big)
        eng.set_system(z)
        with pytest.warns(RuntimeWarning, match="split-bf16"):
            e, f = eng.energy_forces(imgs)
        assert eng.widened and eng.precision_mode() == "split-bf16" and eng.n_experts == 4
        assert np.array_equal(e, e0) and np.array_equal(f, f0)
        assert_same_arenas(eng, ref)
    finally:
        ref.close(); eng.close()


def test_call_order_and_arguments(experts):
    import ctypes as C

    from pdb2reaction_amd.engine import Engine, UmxError

    ws = experts["spectral"]
    z, imgs, _ = synth.make_images(40, 1, seed=2)
    merged, alpha = host_merged(ws, z)
    dp = C.POINTER(C.c_double)
    p = np.ascontiguousarray(imgs, dtype=np.float32)
    eng, host = Engine(0), Engine(0)
    try:
        eng.load_weights(ws)
        eng.natoms = len(z)

        def status(call):
            st = call()
            return st, eng.lib.umx_last_error(eng._h).decode()

        zz = np.ascontiguousarray(z, dtype=np.int32)
        st, msg = status(lambda: eng.lib.umx_set_system(eng._h, len(zz), zz.ctypes.data_as(C.POINTER(C.c_int32)), 0, 1, 1, 0.0, 0))
        assert st == -1 and "umx_set_expert_coefficients" in msg                         # UMX_ERR_ARG, names the missing call
        with pytest.raises(UmxError, match="umx_set_expert_coefficients") as ei:
            eng.energy_forces(imgs)                                                        # evaluation before coefficients
        assert ei.value.status == -1
        st, msg = status(lambda: eng.lib.umx_set_expert_coefficients(eng._h, 3, alpha.ctypes.data_as(dp)))
        assert st == -1 and "3 coefficients" in msg and "4 experts" in msg
        bad = alpha.copy(); bad[2] = np.nan
        st, msg = status(lambda: eng.lib.umx_set_expert_coefficients(eng._h, 4, bad.ctypes.data_as(dp)))
        assert st == -1 and "coefficient 2 is not finite" in msg
        host.load_weights(merged)
        st = host.lib.umx_set_expert_coefficients(host._h, 4, alpha.ctypes.data_as(dp))
        assert st == -1 and "already merged" in host.lib.umx_last_error(host._h).decode()
        # both engines are still usable, and agree
        eng.set_system(z)
        host.set_system(z)
        e, f = eng.energy_forces(imgs)
        e0, f0 = host.energy_forces(imgs)
        assert np.array_equal(e, e0) and np.array_equal(f, f0)
        # new coefficients unbind the system: the evaluation says so, and binding again makes it usable again
        assert eng.lib.umx_set_expert_coefficients(eng._h, 4, alpha.ctypes.data_as(dp)) == 0
        with pytest.raises(UmxError, match="bind a system first"):
            eng.energy_forces(imgs)
        eng.set_system(z)
        assert np.array_equal(eng.energy_forces(imgs)[0], e0)
    finally:
        eng.close(); host.close()


def test_full_size_32_experts():
    """n = 32 experts at the UMA-S shapes (0.58 GB of stacks): arena equality in the default mode, and the time to bind a system on a
    loaded engine (printed; profiles/expert_merge.txt keeps a recorded run)."""
    from pdb2reaction_amd.engine import Engine

    ws = W.make_synthetic_experts(32, seed=1)
    z, imgs, _ = synth.make_images(40, 1, seed=2)
    merged, alpha = host_merged(ws, z)
    dev, host = Engine(0), Engine(0)
    try:
        dev.load_weights(ws)
        assert dev.n_experts == 32
        t0 = time.perf_counter()
        dev.set_system(z)
        t1 = time.perf_counter()
        ms = float(dev.debug_fetch("experts:kernel_ms", np.float32)[0])
        stack_bytes = 4 * sum(int(np.asarray(ws[k]).size) for k in W.EXPERT_WEIGHT_NAMES)
        print(f"[experts n=32] bind {1e3 * (t1 - t0):.2f} ms wall, merge + pack kernels {ms:.3f} ms, stacks {stack_bytes / 1e6:.0f} MB "
              f"-> {stack_bytes / (ms * 1e-3) / 1e12:.2f} TB/s")
        host.load_weights(merged)
        host.set_system(z)
        assert_same_arenas(dev, host)
        e, f = dev.energy_forces(imgs)
        e0, f0 = host.energy_forces(imgs)
        assert np.array_equal(e, e0) and np.array_equal(f, f0)
    finally:
        dev.close(); host.close()
