"""Several engines in ONE process (``parallel.LocalEnginePool``; the reference's single-process ``workers=G`` calculator,
``uma_pysis.py:220-242``) -- all on device 0, which rehearses the host path and the in-process peer sum (``umx_peer_sum``) on a one-GPU
box.  More than one physical device has never run: peer access, cross-device events and xGMI traffic are not covered here.

1. the peer sum against numpy's float32 addition in list order, bit for bit, in every participant's buffer;
2. batches dealt over a pool against one engine, bit for bit;
3. one image graph-parallel over the pool against the float64 oracle (BASELINE tolerances), all engines identical in every bit;
4. the calculator boundary with ``UMX_LOCAL_DEVICES=0,0``.
At most four engines are alive at a time."""
import importlib

import numpy as np
import pytest
import torch

from pdb2reaction_amd import synth, weights as W

pytestmark = pytest.mark.gpu

E_TOL, F_TOL = 1e-4, 1e-3            # BASELINE.json tolerances (eV, eV/A), as tests/test_gpu_graph_parallel.py uses for the rank-level mode


def _sequential_f32(bufs):
    acc = bufs[0].copy()
    for b in bufs[1:]:
        acc = (acc + b).astype(np.float32)            # float32 + float32 in numpy is one IEEE float32 addition
    return acc


def _peer_inputs(g, count, seed):
    """Mixed signs, magnitudes over 2^-20 .. 2^20: the order of addition decides the low bits."""
    rng = np.random.default_rng(seed)
    mant = rng.uniform(1.0, 2.0, size=(g, count))
    expo = rng.integers(-20, 21, size=(g, count))
    sign = rng.choice([-1.0, 1.0], size=(g, count))
    return [np.ascontiguousarray((sign[r] * mant[r] * np.exp2(expo[r])).astype(np.float32)) for r in range(g)]


@pytest.mark.parametrize("g", [2, 3, 8])
@pytest.mark.parametrize("count_kind", ["three", "4g-1", "1152x130", "1152x130+5"])
def test_peer_sum_is_numpy_float32_addition_in_list_order(g, count_kind):
    from pdb2reaction_amd.engine import peer_sum

    count = {"three": 3, "4g-1": 4 * g - 1, "1152x130": 1152 * 130, "1152x130+5": 1152 * 130 + 5}[count_kind]
    # inputs that can tell a wrong evaluation from the right one: for G >= 3 the REVERSED list order must give at least one different bit
    # (otherwise the order of addition is not visible and the test proves nothing); two addends commute in IEEE arithmetic, so there the
    # float32 sum must at least differ from the exact one (a wider or fused evaluation would show).  First seed that qualifies.
    def telling(host, want):
        if g > 2:
            return not np.array_equal(want.view(np.uint32), _sequential_f32(host[::-1]).view(np.uint32))
        return not np.array_equal(want.astype(np.float64), host[0].astype(np.float64) + host[1].astype(np.float64))

    for seed in range(500):
        host = _peer_inputs(g, count, 1000 * g + seed)
        want = _sequential_f32(host)
        if telling(host, want):
            break
    assert telling(host, want), "the inputs do not make the order / the rounding of the additions visible"
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(device=dev) for _ in range(g)]
    bufs = []
    for r in range(g):
        with torch.cuda.stream(streams[r]):
            bufs.append(torch.from_numpy(host[r]).to(dev, non_blocking=False))
    torch.cuda.synchronize(dev)
    for rep in range(2):                              # a second exchange on the same streams re-uses the event set
        if rep == 1:
            for r in range(g):
                with torch.cuda.stream(streams[r]):
                    bufs[r].copy_(torch.from_numpy(host[r]))
        peer_sum([b.data_ptr() for b in bufs], count, [0] * g, [s.cuda_stream for s in streams])
        for r in range(g):
            streams[r].synchronize()
            got = bufs[r].cpu().numpy()
            assert got.shape == (count,)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"participant {r} of {g}, count {count}, exchange {rep}"


def test_peer_sum_refuses_bad_arguments():
    from pdb2reaction_amd.engine import UmxError, peer_sum

    a = torch.zeros(64, dtype=torch.float32, device="cuda:0")
    b = torch.zeros(64, dtype=torch.float32, device="cuda:0")
    with pytest.raises(UmxError, match="16-byte aligned"):
        peer_sum([a.data_ptr() + 4, b.data_ptr()], 8, [0, 0], [0, 0])
    with pytest.raises(UmxError, match="same buffer"):
        peer_sum([a.data_ptr(), a.data_ptr()], 8, [0, 0], [0, 0])
    with pytest.raises(UmxError, match="out of range"):
        peer_sum([a.data_ptr(), b.data_ptr()], 8, [0, 4096], [0, 0])


def _pool(g, z, precision=None, **kw):
    from pdb2reaction_amd.parallel import LocalEnginePool

    pool = LocalEnginePool.create([0] * g, W.make_synthetic_weights(0), precision=precision, **kw)
    pool.set_system(z)
    return pool


@pytest.mark.parametrize("precision", [None, "fp32"])
def test_batches_equal_the_single_engine_bit_for_bit(precision):
    from pdb2reaction_amd.engine import Engine

    z, imgs, _ = synth.make_images(130, 16, seed=3)
    p32 = np.asarray(imgs, dtype=np.float32)
    one = Engine(0, precision=precision)
    one.load_weights(W.make_synthetic_weights(0))
    one.set_system(z)
    want = {k: one.energy_forces(p32[:k]) for k in (16, 5, 2)}
    one.close()
    for g in (2, 3):
        with _pool(g, z, precision) as pool:
            assert pool.devices == [0] * g
            for k in (16, 5, 2):
                e, f = pool.energy_forces(p32[:k])
                assert pool.last_route == "batch" and e.dtype == np.float64 and f.dtype == np.float32
                assert np.array_equal(e, want[k][0]), (g, k, precision)
                assert np.array_equal(f.view(np.uint32), want[k][1].view(np.uint32)), (g, k, precision)
                if k < g:
                    assert pool.last_blocks[-1][0] == pool.last_blocks[-1][1]          # an engine without images


@pytest.mark.parametrize("n_atoms,g", [(130, 2), (130, 3), (20, 2), (20, 3), (2, 3)])
def test_one_image_over_the_pool(oracle, n_atoms, g):
    """(2 atoms over 3 engines: engine 2 owns no target node, hence no edge, and takes part with all-zero partial sums.)"""
    z, imgs, _ = synth.make_images(n_atoms, 1, seed=8)
    p32 = np.asarray(imgs[0], dtype=np.float32)
    e_orc, f_orc = oracle.energy_forces(z, p32.astype(np.float64))
    with _pool(g, z) as pool:
        e, f = pool.energy_forces(p32)
        assert pool.last_route == "graph-parallel" and pool.n_exchanges == 10
        edges = [eng.graph_stats()[0] for eng in pool.engines]
        if n_atoms < g:
            assert pool.last_blocks[-1][0] == pool.last_blocks[-1][1] and edges[-1] == 0
        de, df = abs(float(e[0]) - e_orc), float(np.abs(f[0] - f_orc).max())
        print(f"[pool of {g}, {n_atoms} atoms] |dE| = {de:.3e} eV  max|dF| = {df:.3e} eV/A  edges per engine {edges}")
        assert de <= E_TOL and df <= F_TOL
        e0, f0 = pool.last_all[0]
        for r in range(1, g):
            er, fr = pool.last_all[r]
            assert np.array_equal(er, e0) and np.array_equal(fr.view(np.uint32), f0.view(np.uint32)), f"engine {r} differs from engine 0"
        e2, f2 = pool.energy_forces(p32)                                                # and again: same bits
        assert np.array_equal(e2, e) and np.array_equal(f2.view(np.uint32), f.view(np.uint32))
        # the pool goes back to batches afterwards
        e3, _ = pool.energy_forces(np.stack([p32, p32]))
        assert pool.last_route == "batch" and e3[0] == e3[1] and abs(e3[0] - e_orc) <= E_TOL


def test_calculator_with_two_local_engines(oracle, monkeypatch):
    U = importlib.import_module("pdb2reaction_amd.uma_pysis")
    z, imgs, _ = synth.make_images(12, 6, seed=4)
    elem = [synth.SYMBOLS[int(q)] for q in z]
    xb = np.asarray(imgs, dtype=np.float64).reshape(6, -1) * U.ANG2BOHR
    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    with U.uma_pysis(model="synthetic", workers=1, freeze_atoms=[1], out_hess_torch=False) as c1:
        fb1 = c1.get_forces_batch(elem, xb)
        h1 = c1.get_hessian(elem, xb[0])
        s1 = c1.get_forces(elem, xb[0])
        assert c1._core is not None and c1._core.local_devices == [0] and c1._core._pool is None
    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,0")
    with U.uma_pysis(model="synthetic", workers=2, freeze_atoms=[1], out_hess_torch=False) as c2:
        fb2 = c2.get_forces_batch(elem, xb)
        core = c2._core
        assert core.local_devices == [0, 0] and len(core._pool) == 2 and core.parallel_predict
        assert core._pool.last_route == "batch"
        h2 = c2.get_hessian(elem, xb[0])
        s2 = c2.get_forces(elem, xb[0])
        assert core._pool.last_route == "graph-parallel" and core._pool.n_exchanges == 10
    assert np.array_equal(fb2["energy"], fb1["energy"]) and np.array_equal(fb2["forces"], fb1["forces"])
    assert h2["hessian"].shape == (36, 36) and np.array_equal(h2["hessian"], h1["hessian"])
    # single geometries (the base point of get_hessian, get_forces) go graph-parallel over the pool: BASELINE tolerances
    e_orc, f_orc = oracle.energy_forces(z, np.asarray(imgs[0], dtype=np.float32).astype(np.float64))
    f_orc = np.array(f_orc, dtype=np.float64)
    f_orc[1] = 0.0
    for res in (h2, s2):
        assert abs(res["energy"] / U.EV2AU - s1["energy"] / U.EV2AU) <= E_TOL and abs(res["energy"] / U.EV2AU - e_orc) <= E_TOL
        fr = res["forces"].reshape(-1, 3) / U.F_EVAA_2_AU
        assert np.all(fr[1] == 0.0)
        assert np.abs(fr - s1["forces"].reshape(-1, 3) / U.F_EVAA_2_AU).max() <= F_TOL and np.abs(fr - f_orc).max() <= F_TOL


def test_length_mismatch_is_refused_before_any_engine_exists(monkeypatch):
    U = importlib.import_module("pdb2reaction_amd.uma_pysis")
    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,0,0")
    with pytest.raises(ValueError, match=r"0,0,0.*3 device.*workers=2"):
        U.uma_pysis(model="synthetic", workers=2).get_energy(["H", "H"], [0, 0, 0, 0, 0, 1.4])
