"""The strain derivative W = dE/d eps on the GPU (``umx_energy_forces_virial``), through the C ABI and the Python layers above it.

1. The reduction kernels link by link: W against the float64 sum of ``vec_e (x) gvec_e`` over the captured ``evec`` / ``gvec`` of the
   same evaluation, times rmsd, per component within ``(n_terms + 8) 2^-53 rmsd sum|terms|`` -- the rounding of a float64 sum of n
   terms in any order (the host sums exactly, with ``math.fsum``).  No component and no case is left out.
2. W against the float64 checker (tests/stress_oracle.py) in every precision mode and both feed-forward forms.  The yardstick is not
   the engine: it is ``d32``, the deviation of the SAME checker run in float32 from its float64 run on that case, and the bound is
   ``max|dW| <= m d32`` with m per mode the smallest power of two at or above twice the worst ratio measured over the cases
   (profiles/stress.txt records the ratios), capped at 16 for bf16x3 and fp32 and at 64 for the two modes whose reverse products carry
   16 bits (their force error is ~6x the default's).  The grid form's W is not symmetric (tests/test_stress_cpu.py),
   which is what shows a transposed tensor here; rmsd = 1.5 shows a dropped factor; the three-image batch shows a wrong image segment.
3. Bitwise: E and F of the virial entry are those of ``energy_forces``; W does not depend on the batch, the chunking or the lanes; the
   recompute plan gives the stored plan's W, in one piece and in two partitions; the partitioned W is reproducible and meets bound 2.
4. A pool of two engines on one device: a batch bitwise as one engine, a single geometry from engine 0.
5. ``UMXCalculator(stress=True)`` end to end: the Voigt stress is sym(W) / V of the engine.

The input condition of tests/test_gpu_periodic.py (no edge direction in the ambiguous pole band) is asserted for every case held to the
checker.  [3P-UNVERIFIED]: fairchem's own stress has not been compared."""
import importlib
import math

import numpy as np
import pytest
import torch

from periodic_oracle import PeriodicOracle, assert_clear_of_the_pole_band, periodic_radius_graph
from stress_oracle import make_case, strain_derivative, voigt_stress
from pdb2reaction_amd import synth, weights as W

pytestmark = pytest.mark.gpu

# m per precision mode (see 2. above).  Worst ratios max|dW| / d32 measured over the five (form, case) pairs of this file, one MI355X
# (profiles/stress.txt): fp32 0.39, bf16x3 0.53, split-bf16 4.06, split 4.67 -- twice that, rounded up to a power of two:
M_D32 = {"fp32": 1, "bf16x3": 2, "split-bf16": 16, "split": 16}
M_CAP = {"bf16x3": 16, "fp32": 16, "split-bf16": 64, "split": 64}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def new_engine(weights, **kw):
    from pdb2reaction_amd.engine import Engine

    e = Engine(0, **kw)
    e.load_weights(weights)
    return e


@pytest.fixture()
def eng(weights):
    e = new_engine(weights)
    yield e
    e.close()


# ---- 1. the kernels, link by link ----------------------------------------------------------------------------------------------------
def link_check(eng, weights, p32, label):
    """W of every image of the batch against the float64 sum over the image's own range of the captured edges."""
    rmsd = float(np.asarray(weights["normalizer.rmsd"]).reshape(-1)[0])
    assert rmsd == 1.5                                                    # (the synthetic sets: a dropped factor shows)
    p32 = np.asarray(p32, dtype=np.float32)
    k, n = p32.shape[0], p32.shape[1]
    eng.debug_keep(True)
    try:
        e, f, w = eng.energy_forces_virial(p32)
        row_ptr = eng.debug_fetch("row_ptr", np.int32)
        evec = eng.debug_fetch("evec").reshape(-1, 4).astype(np.float64)
        gvec = eng.debug_fetch("gvec").reshape(-1, 4).astype(np.float64)
    finally:
        eng.debug_keep(False)
    assert len(row_ptr) == k * n + 1 and row_ptr[-1] == len(evec) == len(gvec)      # the captures are those of the whole batch
    assert w.shape == (k, 3, 3) and w.dtype == np.float64
    vec = evec[:, :3] * evec[:, 3:4]
    edges = []
    for i in range(k):
        lo, hi = int(row_ptr[i * n]), int(row_ptr[(i + 1) * n])
        edges.append(hi - lo)
        worst = 0.0
        for a in range(3):
            for b in range(3):
                terms = vec[lo:hi, a] * gvec[lo:hi, b]
                host = rmsd * math.fsum(terms)
                bound = (len(terms) + 8) * 2.0 ** -53 * rmsd * float(np.abs(terms).sum())
                d = abs(w[i, a, b] - host)
                worst = max(worst, d / bound if bound > 0 else (0.0 if d == 0 else np.inf))
                assert d <= bound, (label, i, a, b, w[i, a, b], host, bound)
        print(f"[stress link {label} image {i}] {hi - lo} edges  worst |W - host| / bound = {worst:.3f}  W_xx = {w[i, 0, 0]:+.6f} eV")
    return w, edges


@pytest.mark.parametrize("name", ["cubic", "triclinic", "slab"])
def test_link_periodic(eng, weights, name):
    z, p32, cell, pbc = make_case(name)
    eng.set_system(z)
    eng.set_cell(cell, pbc)
    w, edges = link_check(eng, weights, p32, name)
    assert edges[0] > 0 and np.abs(w).max() > 1.0
    if name == "triclinic":
        src, dst, _, _ = periodic_radius_graph(p32[0].astype(np.float64), cell, pbc, W.CUTOFF)
        pairs = np.stack([src.numpy(), dst.numpy()], 1)
        assert (src == dst).any() and len(np.unique(pairs, axis=0)) < len(pairs)      # self-image edges and repeated pairs


@pytest.mark.parametrize("n", [40, 700])
def test_link_open_cluster(eng, weights, n):
    """700 atoms: more than one slab of edges per image; and W = -sum r (x) F to the float32 of the forces."""
    z, pos = synth.make_cluster(n, seed=4)
    eng.set_system(z)
    p32 = pos.astype(np.float32)[None]
    w, edges = link_check(eng, weights, p32, f"cluster {n}")
    assert (edges[0] > 2 * 4096) == (n == 700)
    e, f, _ = eng.energy_forces_virial(p32)
    rf = -(p32[0].astype(np.float64).T @ f[0].astype(np.float64))
    assert np.abs(w[0] - rf).max() <= 1e-4 * max(1.0, np.abs(w[0]).max())


def test_link_truncated_max_neigh(eng, weights):
    z, p32, cell, pbc = make_case("triclinic")
    eng.set_system(z, max_neigh=7)
    eng.set_cell(cell, pbc)
    w, edges = link_check(eng, weights, p32, "triclinic, max_neigh 7")
    assert edges == [7 * len(z)]


def test_link_batch_of_three(eng, weights):
    z, p32, cell, pbc = make_case("cubic", k=3)
    eng.set_system(z)
    eng.set_cell(cell, pbc)
    w, edges = link_check(eng, weights, p32, "cubic x 3")
    assert len(set(edges)) > 1 or not same_bits(w[0], w[1])              # the images differ: a wrong segment cannot pass
    assert not same_bits(w[0], w[1]) and not same_bits(w[1], w[2])


def test_link_images_without_edges(eng, weights):
    z = np.array([8, 1, 1], dtype=np.int32)
    near = np.array([[0.0, 0, 0], [0.96, 0, 0], [-0.3, 0.9, 0]])
    far = near * 30.0                                                        # every distance beyond the cutoff
    eng.set_system(z)
    for batch, label in (([near, far], "water, apart"), ([far, near, far], "apart, water, apart"), ([far], "apart")):
        w, edges = link_check(eng, weights, np.array(batch, dtype=np.float32), label)
        for i, ne in enumerate(edges):
            assert (ne == 0) == (batch[i] is far)
            if ne == 0:
                assert same_bits(w[i], np.zeros((3, 3)))
    assert same_bits(eng.energy_forces_virial(np.array([near, far], dtype=np.float32))[2][0], eng.energy_forces_virial(near.astype(np.float32))[2][0])


# ---- 2. against the float64 checker ----------------------------------------------------------------------------------------------------
_ref = {}


def reference(ff, name):
    """(z, p32, cell, pbc, W64, d32) of a case: the checker in float64 and its own float32 deviation, once per session."""
    if (ff, name) not in _ref:
        w = W.make_synthetic_weights(0, **({"ff_type": "grid"} if ff == "grid" else {}))
        z, p32, cell, pbc = make_case(name)
        orc = PeriodicOracle(w, cell=cell, pbc=pbc)
        p64 = p32[0].astype(np.float64)
        graph = periodic_radius_graph(p64, orc.cell, orc.pbc, orc.cutoff, orc.max_neigh)
        assert_clear_of_the_pole_band(p64[graph[0].numpy()] + graph[2].numpy() - p64[graph[1].numpy()])
        torch.set_num_threads(16)
        w64 = strain_derivative(orc, z, p64, graph=graph)
        d32 = float(np.abs(strain_derivative(orc, z, p64, torch.float32, graph=graph) - w64).max())
        _ref[(ff, name)] = (z, p32, cell, pbc, w64, d32)
    return _ref[(ff, name)]


FF_CASES = {"spectral": ("triclinic", "cubic", "slab"), "grid": ("triclinic", "slab")}


def oracle_check(eng, ff, name, mode, label):
    z, p32, cell, pbc, w64, d32 = reference(ff, name)
    eng.set_system(z)
    eng.set_cell(cell, pbc)
    w = eng.energy_forces_virial(p32)[2][0]
    dw = float(np.abs(w - w64).max())
    print(f"[stress oracle {label} {ff} {name} {mode}] max|dW| = {dw:.3e} eV  d32 = {d32:.3e} eV  ratio = {dw / d32:.2f}  (m = {M_D32[mode]})  "
          f"asymmetry {np.abs(w - w.T).max():.3e} / {np.abs(w64 - w64.T).max():.3e}")
    return dw / d32


@pytest.mark.parametrize("ff", ["spectral", "grid"])
@pytest.mark.parametrize("mode", ["fp32", "split", "split-bf16", "bf16x3"])
def test_virial_against_the_float64_checker(mode, ff):
    assert M_D32[mode] <= M_CAP[mode]
    w = W.make_synthetic_weights(0, **({"ff_type": "grid"} if ff == "grid" else {}))
    e = new_engine(w, precision=mode)
    try:
        ratios = {name: oracle_check(e, ff, name, mode, "one piece") for name in FF_CASES[ff]}
    finally:
        e.close()
    assert max(ratios.values()) <= M_D32[mode], (mode, ff, ratios)


# ---- 3. bitwise ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cubic", "triclinic"])
def test_energy_and_forces_are_those_of_energy_forces(eng, name):
    z, p32, cell, pbc = make_case(name, k=3)
    eng.set_system(z)
    eng.set_cell(cell, pbc)
    e0, f0 = eng.energy_forces(p32)
    e1, f1, w1 = eng.energy_forces_virial(p32)
    e2, f2 = eng.energy_forces(p32)
    assert same_bits(e1, e0) and same_bits(f1, f0) and same_bits(e2, e0) and same_bits(f2, f0)
    eng.set_cell(None)                                                      # and without a cell
    e0, f0 = eng.energy_forces(p32)
    e1, f1, w1 = eng.energy_forces_virial(p32)
    assert same_bits(e1, e0) and same_bits(f1, f0) and np.isfinite(w1).all()


def test_device_pointer_entry_is_the_host_entry(weights):
    """``umx_energy_forces_virial_dev`` with the caller's buffers: on a torch stream of its own (a fresh engine: the partial buffer grows
    while work is ordered on the caller's stream), again with more images (it grows again), and on the legacy default stream 0."""
    dev = torch.device("cuda", 0)
    z, p32, cell, pbc = make_case("cubic", k=4)
    host = new_engine(weights)
    e_ = new_engine(weights)
    try:
        for en in (host, e_):
            en.set_system(z)
            en.set_cell(cell, pbc)
        e0, f0, w0 = host.energy_forces_virial(p32)
        side = torch.cuda.Stream(device=dev)
        for k, stream in ((2, side), (4, side), (4, None)):
            with torch.cuda.stream(side if stream is not None else torch.cuda.default_stream(dev)):
                pos = torch.from_numpy(p32[:k]).to(dev)
                e_t = torch.full((k,), float("nan"), dtype=torch.float64, device=dev)
                f_t = torch.full((k, len(z), 3), float("nan"), dtype=torch.float32, device=dev)
                w_t = torch.full((k, 9), float("nan"), dtype=torch.float64, device=dev)
                e_.energy_forces_virial_dev(k, pos.data_ptr(), e_t.data_ptr(), f_t.data_ptr(), w_t.data_ptr(),
                                            stream=side.cuda_stream if stream is not None else 0)
                # consumers on the same stream need no further synchronisation
                e1, f1, w1 = e_t.cpu().numpy(), f_t.cpu().numpy(), w_t.cpu().numpy().reshape(k, 3, 3)
            e_.synchronize()
            assert same_bits(w1, w0[:k]) and same_bits(e1, e0[:k]) and same_bits(f1, f0[:k]), (k, stream is not None)
        # without a virial buffer the entry is umx_energy_forces_dev
        e_t.fill_(float("nan")); f_t.fill_(float("nan"))
        torch.cuda.synchronize(dev)
        e_.energy_forces_virial_dev(4, pos.data_ptr(), e_t.data_ptr(), f_t.data_ptr(), 0, stream=0)
        e_.synchronize()
        assert same_bits(e_t.cpu().numpy(), e0) and same_bits(f_t.cpu().numpy(), f0)
    finally:
        e_.close()
        host.close()


def test_virial_without_forces_is_refused(eng):
    import ctypes as C
    from pdb2reaction_amd.engine import UMX_ERR_RANGE  # noqa: F401  (the status codes live next to it)

    z, p32, cell, pbc = make_case("triclinic")
    eng.set_system(z)
    e, w = np.empty(1), np.empty(9)
    st = eng.lib.umx_energy_forces_virial(eng._h, 1, p32.ctypes.data_as(C.POINTER(C.c_float)), e.ctypes.data_as(C.POINTER(C.c_double)), None,
                                          w.ctypes.data_as(C.POINTER(C.c_double)))
    assert st == -1 and b"forces" in eng.lib.umx_last_error(eng._h)          # UMX_ERR_ARG


def test_virial_does_not_depend_on_batch_chunks_or_lanes(weights, monkeypatch):
    z, p32, cell, pbc = make_case("cubic", k=4)

    def run(env, expect_lanes):
        for k_, v in env.items():
            monkeypatch.setenv(k_, v)
        e_ = new_engine(weights)
        try:
            e_.set_system(z)
            e_.set_cell(cell, pbc)
            out = e_.energy_forces_virial(p32)
            assert e_.last_lanes() == expect_lanes and e_.last_partitions() == 0
            return out
        finally:
            e_.close()
            for k_ in env:
                monkeypatch.delenv(k_)

    e0, f0, w0 = run({}, 1)
    base = new_engine(weights)
    try:
        base.set_system(z)
        base.set_cell(cell, pbc)
        for k in range(len(p32)):
            e1, f1, w1 = base.energy_forces_virial(p32[k])
            assert same_bits(w1[0], w0[k]) and e1[0] == e0[k] and same_bits(f1[0], f0[k]), k
        assert same_bits(base.energy_forces_virial(p32[::-1].copy())[2], w0[::-1].copy())       # another position in the batch
    finally:
        base.close()
    for env, lanes in (({"UMX_MAX_CHUNK_IMAGES": "1"}, 1), ({"UMX_STREAMS": "2"}, 2), ({"UMX_STREAMS": "2", "UMX_MAX_CHUNK_IMAGES": "1"}, 2)):
        e1, f1, w1 = run(env, lanes)
        assert same_bits(w1, w0) and same_bits(e1, e0) and same_bits(f1, f0), env


@pytest.mark.parametrize("parts", [0, 2])
def test_recompute_plans_and_partitions(weights, parts, monkeypatch):
    """Mode 2 against the stored plan, bitwise, in one piece and in two partitions; the partitioned W is reproducible run to run and
    meets the checker's bound of the default mode (its sum runs partition by partition: not the bits of the plan in one piece)."""
    if parts:
        monkeypatch.setenv("UMX_FORCE_PARTS", str(parts))
    stored, replay = new_engine(weights, recompute=0), new_engine(weights, recompute=2)
    try:
        for name in ("triclinic", "cubic"):
            z, p32, cell, pbc = make_case(name, k=2)
            for e_ in (stored, replay):
                e_.set_system(z)
                e_.set_cell(cell, pbc)
            e0, f0, w0 = stored.energy_forces_virial(p32)
            e1, f1, w1 = replay.energy_forces_virial(p32)
            assert stored.last_partitions() == parts and replay.last_partitions() == parts
            assert stored.last_recompute() == 0 and replay.last_recompute() == 1
            assert same_bits(w1, w0) and same_bits(e1, e0) and same_bits(f1, f0), (name, parts)
            e2, f2, w2 = stored.energy_forces_virial(p32)
            assert same_bits(w2, w0) and same_bits(f2, f0), (name, parts)
            ef = stored.energy_forces(p32)
            assert same_bits(ef[0], e0) and same_bits(ef[1], f0)
            if parts:
                ratio = oracle_check(stored, "spectral", name, "bf16x3", f"{parts} partitions")
                assert ratio <= M_D32["bf16x3"], (name, ratio)
                assert same_bits(stored.energy_forces_virial(reference("spectral", name)[1])[2][0], w0[0])
    finally:
        stored.close()
        replay.close()


# ---- 4. the pool, 5. the facade --------------------------------------------------------------------------------------------------------
class _Atoms:
    def __init__(self, z, pos, cell, pbc):
        self.numbers, self._pos, self.cell, self.pbc, self.info = z, np.asarray(pos, dtype=np.float64), cell, pbc, {}

    def get_positions(self):
        return self._pos


def test_a_pool_of_two_engines_on_one_device(eng, monkeypatch):
    A = importlib.import_module("pdb2reaction_amd.ase_calculator")
    z, p32, cell, pbc = make_case("triclinic", k=5)
    eng.set_system(z)
    eng.set_cell(cell, pbc)
    e0, f0, w0 = eng.energy_forces_virial(p32)
    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,0")
    two = A.UMXCalculator(model="synthetic", workers=2, stress=True)
    try:
        images = [_Atoms(z, p, cell, pbc) for p in p32]
        e2, f2, s2 = two.calculate_images(images, stress=True)
        pool = two._engine
        assert two.local_devices == [0, 0] and len(pool) == 2 and pool.last_route == "batch"
        assert same_bits(e2, e0) and same_bits(f2, f0.astype(np.float64))
        e3, f3, w3 = pool.energy_forces_virial(p32)
        assert same_bits(w3, w0) and same_bits(e3, e0) and same_bits(f3, f0)
        assert same_bits(s2, np.stack([voigt_stress(w, cell) for w in w0]))
        e4, f4, w4 = pool.energy_forces_virial(p32[3])                       # one geometry: engine 0 alone, not graph-parallel
        assert pool.last_route == "single" and same_bits(w4[0], w0[3]) and e4[0] == e0[3] and same_bits(f4[0], f0[3])
        two.calculate(images[3], ["energy", "forces", "stress"])
        assert pool.last_route == "single" and same_bits(two.results["stress"], voigt_stress(w0[3], cell))
    finally:
        two.close()


def test_the_facade_end_to_end(eng, monkeypatch):
    A = importlib.import_module("pdb2reaction_amd.ase_calculator")
    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    z, p32, cell, pbc = make_case("cubic")
    eng.set_system(z)
    eng.set_cell(cell, pbc)
    e0, f0, w0 = eng.energy_forces_virial(p32)
    e1, f1, s1 = eng.energy_forces_stress(p32)
    assert same_bits(s1[0], voigt_stress(w0[0], cell)) and same_bits(e1, e0) and same_bits(f1, f0)
    calc = A.UMXCalculator(model="synthetic", stress=True)
    try:
        at = _Atoms(z, p32[0], cell, pbc)
        s = calc.get_stress(at)
        assert calc.get_potential_energy(at) == e0[0] and same_bits(calc.get_forces(at), f0[0].astype(np.float64))
        assert s.shape == (6,) and same_bits(s, voigt_stress(w0[0], cell))
        assert abs(s[0] - 0.5 * (w0[0, 0, 0] + w0[0, 0, 0]) / 14.0 ** 3) <= 1e-15 and abs(s[3] - 0.5 * (w0[0, 1, 2] + w0[0, 2, 1]) / 14.0 ** 3) <= 1e-15
        slab = _Atoms(z, p32[0], cell, (True, True, False))
        assert np.isfinite(calc.get_potential_energy(slab))
        with pytest.raises(A.PropertyNotImplementedError):
            calc.get_stress(slab)
    finally:
        calc.close()
    with pytest.raises(ValueError, match="periodic along all three"):
        eng.set_cell(cell, (True, True, False))
        eng.energy_forces_stress(p32)
