"""Float64 positions on the GPU (``umx_energy_forces_f64[_dev]``), through the C ABI and the Python layers above it.

With ``double_positions=True`` the radius-graph kernels form every edge vector as the float64 difference ``r_j + t - r_i`` and round
it ONCE to float32; from that rounded vector on the arithmetic is the float entries'.  Two exact statements follow, and both are
asserted bit for bit on E (float64), F (float32) and W (float64):

1. open boundaries, coordinates quantised to multiples of 2^-20 A with |x| < 16 A (every coordinate is a float32, every difference
   fits float64 exactly, and IEEE float32 subtraction IS the exact difference rounded once): the double entry gives the bits of the
   float entry -- in one piece, in two partitions, with the recompute plan, on two lanes and with ``max_neigh`` binding;
2. the rigid translation T = (1024, -2048, 512) A is exact in float64 (x + T needs 32 bits) and leaves every float64 difference the
   same real number: the double entry at x + T gives the bits of 1.  The float entry at x + T is evaluated and printed only.

On top: the double entry at x + T against the float64 checker evaluated at the float64 x + T (|dE| <= 1e-4 eV, max|dF| <= 1e-3 eV/A,
include/umx.h); periodic cells (tests/cells_cases.py) translated by 200 a + 300 b - 150 c plus an incommensurate offset against the
periodic checker at that float64 geometry, with the virial rule of tests/test_gpu_stress.py; the finite-difference Hessian at x + T
against the one at x; refusals and defaults.  Shapes: 14 atoms (one partial block of 64 sources), 70 atoms (two blocks, the second
partial), K = 1 and K = 3 images.

The virial rule's yardstick d32 (the checker's own float32 deviation) is taken at the UNTRANSLATED geometry: W does not depend on the
frame, the checker in float32 does, and at 1000 A its deviation would widen the bound -- the frame where float32 loses least gives
the bound the existing stress tests use."""
import importlib

import numpy as np
import pytest
import torch

from cells_cases import assert_image_is_clear, family
from periodic_oracle import PeriodicOracle, assert_clear_of_the_pole_band
from stress_oracle import strain_derivative
from test_gpu_cells import M_D32, same_bits, same_efw
from test_gpu_periodic import TOL_E, TOL_F
from pdb2reaction_amd import synth, weights as W

pytestmark = pytest.mark.gpu

T = np.array([1024.0, -2048.0, 512.0])
Q = 2.0 ** -20


def quantised(n, k):
    """(z, x float64 [k,n,3]): a synthetic string, every coordinate a multiple of 2^-20 A with |x| < 16 A."""
    z, imgs, _ = synth.make_images(n, k, seed=21)
    x = np.round(imgs / Q) * Q
    assert np.abs(x).max() < 16.0 and same_bits(x.astype(np.float32).astype(np.float64), x)
    assert same_bits((x + T) - T, x)                                         # x + T is exact in float64
    return z, x


def symbols(z):
    return [next(s for s, v in synth.Z_OF_SYMBOL.items() if v == int(a)) for a in z]


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


def efw_max(a, b):
    return abs(a[0] - b[0]).max(), float(np.abs(a[1].astype(np.float64) - b[1]).max()), float(np.abs(a[2] - b[2]).max())


# ---- 1. same bits where nothing should differ, 2. translation invariance -----------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(14, 1), (14, 3), (70, 1), (70, 3)])
def test_same_bits_at_the_origin_and_under_translation(eng, n, k):
    z, x = quantised(n, k)
    eng.set_system(z)
    f32 = eng.energy_forces_virial(x.astype(np.float32))
    assert eng.graph_stats()[0] > 0 and np.abs(f32[2]).max() > 0
    f64 = eng.energy_forces_virial(x, double_positions=True)
    assert same_efw(f64, f32), (n, k, efw_max(f64, f32))
    moved = eng.energy_forces_virial(x + T, double_positions=True)
    assert same_efw(moved, f32), (n, k, efw_max(moved, f32))
    ef = eng.energy_forces(x + T, double_positions=True)                      # the entry without a virial
    assert same_bits(ef[0], f32[0]) and same_bits(ef[1], f32[1])
    e_only = eng.energy_forces(x + T, forces=False, double_positions=True)
    assert e_only[1] is None and np.abs(e_only[0] - f32[0]).max() <= TOL_E
    old = eng.energy_forces_virial((x + T).astype(np.float32))               # the old behaviour: printed, not asserted
    de, df, dw = efw_max(old, f32)
    print(f"[double positions n={n} k={k}] float32 entry at x + T against x: |dE| = {de:.3e} eV  max|dF| = {df:.3e} eV/A  max|dW| = {dw:.3e} eV")


# (two lanes need two chunks, hence more than one image: K = 1 runs the other two settings only)
@pytest.mark.parametrize("setting,k", [("parts2", 1), ("parts2", 3), ("recompute2", 1), ("recompute2", 3), ("streams2", 3)])
@pytest.mark.parametrize("n", [14, 70])
def test_same_bits_in_partitions_recompute_and_lanes(weights, monkeypatch, setting, k, n):
    z, x = quantised(n, k)
    if setting == "parts2":
        monkeypatch.setenv("UMX_FORCE_PARTS", "2")
    if setting == "streams2":
        monkeypatch.setenv("UMX_STREAMS", "2")
    e_ = new_engine(weights, **({"recompute": 2} if setting == "recompute2" else {}))
    try:
        e_.set_system(z)
        f32 = e_.energy_forces_virial(x.astype(np.float32))
        for p in (x, x + T):
            f64 = e_.energy_forces_virial(p, double_positions=True)
            assert e_.last_partitions() == (2 if setting == "parts2" else 0)
            assert e_.last_recompute() == (1 if setting == "recompute2" else 0)
            assert e_.last_lanes() == (2 if setting == "streams2" else 1)
            assert same_efw(f64, f32), (setting, n, k, efw_max(f64, f32))
    finally:
        e_.close()


@pytest.mark.parametrize("n", [14, 70])
def test_same_bits_with_max_neigh_binding(eng, n):
    """The truncating fill: every atom has more than 7 candidates, the 7 nearest by (d^2, source) are kept."""
    z, x = quantised(n, 3)
    eng.set_system(z, max_neigh=7)
    f32 = eng.energy_forces_virial(x.astype(np.float32))
    assert eng.graph_stats() == (3 * 7 * n, 7)
    f64 = eng.energy_forces_virial(x, double_positions=True)
    assert eng.graph_stats() == (3 * 7 * n, 7) and same_efw(f64, f32)
    assert same_efw(eng.energy_forces_virial(x + T, double_positions=True), f32)
    eng.set_system(z)
    assert not same_bits(eng.energy_forces_virial(x, double_positions=True)[0], f32[0])     # the cap did bind


# ---- 3. against the float64 checker at the shifted frame ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [14, 70])
def test_the_shifted_frame_matches_the_float64_oracle(eng, oracle, n):
    z, x = quantised(n, 1)
    p = x[0] + T
    d = p[:, None, :] - p[None, :, :]
    r = np.linalg.norm(d, axis=-1)
    assert_clear_of_the_pole_band(d[(r > 0) & (r <= W.CUTOFF)])
    eng.set_system(z)
    e, f = eng.energy_forces(p, double_positions=True)
    e_ref, f_ref = oracle.energy_forces(z, p)                                # float64, no cast
    de, df = abs(e[0] - e_ref), float(np.abs(f[0] - f_ref).max())
    e32, f32 = eng.energy_forces(p.astype(np.float32))
    print(f"[double positions oracle n={n}] at x + T: |dE| = {de:.3e} eV  max|dF| = {df:.3e} eV/A   "
          f"(float32 entry: |dE| = {abs(e32[0] - e_ref):.3e} eV  max|dF| = {np.abs(f32[0] - f_ref).max():.3e} eV/A)")
    assert de <= TOL_E, (n, e[0], e_ref)
    assert df <= TOL_F, (n, df)


# ---- 4. periodic -----------------------------------------------------------------------------------------------------------------------------
PICK = {"triclinic": [0, 1, 2], "slab": [0, 1, 0]}                          # K = 3 images, each in its own cell
OFFSET = np.array([0.1234567891, -0.2345678912, 0.3456789123])
_moved, _graphs, _batch = {}, {}, {}


def moved_family(name):
    """(z, p32, p64 [3,N,3], cells, pbc): the family's images, each translated by 200 a + 300 b - 150 c of ITS cell plus OFFSET, in
    float64.  EVERY image passes ``assert_image_is_clear`` at that translated float64 geometry (its graphs are kept for the checker)."""
    if name not in _moved:
        z, p32, cells, pbc = family(name, PICK[name])
        shift = 200.0 * cells[:, 0] + 300.0 * cells[:, 1] - 150.0 * cells[:, 2] + OFFSET
        p64 = p32.astype(np.float64) + shift[:, None, :]
        _graphs[name] = [assert_image_is_clear(p64[k], cells[k], pbc) for k in range(len(p64))]
        _moved[name] = (z, p32, p64, cells, pbc)
    return _moved[name]


def moved_batch(weights, name):
    """E, F, W of the translated family in one per-image-cell call with double positions, the singles, and the mode; once per session."""
    if name not in _batch:
        z, p32, p64, cells, pbc = moved_family(name)
        e_ = new_engine(weights)
        try:
            e_.set_system(z)
            e_.set_cells(cells, pbc)
            batch = e_.energy_forces_virial(p64, double_positions=True)
            singles = []
            for k in range(len(p64)):
                e_.set_cell(cells[k], pbc)
                singles.append(e_.energy_forces_virial(p64[k], double_positions=True))
            _batch[name] = (batch, singles, e_.precision_mode())
        finally:
            e_.close()
    return _batch[name]


@pytest.mark.parametrize("name", ["triclinic", "slab"])
def test_periodic_image_k_is_the_single_evaluation_in_cell_k(weights, name):
    batch, singles, _ = moved_batch(weights, name)
    for k, one in enumerate(singles):
        assert same_efw([x[k:k + 1] for x in batch], one), (name, k)
    assert not same_bits(batch[0][0], batch[0][1])                           # the images differ: a wrong cell cannot pass


# (the other images of the two batches are held to these through the bitwise test above; the checker costs seconds per image.  All of
# them, compared with the checker or not, have passed assert_image_is_clear in moved_family.)
@pytest.mark.parametrize("name,k", [("triclinic", 0), ("triclinic", 2), ("slab", 0)])
def test_periodic_translated_images_match_the_periodic_oracle(weights, name, k):
    z, p32, p64, cells, pbc = moved_family(name)
    (e, f, w), _, mode = moved_batch(weights, name)
    torch.set_num_threads(16)
    orc = PeriodicOracle(weights, cell=cells[k], pbc=pbc)
    graph = _graphs[name][k]                                                 # of assert_image_is_clear(p64[k], ...), in moved_family
    e_ref, f_ref = orc.energy_forces(z, p64[k])
    de, df = abs(e[k] - e_ref), float(np.abs(f[k] - f_ref).max())
    w64 = strain_derivative(orc, z, p64[k], graph=graph)
    g0 = assert_image_is_clear(p32[k], cells[k], pbc)                        # d32 at the untranslated frame (see the module docstring)
    x0 = p32[k].astype(np.float64)
    d32 = float(np.abs(strain_derivative(orc, z, x0, torch.float32, graph=g0) - strain_derivative(orc, z, x0, graph=g0)).max())
    dw = float(np.abs(w[k] - w64).max())
    print(f"[double positions periodic {name} image {k} {mode}] |dE| = {de:.3e} eV  max|dF| = {df:.3e} eV/A  max|dW| = {dw:.3e} eV  "
          f"d32 = {d32:.3e} eV  ratio = {dw / d32:.2f}  (m = {M_D32[mode]})")
    assert de <= TOL_E, (name, k, e[k], e_ref)
    assert df <= TOL_F, (name, k, df)
    assert dw <= M_D32[mode] * d32, (name, k, dw, d32)


# ---- 5. the finite-difference Hessian -------------------------------------------------------------------------------------------------------
def test_fd_hessian_does_not_depend_on_the_frame(monkeypatch):
    """D = max|H64(x + T) - H64(x)| <= D0 = max|H32(x) - H64(x)|, on the device path and on the host path of ``hessian.fd_hessian``
    (H64: ``uma_pysis(double_positions=True)``, H32: the default).  D0 is what float32 positions cost at the frame where they lose
    least; max|H32(x + T) - H64(x)| is printed."""
    U = importlib.import_module("pdb2reaction_amd.uma_pysis")
    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    z, x = quantised(14, 1)
    elem = symbols(z)
    at_x, at_xt = (x[0] * U.ANG2BOHR).reshape(-1), ((x[0] + T) * U.ANG2BOHR).reshape(-1)
    c64 = U.uma_pysis(model="synthetic", out_hess_torch=False, double_positions=True)
    c32 = U.uma_pysis(model="synthetic", out_hess_torch=False)
    try:
        for path in ("device", "host"):
            if path == "host":
                monkeypatch.delattr(U.UMAcore, "compute_batch_dev")          # fd_hessian then takes the host form
            h64, h64t = c64.get_hessian(elem, at_x)["hessian"], c64.get_hessian(elem, at_xt)["hessian"]
            h32, h32t = c32.get_hessian(elem, at_x)["hessian"], c32.get_hessian(elem, at_xt)["hessian"]
            assert h64.shape == (42, 42) and h64.dtype == np.float64 and np.abs(h64).max() > 0
            d, d0, dt = float(np.abs(h64t - h64).max()), float(np.abs(h32 - h64).max()), float(np.abs(h32t - h64).max())
            print(f"[double positions hessian {path}] D = max|H64(x+T) - H64(x)| = {d:.3e}  D0 = max|H32(x) - H64(x)| = {d0:.3e}  "
                  f"max|H32(x+T) - H64(x)| = {dt:.3e}  Hartree/Bohr^2   (max|H| = {np.abs(h64).max():.3e})")
            assert d <= d0, (path, d, d0)
    finally:
        c64.close()
        c32.close()


# ---- 6. refusals and defaults ------------------------------------------------------------------------------------------------------------------
def test_a_nan_coordinate_is_refused_as_on_the_float_path(eng):
    from pdb2reaction_amd.engine import UmxError

    z, x = quantised(14, 3)
    eng.set_system(z)
    good = eng.energy_forces(x, double_positions=True)
    bad = x.copy()
    bad[1, 7, 2] = np.nan
    for kw in ({}, {"double_positions": True}):
        with pytest.raises(UmxError, match=r"non-finite position \(image 1\)") as ei:
            eng.energy_forces(bad, **kw)
        assert ei.value.status == -1
    dev = torch.device("cuda", 0)
    e_t = torch.zeros(3, dtype=torch.float64, device=dev)
    f_t = torch.zeros(3, 14, 3, dtype=torch.float32, device=dev)
    pos = torch.from_numpy(bad).to(dev)
    torch.cuda.synchronize(dev)
    with pytest.raises(UmxError, match=r"non-finite position \(device buffer\)") as ei:      # status bit 2, set by the graph kernel
        eng.energy_forces_dev(3, pos.data_ptr(), e_t.data_ptr(), f_t.data_ptr(), double_positions=True)
    assert ei.value.status == -1 and eng.take_range_error() is False
    pos = torch.from_numpy(x).to(dev)                                        # and the engine goes on: the device entry gives the host entry's bits
    torch.cuda.synchronize(dev)
    eng.energy_forces_dev(3, pos.data_ptr(), e_t.data_ptr(), f_t.data_ptr(), double_positions=True)
    eng.synchronize()
    assert same_bits(e_t.cpu().numpy(), good[0]) and same_bits(f_t.cpu().numpy(), good[1])


def test_the_flag_off_is_the_cast_to_float32(eng):
    z, x = quantised(14, 3)
    y = x + T + 1.0e-7                                                       # float64 values that are no float32
    eng.set_system(z)
    assert same_efw(eng.energy_forces_virial(y), eng.energy_forces_virial(y.astype(np.float32)))
    a, b = eng.energy_forces(y), eng.energy_forces(y.astype(np.float32))
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    assert not same_bits(eng.energy_forces(y, double_positions=True)[0], a[0])


def test_the_pool_takes_the_flag_and_refuses_graph_parallel(weights):
    from pdb2reaction_amd.parallel import LocalEnginePool

    z, x = quantised(14, 3)
    one = new_engine(weights)
    try:
        one.set_system(z)
        want = one.energy_forces_virial(x + T, double_positions=True)
    finally:
        one.close()
    with LocalEnginePool.create([0, 0], weights) as pool:
        pool.set_system(z)
        assert same_efw(pool.energy_forces_virial(x + T, double_positions=True), want) and pool.last_route == "batch"
        e, f = pool.energy_forces(x[1] + T, double_positions=True)           # one geometry: engine 0 alone
        assert pool.last_route == "single" and same_bits(e, want[0][1:2]) and same_bits(f, want[1][1:2])
        with pytest.raises(ValueError, match="float32 positions only"):
            pool.energy_forces_virial(x[1] + T, graph_parallel=True, double_positions=True)
        with pytest.raises(ValueError, match="float32 positions only"):
            pool.energy_forces_stress(x[1] + T, graph_parallel=True, double_positions=True)


def test_the_device_entry_holds_the_tensor_to_the_flag(monkeypatch):
    U = importlib.import_module("pdb2reaction_amd.uma_pysis")
    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    z, x = quantised(14, 3)
    elem = symbols(z)
    dev = torch.device("cuda", 0)
    p64 = torch.from_numpy(x + T).to(dev)
    for flag in (True, False):
        core = U.UMAcore(elem, model="synthetic", double_positions=flag)
        try:
            ok, wrong = (p64, p64.to(torch.float32)) if flag else (p64.to(torch.float32), p64)
            with pytest.raises(TypeError, match="double_positions"):
                core.compute_batch_dev(wrong)
            f = core.compute_batch_dev(ok)
            torch.cuda.synchronize(dev)
            want = core.compute_batch((x + T), forces=True)["forces"]
            assert f.dtype == torch.float32 and same_bits(f.cpu().numpy(), want)
        finally:
            core.close()


def test_the_facade_forwards_the_flag(eng, monkeypatch):
    A = importlib.import_module("pdb2reaction_amd.ase_calculator")
    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    z, p32, p64, cells, pbc = moved_family("triclinic")

    class Atoms:
        def __init__(self, pos, cell):
            self.numbers, self._pos, self.cell, self.pbc, self.info = z, pos, cell, pbc, {}

        def get_positions(self):
            return self._pos

    eng.set_system(z)
    eng.set_cells(cells, pbc)
    e0, f0, s0 = eng.energy_forces_stress(p64, double_positions=True)
    eng.set_cell(cells[1], pbc)
    e1, f1, s1 = eng.energy_forces_stress(p64[1], double_positions=True)
    calc = A.UMXCalculator(model="synthetic", stress=True, double_positions=True)
    try:
        images = [Atoms(p, c) for p, c in zip(p64, cells)]
        e, f, s = calc.calculate_images(images, stress=True, per_image_cells=True)
        assert same_bits(e, e0) and same_bits(f, f0.astype(np.float64)) and same_bits(s, s0)
        e, f = calc.calculate_images(images, per_image_cells=True)
        assert same_bits(e, e0) and same_bits(f, f0.astype(np.float64))
        assert calc.get_potential_energy(images[1]) == e1[0] and same_bits(calc.get_stress(images[1]), s1[0])
        assert same_bits(calc.get_forces(images[1]), f1[0].astype(np.float64))
    finally:
        calc.close()
