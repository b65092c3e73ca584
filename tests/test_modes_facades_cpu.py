"""The facades of the lowest-modes solver without a GPU: ``uma_pysis.get_lowest_modes`` -- units, signed wavenumbers, ``freeze_atoms``,
the masses ``ValueError``, the graph-parallel refusal -- on the toy core of tests/toy_core.py (wrapped as tests/test_hvp_cpu.py wraps it,
not edited), ``UMXCalculator.lowest_modes`` on a stand-in, the ``hei_modes`` key of ``optimize_path_gsm`` and the pool's dealing."""
import importlib
import types

import numpy as np
import pytest

import modes_cases as MC
from test_hvp_cpu import BOHR_IN_ANG, EV_A2_TO_AU, QuadCore
from toy_core import toy_geometry
from pdb2reaction_amd import modes as M

U = importlib.import_module("pdb2reaction_amd.uma_pysis")
MASSES = np.array([12.011, 1.008, 15.999, 14.007])


class ModesCore(QuadCore):
    """The toy core with K made a proper Hessian -- symmetric, one negative eigenvalue -- and ``UMAcore.lowest_modes``'s contract over
    its own ``hvp`` through the host backend."""

    def __init__(self, n):
        super().__init__(n)
        rng = np.random.default_rng(8)
        q, _ = np.linalg.qr(rng.standard_normal((3 * n, 3 * n)))
        self.K = (q * np.concatenate([[-3.0], rng.uniform(1.0, 30.0, 3 * n - 1)])) @ q.T
        self.K = 0.5 * (self.K + self.K.T)
        self.modes_calls = []

    def lowest_modes(self, coord_ang, masses_amu, k=1, **kw):
        self.modes_calls.append((np.array(coord_ang), np.array(masses_amu), k, dict(kw)))
        return M.lowest_modes(M.HostBackend(lambda b, d, step=1e-3, scheme="central": self.hvp(b, d, step=step, scheme=scheme)),
                              coord_ang, masses_amu, k, **kw)


def calc_on(core, **kw):
    calc = U.uma_pysis(model="synthetic", **kw)
    calc._core = core
    return calc


def test_get_lowest_modes_units_signs_and_keys():
    n = 4
    elem = ["C", "H", "O", "N"]
    x_ang = toy_geometry(n)
    core = ModesCore(n)
    calc = calc_on(core)
    out = calc.get_lowest_modes(elem, (x_ang / BOHR_IN_ANG).reshape(-1), 2, MASSES, project="none", tol=1e-10 * EV_A2_TO_AU)
    assert set(out) == {"freqs_cm", "eigenvalues", "modes", "converged", "residuals", "images"}
    lam, vec, _, _ = MC.dense_reference(core.K, x_ang, MASSES, project="none")       # eV/A^2/amu
    assert out["converged"].all() and out["modes"].shape == (2, 3 * n) and isinstance(out["images"], int) and out["images"] > 0
    # 1 eV/A^2 = (1 / 27.2114 Hartree) x (0.529177 A/Bohr)^2, constants written out by hand in tests/test_hvp_cpu.py
    assert np.abs(out["eigenvalues"] / (lam[:2] * EV_A2_TO_AU) - 1.0).max() < 1e-8
    assert (out["residuals"] <= 1e-10 * EV_A2_TO_AU * (1.0 + 1e-8)).all()
    assert lam[0] < 0.0 < lam[1] and out["freqs_cm"][0] < 0.0 < out["freqs_cm"][1]   # signed: the imaginary one is negative
    assert np.abs(out["freqs_cm"] / (np.sign(lam[:2]) * np.sqrt(np.abs(lam[:2])) * 521.47) - 1.0).max() < 1e-5
    # the Cartesian convention: w * u normalised
    w = MC.weights_vector(MASSES)
    for m_out, u in zip(out["modes"], vec[:2]):
        cart = w * u / np.linalg.norm(w * u)
        assert min(np.abs(m_out - cart).max(), np.abs(m_out + cart).max()) < 1e-7
    pos, masses, k, kw = core.modes_calls[-1]
    assert np.abs(pos - x_ang).max() < 1e-8 and np.array_equal(masses, MASSES) and k == 2
    assert kw["step"] == 1e-3 and kw["scheme"] == "central" and kw["frozen"] == () and abs(kw["tol"] / 1e-10 - 1.0) < 1e-8
    assert core.hvp_calls[-1][2] == 1e-3                                    # step_bohr=None: 1e-3 A reaches the products
    calc.get_lowest_modes(elem, x_ang / BOHR_IN_ANG, 1, MASSES, project="none", step_bohr=0.01, scheme="forward")
    assert abs(core.hvp_calls[-1][2] / (0.01 * BOHR_IN_ANG) - 1.0) < 1e-8 and core.hvp_calls[-1][3] == "forward"
    assert core.modes_calls[-1][3]["tol"] is None                            # tol=None: the solver's default


def test_freeze_atoms_the_masses_error_and_the_graph_parallel_refusal():
    n = 4
    elem = ["C", "H", "O", "N"]
    x_ang = toy_geometry(n)
    x_bohr = (x_ang / BOHR_IN_ANG).reshape(-1)
    core = ModesCore(n)
    frozen = calc_on(core, freeze_atoms=[1])
    out = frozen.get_lowest_modes(elem, x_bohr, 2, MASSES, project="none", tol=1e-10 * EV_A2_TO_AU)
    lam, _, _, _ = MC.dense_reference(core.K, x_ang, MASSES, frozen=[1], project="none")
    assert core.modes_calls[-1][3]["frozen"] == (1,)
    assert out["converged"].all() and np.abs(out["eigenvalues"] / (lam[:2] * EV_A2_TO_AU) - 1.0).max() < 1e-8
    assert not out["modes"][:, 3:6].any() and out["modes"][:, :3].any()
    assert all(not v[:, 1, :].any() for _, v, _, _ in core.hvp_calls)        # no probe moves the frozen atom
    calc = calc_on(core)
    with pytest.raises(ValueError, match="masses_amu is needed"):            # no pysisyphus here, and no table in the package
        calc.get_lowest_modes(elem, x_bohr, 1)
    with pytest.raises(ValueError, match="4 atoms, but masses_amu has 3"):
        calc.get_lowest_modes(elem, x_bohr, 1, MASSES[:3])
    core._gp = object()
    with pytest.raises(ValueError, match="graph-parallel"):
        calc.get_lowest_modes(elem, x_bohr, 1, MASSES)
    real = U.UMAcore.__new__(U.UMAcore)                                      # the real core's method refuses too, before it touches an engine
    real._gp = object()
    with pytest.raises(ValueError, match="graph-parallel"):
        real.lowest_modes(x_ang, MASSES)


def test_the_ase_facade_takes_the_atoms_masses():
    from pdb2reaction_amd.ase_calculator import UMXCalculator

    seen = []
    eng = types.SimpleNamespace(lowest_modes=lambda base, masses, k, **kw: seen.append((base, masses, k, kw)) or "result")
    calc = UMXCalculator.__new__(UMXCalculator)
    calc._ensure = lambda atoms: eng
    x = toy_geometry(4)
    atoms = types.SimpleNamespace(get_positions=lambda: x, get_masses=lambda: MASSES)
    assert calc.lowest_modes(atoms, 2, frozen=[3], tol=1e-4, block=3) == "result"
    base, masses, k, kw = seen[0]
    assert np.array_equal(base, x) and base.dtype == np.float64 and np.array_equal(masses, MASSES) and k == 2
    assert kw == {"frozen": [3], "tol": 1e-4, "block": 3}


def test_optimize_path_gsm_reports_hei_modes_only_when_asked():
    from test_path_opt import DoubleWell
    from pdb2reaction_amd._calculator_base import ANG2BOHR
    from pdb2reaction_amd.path_opt import optimize_path_gsm

    class WithModes(DoubleWell):
        calls = []

        def get_lowest_modes(self, elem, coords_bohr, k=1, masses_amu=None, **kw):
            WithModes.calls.append((list(elem), np.array(coords_bohr), k, masses_amu, kw))
            return {"freqs_cm": np.array([-410.0, 95.0])[:k], "eigenvalues": np.zeros(k), "modes": np.zeros((k, 18)), "converged": np.array([True, False])[:k],
                    "residuals": np.zeros(k), "images": 44}

    rng = np.random.default_rng(0)
    ref_ang = rng.uniform(-2.0, 2.0, (6, 3))
    elem = ["c", "H", "h", "O", "N", "H"]
    r_ang, p_ang = ref_ang.copy(), ref_ang.copy()
    r_ang[0, 0] -= 0.6 / ANG2BOHR
    p_ang[0, 0] += 0.6 / ANG2BOHR
    kw = dict(max_nodes=3, max_cycles=2, align=False)
    plain = optimize_path_gsm(elem, r_ang, p_ang, calc=WithModes(ref_ang * ANG2BOHR), **kw)
    assert "hei_modes" not in plain and WithModes.calls == []
    masses = np.arange(1.0, 7.0)
    res = optimize_path_gsm(elem, r_ang, p_ang, calc=WithModes(ref_ang * ANG2BOHR), hei_modes=2, masses_amu=masses, hei_modes_kw={"tol": 1e-5}, **kw)
    assert set(res) == set(plain) | {"hei_modes"} and len(WithModes.calls) == 1          # one call, after the run
    el, xb, k, m, more = WithModes.calls[0]
    assert el == [e.capitalize() for e in elem] and k == 2 and np.array_equal(m, masses) and more == {"tol": 1e-5}
    assert np.abs(xb.reshape(6, 3) - res["images_ang"][res["hei_index"]] * ANG2BOHR).max() < 1e-12     # the final highest-energy image, Bohr
    h = res["hei_modes"]
    assert set(h) == {"freqs_cm", "converged", "images", "n_imaginary"}
    assert list(h["freqs_cm"]) == [-410.0, 95.0] and list(h["converged"]) == [True, False] and h["images"] == 44 and h["n_imaginary"] == 1


# ---- LocalEnginePool.lowest_modes: the host backend over pool.hvp, every block of directions dealt over the engines -----------------------
class _Engine:
    """A stand-in engine whose products apply one fixed matrix, and which records what it was dealt."""

    def __init__(self, log, name, a):
        self.log, self.name, self.device, self.natoms, self.widened, self.a = log, name, 0, a.shape[0] // 3, False, a
        self.pin = None

    def set_workspace_limit(self, n):
        pass

    def close(self):
        pass

    def pin_graph(self, x, double_positions=False):
        self.log.append((self.name, "pin", double_positions))
        self.pin = (1, 1)

    def unpin_graph(self):
        self.log.append((self.name, "unpin"))
        self.pin = None

    def pinned_graph(self):
        return self.pin

    def hvp(self, base, dirs, base_of=None, step=1e-3, scheme="central", pin=True, return_curvature=False):
        d = np.asarray(dirs)
        self.log.append((self.name, "hvp", len(d), self.pin is not None))
        return _rowwise(self.a, d), np.zeros(len(d))


def _rowwise(a, dirs):
    """One matrix-vector product per direction: the bits of a row do not depend on the block it is dealt in (as on the engine)."""
    d = np.asarray(dirs, dtype=np.float64)
    return np.stack([a @ v.reshape(-1) for v in d]).reshape(d.shape)


def test_the_pool_deals_the_blocks_directions():
    from pdb2reaction_amd.parallel import LocalEnginePool
    import hvp_cases as HC

    a = HC.quadratic()[0]
    base, ones = np.random.default_rng(1).standard_normal((10, 3)), np.ones(10)
    log = []
    pool = LocalEnginePool([_Engine(log, "a", a), _Engine(log, "b", a)], gp=False, peer_sum=lambda *x: None, tensor_device=lambda e: "cpu",
                           free_bytes=lambda d: 1 << 40)
    try:
        pool.natoms = 10
        res = pool.lowest_modes(base, ones, 2, project="none", block=4, tol=1e-9)
        alone = M.lowest_modes(M.HostBackend(lambda b, d, step=1e-3, scheme="central": _rowwise(a, d)), base, ones, 2, project="none", block=4, tol=1e-9)
        assert res.converged.all() and MC.same_result(res, alone)
        assert log[:2] == [("a", "pin", True), ("b", "pin", True)] and log[-2:] == [("a", "unpin"), ("b", "unpin")]
        calls = [e for e in log if e[1] == "hvp"]
        assert all(pinned for _, _, _, pinned in calls)                      # every product replays the solver's pin
        assert sorted(calls[:2]) == [("a", "hvp", 2, True), ("b", "hvp", 2, True)]     # the first block of four: two directions each
        assert sum(m for _, _, m, _ in calls) == res.products
        assert pool.pinned_graph() is None
    finally:
        pool.close()
