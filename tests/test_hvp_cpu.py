"""Hessian-vector products without a GPU: the Lanczos recursion on a product function, the driver's ``climb_lanczos_hvp`` key, and
``uma_pysis.get_hvp`` -- units, frozen rows, refusals -- on the toy core of tests/toy_core.py (wrapped here, not edited)."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import hvp_cases as HC
from toy_core import ToyPairCore, toy_geometry
from pdb2reaction_amd import engine as E
from pdb2reaction_amd import hessian as H
from pdb2reaction_amd.gsm import GrowingStringDriver, lanczos_lowest_mode, lanczos_lowest_mode_t

U = importlib.import_module("pdb2reaction_amd.uma_pysis")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# written out by hand: CODATA-2018 Hartree in eV, Bohr radius in Angstrom (the package's constants are of another vintage: they agree
# to 1.4e-9 relative, so the unit checks below hold 1e-8 -- a wrong power of the Bohr radius is off by a factor of 1.9)
AU2EV, BOHR_IN_ANG = 27.211386245988, 0.529177210903
EV_A2_TO_AU = (1.0 / AU2EV) * BOHR_IN_ANG * BOHR_IN_ANG


# ---- the C ABI and its bindings -----------------------------------------------------------------------------------------------------------
def test_the_two_exports_and_their_signatures():
    from pdb2reaction_amd import parallel as P
    from pdb2reaction_amd.ase_calculator import UMXCalculator

    lib = E.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "umx.h")).read(), flags=re.S)
    for sym in ("umx_hvp", "umx_hvp_dev"):
        assert re.search(r"int\s+" + sym + r"\s*\(\s*umx_engine\s*\*", txt), sym
        assert hasattr(lib, sym) and sym in E.EXPORTED_SYMBOLS
    assert lib.umx_abi_version() == 10                                       # additive: no version bump
    assert len(lib.umx_hvp.argtypes) == 12 and len(lib.umx_hvp_dev.argtypes) == 13
    assert lib.umx_hvp(None, 1, None, 1, None, None, 1e-3, 0, None, None, None, None) != 0      # no engine: refused, not a crash
    assert lib.umx_hvp_dev(None, 1, None, 1, None, None, 1e-3, 0, None, None, None, None, None) != 0
    for owner in (E.Engine, P.LocalEnginePool, P.EngineStringEvaluator, U.UMAcore, UMXCalculator):
        assert callable(getattr(owner, "hvp")), owner
    assert callable(E.Engine.hvp_dev) and callable(U.uma_pysis.get_hvp)
    from pdb2reaction_amd import build

    assert any(os.path.basename(d) == "umx_hvp.h" for d in build.dependencies())


# ---- the recursion -----------------------------------------------------------------------------------------------------------------------
def _recursion_before(grad_fn, x, g0, guess, *, dx=5e-3, dl=1e-2, max_cycles=25, orient=None):
    """``gsm.lanczos_lowest_mode_t`` as it stood before ``hvp_fn``: the forward difference of gradients, nothing else -- kept here so that
    the default path is compared with something that is not itself."""
    n = x.numel()
    x = x.reshape(-1)
    guess = guess.reshape(-1).to(x.dtype)
    r = guess.clone()
    beta = float(r.norm())
    qs, alphas, betas = [], [], []
    q_prev = torch.zeros_like(x)
    w_prev = None
    w_min, v_min = 0.0, r / beta
    steps = 0
    for steps in range(1, min(int(max_cycles), n) + 1):
        q = r / beta
        if qs:
            qm = torch.stack(qs)
            q = q - qm.T @ (qm @ q)
        q = q / q.norm().clamp_min(1e-30)
        u = (grad_fn(x + dx * q).reshape(-1) - g0.reshape(-1)) / dx
        if qs:
            u = u - beta * q_prev
        alpha = float(q @ u)
        r = u - alpha * q
        qs.append(q)
        alphas.append(alpha)
        w, v = np.linalg.eigh(np.diag(alphas) + np.diag(betas, 1) + np.diag(betas, -1))
        w_min = float(w[0])
        v_min = torch.stack(qs, dim=1) @ torch.as_tensor(v[:, 0], dtype=x.dtype, device=x.device)
        beta = float(r.norm())
        if w_prev is not None and abs(w_min - w_prev) <= dl * max(abs(w_prev), 1e-12):
            break
        if beta < 1e-10:
            break
        w_prev, q_prev = w_min, q
        betas.append(beta)
    v_min = v_min / v_min.norm().clamp_min(1e-30)
    if float(v_min @ (guess if orient is None else orient.reshape(-1).to(x.dtype))) < 0.0:
        v_min = -v_min
    return w_min, v_min, steps


def test_lanczos_on_a_product_function():
    a, x = HC.quadratic()
    w, v = np.linalg.eigh(a)
    assert w[0] < 0.0 < w[1]
    at, xt = torch.as_tensor(a), torch.as_tensor(x)
    guess = torch.as_tensor(np.random.default_rng(2).standard_normal(len(x)))
    seen = []

    def hvp_fn(q):
        seen.append(float(q.norm()))
        return at @ q

    w_l, v_l, steps = lanczos_lowest_mode_t(None, xt, None, guess, dl=0.0, max_cycles=30, hvp_fn=hvp_fn)
    assert steps == len(seen) and all(abs(s - 1.0) < 1e-12 for s in seen)     # every probe is a unit vector
    sign = 1.0 if float(v_l @ torch.as_tensor(v[:, 0])) > 0 else -1.0
    assert abs(w_l - w[0]) < 1e-8 and np.abs(sign * v_l.numpy() - v[:, 0]).max() < 1e-8
    # hvp_fn=None: the unchanged path -- bit for bit the recursion as it stood before the keyword existed, written out below
    g0 = a @ x
    grad_t = lambda xq: torch.as_tensor(a @ xq.numpy())                      # noqa: E731
    for kw in ({}, {"dl": 1e-6, "max_cycles": 12}, {"dx": 1e-2}):
        w_old, v_old, n_old = _recursion_before(grad_t, xt, torch.as_tensor(g0), guess, **kw)
        w_new, v_new, n_new = lanczos_lowest_mode_t(grad_t, xt, torch.as_tensor(g0), guess, hvp_fn=None, **kw)
        assert w_old == w_new and n_old == n_new and np.array_equal(v_old.numpy(), v_new.numpy()), kw
        w_np, v_np, n_np = lanczos_lowest_mode(lambda xq: a @ xq, x, g0, guess.numpy(), **kw)       # the numpy face takes the same path
        assert w_np == w_old and n_np == n_old and np.array_equal(v_np, v_old.numpy())
    w_old, v_old, n_old = _recursion_before(grad_t, xt, torch.as_tensor(g0), guess)
    v_old = v_old.numpy()
    # the same stop rule on exact products lands where the forward difference of this quadratic does
    w_h, v_h, n_h = lanczos_lowest_mode_t(None, xt, None, guess, hvp_fn=lambda q: at @ q)
    assert n_h == n_old and abs(w_h - w_old) < 1e-6 and np.abs(v_h.numpy() - v_old).max() < 1e-5


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
class ToyCalc:
    """The toy core behind the driver's calculator contract (Bohr / Hartree), with an ``hvp`` from the core's analytic Hessian that
    records how it was called."""

    def __init__(self, n, with_hvp=True):
        self.core = ToyPairCore(n, seed=3)
        self.n = n
        self.calls = []                                                      # (|q|, scheme, base handed in, base asked for)
        self.pins = []                                                       # "pin" / "unpin", and "hvp" for every product in between
        if not with_hvp:
            self.hvp = None

    def get_forces_batch(self, atoms, coords):
        c = np.asarray(coords, dtype=np.float64).reshape(len(coords), self.n, 3) * BOHR_IN_ANG
        res = self.core.compute_batch(c, forces=True)
        return {"energy": res["energy"] / AU2EV, "forces": (res["forces"].astype(np.float64) * H.EV_PER_ANG_TO_AU).reshape(len(coords), -1)}

    def hvp_pin(self, x0):
        self.pins.append("pin")

    def hvp_unpin(self):
        self.pins.append("unpin")

    def hvp(self, x0, q, dx, scheme="central", base=None, return_base=False):
        self.pins.append("hvp")
        self.calls.append((float(np.linalg.norm(q)), scheme, base is not None, bool(return_base), float(dx)))
        h = self.core.compute(np.asarray(x0).reshape(self.n, 3) * BOHR_IN_ANG, hessian=True)["hessian"].double().numpy().reshape(3 * self.n, 3 * self.n)
        hv = (h @ np.asarray(q, dtype=np.float64).reshape(-1)) * H.EV_PER_ANG2_TO_AU
        return (hv, "f0-token") if return_base else hv


def drive(mode="absent", with_hvp=True):
    n = 4
    calc = ToyCalc(n, with_hvp)
    r, p = toy_geometry(n, 0).reshape(-1) / BOHR_IN_ANG, toy_geometry(n, 1).reshape(-1) / BOHR_IN_ANG
    gs = {"max_nodes": 3, "perp_thresh": 1e9, "climb_rms": 1e9, "climb_lanczos_rms": 1e9}
    if mode != "absent":
        gs["climb_lanczos_hvp"] = mode
    drv = GrowingStringDriver(["X"] * n, r, p, calc, gs_kw=gs, stopt_kw={"max_cycles": 8, "max_step": 0.05})
    return drv, drv.run(), calc


def test_the_driver_key():
    d0, r0, c0 = drive("absent")
    d1, r1, c1 = drive(None)
    assert d0.lanczos_calls >= 3 and d0.lanczos_evals > 0
    assert np.array_equal(r0.coords, r1.coords) and np.array_equal(r0.energies, r1.energies)
    assert (d0.n_eval, d0.lanczos_evals, d0.lanczos_calls) == (d1.n_eval, d1.lanczos_evals, d1.lanczos_calls)
    assert c0.calls == [] and c1.calls == [] and c0.core.calls == c1.core.calls      # today's evaluations, no product asked for
    for mode in ("central", "forward"):
        d, r, c = drive(mode)
        assert d.lanczos_calls >= 3 and len(c.calls) >= d.lanczos_calls
        assert all(abs(nq - 1.0) < 1e-12 and sch == mode and dx == 5e-3 for nq, sch, _, _, dx in c.calls)
        recursions = d.lanczos_calls + d.lanczos_warm_rejected
        # the evaluator is asked to pin once per recursion, around all of its products, and to unpin afterwards
        assert c.pins.count("pin") == c.pins.count("unpin") == recursions and c.pins[0] == "pin" and c.pins[-1] == "unpin"
        assert all(b in ("hvp", "unpin") for a, b in zip(c.pins, c.pins[1:]) if a in ("pin", "hvp")) and "pin" not in c0.pins
        if mode == "central":
            assert d.lanczos_evals == 2 * len(c.calls) and not any(given or asked for _, _, given, asked, _ in c.calls)
        else:
            # one image per step plus the base once per recursion: the first product asks for the base, the others hand it back
            assert sum(asked for _, _, _, asked, _ in c.calls) == recursions
            assert all(given != asked for _, _, given, asked, _ in c.calls)
            assert d.lanczos_evals == len(c.calls) + recursions
        assert r.timing["lanczos_evals"] == d.lanczos_evals and np.isfinite(r.energies).all()
        assert sum(lg[2] for lg in d.lanczos_log) <= d.lanczos_evals              # the log counts images too
    with pytest.raises(ValueError, match="climb_lanczos_hvp='central' needs an evaluator with an `hvp"):
        drive("central", with_hvp=False)
    with pytest.raises(ValueError, match="climb_lanczos_hvp='analytic'"):
        drive("analytic")


# ---- uma_pysis.get_hvp ---------------------------------------------------------------------------------------------------------------------
class QuadCore(ToyPairCore):
    """The toy core with a product entry: H = K, a fixed matrix in eV/A^2 (the Hessian of the quadratic 1/2 x K x), applied by hand."""

    def __init__(self, n):
        super().__init__(n)
        k = np.arange(1.0, 9.0 * n * n + 1.0).reshape(3 * n, 3 * n) / 7.0
        self.K = k + k.T
        self.hvp_calls = []

    def hvp(self, coord_ang, vectors, *, step=1e-3, scheme="central", base_of=None):
        v = np.asarray(vectors, dtype=np.float64)
        self.hvp_calls.append((np.array(coord_ang, dtype=np.float64), v.copy(), float(step), scheme))
        return (v.reshape(len(v), -1) @ self.K.T).reshape(v.shape)


def test_get_hvp_units_frozen_rows_and_refusals():
    n = 3
    elem = ["C", "H", "O"]
    x_ang = toy_geometry(n)
    x_bohr = (x_ang / BOHR_IN_ANG).reshape(-1)
    assert abs(H.EV_PER_ANG2_TO_AU / EV_A2_TO_AU - 1.0) < 1e-8
    core = QuadCore(n)
    calc = U.uma_pysis(model="synthetic")
    calc._core = core
    v = np.zeros((2, 3 * n))
    v[0, 4], v[1, :] = 1.0, np.arange(1.0, 3 * n + 1)
    out = calc.get_hvp(elem, x_bohr, v)
    assert set(out) == {"hvp"} and out["hvp"].shape == (2, 3 * n) and out["hvp"].dtype == np.float64
    # by hand: column 4 of K, and K times (1..9), in eV/A^2; 1 eV/A^2 = (1 / 27.2114 Hartree) x (0.529177 A/Bohr)^2
    want = np.stack([core.K[:, 4], core.K @ np.arange(1.0, 3 * n + 1)]) * EV_A2_TO_AU
    assert np.abs(out["hvp"] / want - 1.0).max() < 1e-8
    pos, vec, step, scheme = core.hvp_calls[-1]
    assert np.abs(pos - x_ang).max() < 1e-8 and vec.shape == (2, n, 3) and np.array_equal(vec.reshape(2, -1), v)
    assert step == 1e-3 and scheme == "central"                              # step_bohr=None: 1e-3 A
    calc.get_hvp(elem, x_bohr.reshape(n, 3), v[1], step_bohr=0.01, scheme="forward")      # (3N,) and (N,3) are taken too
    pos, vec, step, scheme = core.hvp_calls[-1]
    assert vec.shape == (1, n, 3) and abs(step / (0.01 * BOHR_IN_ANG) - 1.0) < 1e-8 and scheme == "forward"
    # frozen rows: zero in the vectors the core sees, zero in the result, the caller's array untouched -- the active block's product
    frozen = U.uma_pysis(model="synthetic", freeze_atoms=[1])
    frozen._core = core
    keep = v.copy()
    out = frozen.get_hvp(elem, x_bohr, v)["hvp"]
    vec = core.hvp_calls[-1][1].reshape(2, -1)
    assert np.array_equal(v, keep) and not vec[:, 3:6].any() and np.array_equal(vec[:, :3], v[:, :3]) and np.array_equal(vec[:, 6:], v[:, 6:])
    assert not out[:, 3:6].any() and out[:, :3].any()
    act = [0, 1, 2, 6, 7, 8]
    want = (core.K[np.ix_(act, act)] @ v[:, act].T).T * EV_A2_TO_AU
    assert not want[0].any() and not out[0].any()                           # e_4 lies on the frozen atom: nothing is left of it
    assert np.abs(out[1, act] / want[1] - 1.0).max() < 1e-8
    # refusals
    for bad, pattern in ((dict(scheme="backward"), "scheme must be"), (dict(step_bohr=0.0), "step must be finite and positive"),
                         (dict(step_bohr=float("nan")), "step must be finite and positive")):
        with pytest.raises(ValueError, match=pattern):
            calc.get_hvp(elem, x_bohr, v, **bad)
    for shape in (np.zeros(3 * n + 1), np.zeros((2, 3 * n - 3)), np.zeros((0, 3 * n))):
        with pytest.raises(ValueError, match="vectors must be"):
            calc.get_hvp(elem, x_bohr, shape)
    core._gp = object()                                                      # a graph-parallel core, as hessian_pin_graph refuses it
    with pytest.raises(ValueError, match="graph-parallel"):
        calc.get_hvp(elem, x_bohr, v)


# ---- LocalEnginePool.hvp: directions dealt in contiguous blocks, every engine all bases and its slice of base_of --------------------------
class _Engine:
    def __init__(self, log, name):
        self.log, self.name, self.device, self.natoms, self.widened = log, name, 0, 2, False

    def set_workspace_limit(self, n):
        pass

    def close(self):
        pass

    def hvp(self, base, dirs, base_of=None, step=1e-3, scheme="central", pin=True, return_curvature=False):
        self.log.append((self.name, np.array(base), np.array(dirs), None if base_of is None else list(base_of), step, scheme, pin))
        hv = 2.0 * np.asarray(dirs)
        return hv, hv.reshape(len(hv), -1).sum(axis=1)


def test_the_pool_deals_directions():
    from pdb2reaction_amd.parallel import LocalEnginePool

    log = []
    pool = LocalEnginePool([_Engine(log, "a"), _Engine(log, "b")], gp=False, peer_sum=lambda *a: None, tensor_device=lambda e: "cpu", free_bytes=lambda d: 1 << 40)
    try:
        pool.natoms = 2
        base = np.arange(12.0).reshape(2, 2, 3)
        dirs = np.arange(30.0).reshape(5, 2, 3)
        hv, curv = pool.hvp(base, dirs, [1, 0, 1, 1, 0], step=2e-3, scheme="forward", return_curvature=True)
        assert np.array_equal(hv, 2.0 * dirs) and np.array_equal(curv, (2.0 * dirs).reshape(5, -1).sum(axis=1))
        assert pool.last_route == "batch" and pool.last_blocks == [(0, 3), (3, 5)]
        got = {name: (b, d, bo, st, sc, pin) for name, b, d, bo, st, sc, pin in log}
        for name, (lo, hi) in (("a", (0, 3)), ("b", (3, 5))):
            b, d, bo, st, sc, pin = got[name]
            assert np.array_equal(b, base) and np.array_equal(d, dirs[lo:hi]) and bo == [1, 0, 1, 1, 0][lo:hi] and (st, sc, pin) == (2e-3, "forward", True)
        log.clear()
        one = pool.hvp(base[0], dirs[2])                                     # a single direction: engine 0 alone
        assert pool.last_route == "single" and [entry[0] for entry in log] == ["a"] and np.array_equal(one, 2.0 * dirs[2:3])
        with pytest.raises(ValueError, match="5 directions, but base_of has 2"):
            pool.hvp(base, dirs, [0, 1])
    finally:
        pool.close()
