"""The facades of the dimer without a GPU: the C ABI's three new exports against the header and the ctypes binding,
``uma_pysis.get_ts`` -- units, ``freeze_atoms``, the graph-parallel refusal -- on a stand-in core over an analytic surface,
``UMXCalculator.refine_saddle`` on a stand-in engine, the ``ts`` key of ``optimize_path_gsm`` and the pool's dealing of candidates."""
import importlib
import os
import re
import types

import numpy as np
import pytest

import dimer_cases as DC
from pdb2reaction_amd import dimer as D
from pdb2reaction_amd import engine as E

U = importlib.import_module("pdb2reaction_amd.uma_pysis")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AU2EV, BOHR_IN_ANG = 27.211386245988, 0.529177210903                        # written out by hand, as in tests/test_hvp_cpu.py


# ---- the C ABI and its bindings -----------------------------------------------------------------------------------------------------------
def test_the_three_exports_and_their_owners():
    from pdb2reaction_amd import build, parallel as P
    from pdb2reaction_amd.ase_calculator import UMXCalculator
    from pdb2reaction_amd.path_opt import optimize_path_gsm
    import inspect

    lib = E.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "umx.h")).read(), flags=re.S)
    for sym, nargs in (("umx_row_dot_dev", 7), ("umx_row_axpby_dev", 9), ("umx_row_absmax_dev", 6)):
        assert re.search(r"int\s+" + sym + r"\s*\(\s*umx_engine\s*\*", txt), sym
        assert hasattr(lib, sym) and sym in E.EXPORTED_SYMBOLS and len(getattr(lib, sym).argtypes) == nargs
    assert lib.umx_row_dot_dev(None, 1, None, None, 3, None, None) != 0      # no engine: refused, not a crash
    assert lib.umx_row_axpby_dev(None, 1, None, None, None, None, 3, None, None) != 0
    assert lib.umx_row_absmax_dev(None, 1, None, 3, None, None) != 0
    assert lib.umx_abi_version() == 10                                       # additive: no version bump
    for owner in (E.Engine, P.LocalEnginePool, U.UMAcore):
        assert callable(getattr(owner, "refine_saddles")), owner
    assert callable(U.uma_pysis.get_ts) and callable(UMXCalculator.refine_saddle)
    for name in ("row_dot_dev", "row_axpby_dev", "row_absmax_dev"):
        assert callable(getattr(E.Engine, name))
    assert any(os.path.basename(d) == "umx_rowblocks.h" for d in build.dependencies())
    sig = inspect.signature(E.Engine.refine_saddles).parameters
    assert [p for p in sig][1:3] == ["x0", "modes0"] and sig["thresh"].default == "gau" and sig["step"].default == 1e-3 and sig["max_cycles"].default == 200
    assert (sig["max_rot"].default, sig["rot_tol"].default, sig["max_step"].default, sig["verify"].default) == (2, 0.1, 0.1, False)
    assert inspect.signature(optimize_path_gsm).parameters["hei_tsopt"].default is False
    assert D.ROW_MAX == 64 and D.C_FLOOR == 1e-2 and D.KEEP_LAST == 7


# ---- uma_pysis.get_ts ----------------------------------------------------------------------------------------------------------------------
class SurfaceCore:
    """A stand-in for ``UMAcore``: ``refine_saddles`` through the host backend over surface A (eV, A)."""

    def __init__(self):
        self.ef, self.saddle, self.a = DC.surface_a(0.5)
        self.z = list(range(10))
        self.calls = []

    def refine_saddles(self, coord_ang, modes0=None, **kw):
        coord_ang = np.asarray(coord_ang, dtype=np.float64).reshape(-1, 10, 3)     # as UMAcore.refine_saddles shapes it
        self.calls.append((coord_ang.copy(), None if modes0 is None else np.array(modes0), dict(kw)))
        kw.setdefault("project", "none")
        if modes0 is None:                                                   # (the stand-in has no lowest_modes: any direction will do)
            modes0 = np.ones((len(coord_ang), 10, 3))
        return D.refine_saddles(D.HostBackend(DC.fd_hvp(self.ef)), coord_ang, modes0, **kw)


def calc_on(core, **kw):
    calc = U.uma_pysis(model="synthetic", **kw)
    calc._core = core
    return calc


def test_get_ts_units_keys_and_keywords():
    core = SurfaceCore()
    calc = calc_on(core)
    elem = ["C"] * 10
    rng = np.random.default_rng(2)
    x_ang = core.saddle + 0.1 * rng.standard_normal((10, 3))
    mode = rng.standard_normal(30)
    out = calc.get_ts(elem, (x_ang / BOHR_IN_ANG).reshape(-1), mode)
    assert set(out) == {"coords", "energy", "forces", "mode", "curvature", "converged", "cycles", "images"}
    want = D.refine_saddles(D.HostBackend(DC.fd_hvp(core.ef)), core.calls[-1][0], mode.reshape(1, 10, 3), project="none")[0]
    assert out["converged"] and want.converged and out["cycles"] == want.cycles and out["images"] == want.images
    assert np.abs(core.calls[-1][0][0] - x_ang).max() < 1e-8 and core.calls[-1][2]["thresh"] == "gau" and core.calls[-1][2]["frozen"] == ()
    assert out["coords"].shape == (30,) and np.abs(out["coords"] * BOHR_IN_ANG - want.x.reshape(-1)).max() < 1e-8
    assert abs(out["energy"] * AU2EV / want.energy - 1.0) < 1e-8
    assert np.abs(out["forces"] * AU2EV / BOHR_IN_ANG - want.forces.reshape(-1)).max() < 1e-8 * np.abs(want.forces).max() + 1e-12
    assert abs(out["curvature"] * AU2EV / BOHR_IN_ANG ** 2 / want.curvature - 1.0) < 1e-8
    assert DC.same_bits(out["mode"], want.mode.reshape(-1)) and abs(np.linalg.norm(out["mode"]) - 1.0) < 1e-12
    # thresholds in Hartree/Bohr, steps in Bohr
    calc.get_ts(elem, x_ang / BOHR_IN_ANG, mode, thresh=(1e-3, 5e-4), step_bohr=0.004, max_step_bohr=0.1, max_cycles=3, max_rot=1)
    kw = core.calls[-1][2]
    assert abs(kw["thresh"][0] / (1e-3 * AU2EV / BOHR_IN_ANG) - 1.0) < 1e-8 and abs(kw["thresh"][1] / (5e-4 * AU2EV / BOHR_IN_ANG) - 1.0) < 1e-8
    assert abs(kw["step"] / (0.004 * BOHR_IN_ANG) - 1.0) < 1e-8 and abs(kw["max_step"] / (0.1 * BOHR_IN_ANG) - 1.0) < 1e-8
    assert kw["max_cycles"] == 3 and kw["max_rot"] == 1
    calc.get_ts(elem, x_ang / BOHR_IN_ANG, max_cycles=1)                     # mode=None reaches the core as None
    assert core.calls[-1][1] is None


def test_get_ts_freeze_atoms_and_the_graph_parallel_refusal():
    core = SurfaceCore()
    elem = ["C"] * 10
    rng = np.random.default_rng(4)
    x_ang = core.saddle + 0.05 * rng.standard_normal((10, 3))
    x_bohr = (x_ang / BOHR_IN_ANG).reshape(-1)
    frozen = calc_on(core, freeze_atoms=[7, 2])
    out = frozen.get_ts(elem, x_bohr, rng.standard_normal(30), max_cycles=4, thresh=(1e-12, 1e-12))
    assert core.calls[-1][2]["frozen"] == (2, 7) and not out["converged"] and out["cycles"] == 4
    from pdb2reaction_amd._calculator_base import ANG2BOHR

    moved = out["coords"].reshape(10, 3) - core.calls[-1][0][0] * ANG2BOHR   # against the solver's own start in the facade's conversion
    assert not moved[[2, 7]].any() and np.abs(moved).max() > 1e-3            # the frozen rows stay at the start's values, bit for bit
    assert not out["forces"].reshape(10, 3)[[2, 7]].any() and not out["mode"].reshape(10, 3)[[2, 7]].any()
    core._gp = object()
    with pytest.raises(ValueError, match="graph-parallel"):
        frozen.get_ts(elem, x_bohr)
    real = U.UMAcore.__new__(U.UMAcore)                                      # the real core's method refuses too, before it touches an engine
    real._gp = object()
    with pytest.raises(ValueError, match="graph-parallel"):
        real.refine_saddles(x_ang)


# ---- UMXCalculator.refine_saddle -----------------------------------------------------------------------------------------------------------
def test_the_ase_facade_returns_new_atoms_and_feeds_the_masses():
    from pdb2reaction_amd.ase_calculator import UMXCalculator

    seen = []
    x = np.arange(12.0).reshape(4, 3)
    result = types.SimpleNamespace(x=x + 1.0)
    eng = types.SimpleNamespace(refine_saddles=lambda x0, modes0=None, **kw: seen.append((x0, modes0, kw)) or [result])
    calc = UMXCalculator.__new__(UMXCalculator)
    calc._ensure = lambda atoms: eng

    class Atoms:
        def __init__(self, p):
            self.p = np.array(p)

        def get_positions(self):
            return self.p

        def get_masses(self):
            return np.array([12.0, 1.0, 16.0, 14.0])

        def copy(self):
            return Atoms(self.p)

        def set_positions(self, p):
            self.p = np.array(p)

    atoms = Atoms(x)
    new, res = calc.refine_saddle(atoms, mode="m", frozen=[3], max_cycles=9)
    assert res is result and new is not atoms and np.array_equal(new.get_positions(), x + 1.0) and np.array_equal(atoms.get_positions(), x)
    x0, m0, kw = seen[0]
    assert np.array_equal(x0, x) and x0.dtype == np.float64 and m0 == "m" and kw == {"frozen": [3], "max_cycles": 9}
    calc.refine_saddle(atoms, verify=True)
    assert np.array_equal(seen[1][2]["masses"], [12.0, 1.0, 16.0, 14.0]) and seen[1][2]["verify"] is True and seen[1][1] is None


# ---- optimize_path_gsm(hei_tsopt=True) -----------------------------------------------------------------------------------------------------
def test_optimize_path_gsm_refines_the_hei_only_when_asked():
    from test_path_opt import DoubleWell
    from pdb2reaction_amd._calculator_base import ANG2BOHR
    from pdb2reaction_amd.path_opt import optimize_path_gsm

    class WithTs(DoubleWell):
        ts_calls, modes_calls = [], []

        def get_ts(self, elem, coords_bohr, mode=None, **kw):
            WithTs.ts_calls.append((list(elem), np.array(coords_bohr), np.array(mode), kw))
            return {"coords": np.asarray(coords_bohr) + 0.25, "energy": -1.5, "forces": np.zeros(18), "mode": np.zeros(18), "curvature": -0.02,
                    "converged": True, "cycles": 5, "images": 17}

        def get_lowest_modes(self, elem, coords_bohr, k=1, masses_amu=None, **kw):
            WithTs.modes_calls.append(np.array(coords_bohr))
            return {"freqs_cm": np.array([-410.0]), "converged": np.array([True]), "images": 44}

    rng = np.random.default_rng(0)
    ref_ang = rng.uniform(-2.0, 2.0, (6, 3))
    elem = ["c", "H", "h", "O", "N", "H"]
    r_ang, p_ang = ref_ang.copy(), ref_ang.copy()
    r_ang[0, 0] -= 0.6 / ANG2BOHR
    p_ang[0, 0] += 0.6 / ANG2BOHR
    kw = dict(max_nodes=3, max_cycles=2, align=False)
    plain = optimize_path_gsm(elem, r_ang, p_ang, calc=WithTs(ref_ang * ANG2BOHR), **kw)
    assert set(plain) == {"images_ang", "energies", "hei_index", "converged", "cycles", "force_evaluations", "fully_grown", "history", "timing", "device",
                          "preopt", "align", "files", "defaults", "cell", "pbc"}                 # the keys as they were
    assert WithTs.ts_calls == [] and WithTs.modes_calls == []
    res = optimize_path_gsm(elem, r_ang, p_ang, calc=WithTs(ref_ang * ANG2BOHR), hei_tsopt=True, hei_tsopt_kw={"max_cycles": 7}, hei_modes=1,
                            masses_amu=np.ones(6), **kw)
    assert set(res) == set(plain) | {"ts", "hei_modes"} and len(WithTs.ts_calls) == 1
    el, xb, mode, more = WithTs.ts_calls[0]
    hei = res["hei_index"]
    imgs = res["images_ang"] * ANG2BOHR
    assert el == [e.capitalize() for e in elem] and more == {"max_cycles": 7}
    assert np.abs(xb.reshape(6, 3) - imgs[hei]).max() < 1e-12                 # the final highest-energy image, Bohr
    tangent = imgs[min(hei + 1, len(imgs) - 1)] - imgs[max(hei - 1, 0)]
    assert np.abs(mode.reshape(6, 3) - tangent).max() < 1e-12 and np.abs(tangent).max() > 0.1
    t = res["ts"]
    assert set(t) == {"coords_ang", "energy", "curvature", "converged", "cycles", "images"}
    assert np.abs(t["coords_ang"] * ANG2BOHR - (xb.reshape(6, 3) + 0.25)).max() < 1e-12 and t["energy"] == -1.5 and t["curvature"] == -0.02
    assert t["converged"] is True and t["cycles"] == 5 and t["images"] == 17
    assert np.abs(WithTs.modes_calls[0] - (xb + 0.25)).max() < 1e-12          # the frequencies are those of the refined geometry


# ---- LocalEnginePool.refine_saddles: candidates dealt over the engines ---------------------------------------------------------------------
class _Engine:
    """A stand-in engine over an analytic surface, which records what it was dealt."""

    def __init__(self, log, name, ef):
        self.log, self.name, self.device, self.natoms, self.widened = log, name, 0, 10, False
        self._hvp = DC.fd_hvp(ef)

    def set_workspace_limit(self, n):
        pass

    def close(self):
        pass

    def pinned_graph(self):
        return None

    def _pbc_flags(self):
        return None

    def hvp(self, base, dirs, base_of=None, step=1e-3, scheme="central", pin=True, return_curvature=False, return_base=False, base_forces=None):
        self.log.append((self.name, len(base), len(dirs), list(base_of), base_forces is not None))
        return self._hvp(base, dirs, base_of=base_of, step=step, scheme=scheme, return_base=return_base, base_forces=base_forces)


def test_the_pool_deals_the_candidates_and_gives_the_single_engines_bits():
    from pdb2reaction_amd.parallel import LocalEnginePool

    ef, saddle, _ = DC.surface_a(0.5)
    rng = np.random.default_rng(9)
    x0 = saddle[None] + 0.18 * rng.standard_normal((3, 10, 3))
    n0 = rng.standard_normal((3, 10, 3))
    log = []
    pool = LocalEnginePool([_Engine(log, "a", ef), _Engine(log, "b", ef)], gp=False, peer_sum=lambda *x: None, tensor_device=lambda e: "cpu",
                           free_bytes=lambda d: 1 << 40)
    try:
        pool.natoms = 10
        res = pool.refine_saddles(x0, n0, project="none")
        alone = D.refine_saddles(D.HostBackend(DC.fd_hvp(ef)), x0, n0, project="none")
        assert all(r.converged for r in res) and all(DC.same_result(a, b) is None for a, b in zip(res, alone))
        assert sorted(log[:2]) == [("a", 2, 2, [0, 1], False), ("b", 1, 1, [0], False)]        # three candidates: two and one, each with its own bases
        assert all(bases == dirs and bo == list(range(dirs)) for _, bases, dirs, bo, _ in log) and any(given for *_, given in log)
        with pytest.raises(ValueError, match="one direction per base"):
            pool.hvp_candidates(x0, n0[:2])
    finally:
        pool.close()
