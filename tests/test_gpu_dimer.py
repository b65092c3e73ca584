"""The batched dimer on the engine (``Engine.refine_saddles``, pdb2reaction_amd/dimer.py): the saddle fixture of tests/dimer_cases.py,
12 atoms, synthetic weights seed 0, open boundaries, a neighbour cap that cannot bind.

What is held.  The device backend against the host backend over ``Engine.hvp``, every field and history record bit for bit; a batch
against its singles, bit for bit (``umx_hvp``'s image-alone guarantee carried through the row kernels); every recorded cycle against an
independent evaluation of its geometry and an independent product along its direction; convergence of the device backend on an analytic
surface written in torch; convergence on the engine from five noisy starts without a start direction; the calculators.
Bounds on the engine: 15 cycles, 0.1 A from the fixture, C in [-0.9, -0.4] -- the float64 checker's figures (3-4 cycles, 0.037 A, -0.70
... -0.57; tests/dimer_cases.py) with a three- to five-fold margin: the engine follows the checker to 1e-3 eV/A, not to the bit."""
import numpy as np
import pytest

import dimer_cases as DC
import hvp_cases as HC
import modes_cases as MC
from pdb2reaction_amd import dimer as D
from pdb2reaction_amd import modes as M

pytestmark = pytest.mark.gpu

NEVER = (1e-9, 1e-9)                                                         # thresholds no cycle meets: the run ends at max_cycles
SIX = dict(max_cycles=6, thresh=NEVER)


@pytest.fixture(scope="module")
def eng(weights):
    from pdb2reaction_amd.engine import Engine

    e = Engine(0)
    e.load_weights(weights)
    yield e
    e.close()


def bind(e, cell=None, pbc=None, z=DC.Z, max_neigh=DC.MAX_NEIGH):
    e.set_system(z, max_neigh=max_neigh)
    e.set_cell(cell, pbc)


@pytest.fixture(scope="module")
def six(eng):
    """Computed once and left unchanged: starts 0, 1, 2 and their start directions (the lowest mode at the fixture plus 5 % noise), the
    K = 3 run of six cycles on the device backend, and whether the engine was left unpinned."""
    assert DC.MAX_NEIGH >= len(DC.Z) - 1                                     # the cap cannot bind
    bind(eng)
    mode = eng.lowest_modes(DC.X, np.ones(12), 1).modes[0]
    x0 = np.stack([DC.start(s) for s in range(3)])
    n0 = np.stack([DC.noisy_mode(mode, s) for s in range(3)])
    res = eng.refine_saddles(x0, n0, **SIX)
    return dict(mode=mode, x0=x0, n0=n0, res=res, pin_after=eng.pinned_graph())


def test_host_and_device_backends_give_the_same_bits(eng, six):
    bind(eng)
    host = D.refine_saddles(D.HostBackend(eng.hvp, pinner=eng), six["x0"], six["n0"], **SIX)
    assert six["pin_after"] is None and eng.pinned_graph() is None
    for i, (h, d) in enumerate(zip(host, six["res"])):
        assert d.reason == "max_cycles" and not d.converged and d.cycles == 6 and len(d.history) == 6
        assert DC.same_result(h, d) is None, (i, DC.same_result(h, d))
    print("cycles x images:", [(r.cycles, r.images, [h["rotations"] for h in r.history]) for r in six["res"]])


def test_a_batch_is_its_singles_bit_for_bit(eng, six):
    bind(eng)
    for i in range(3):
        single = eng.refine_saddles(six["x0"][i], six["n0"][i], **SIX)[0]
        assert DC.same_result(single, six["res"][i]) is None, (i, DC.same_result(single, six["res"][i]))


def test_every_recorded_cycle_against_independent_evaluations(eng, six):
    """Energy and max|F| of the record: one unpinned ``energy_forces`` of the recorded geometry and the NumPy statement of the projection,
    bit for bit.  ``curv_probe``: one forward ``Engine.hvp`` along the recorded direction gives n.Hn of the UNPROJECTED product; the record
    holds n.P(Hn), which differs by (Q n).(Q Hn) with |Q n| <= 1: held to twice the largest |Q.Hn| entry, computed here.  Without a
    projection nothing stands between the two: 1e-9 max(1, |C|)."""
    bind(eng)
    active = np.ones(12, dtype=bool)
    for i, r in enumerate(six["res"]):
        for t, h in enumerate(r.history):
            e, f = eng.energy_forces(h["x"][None], double_positions=True)
            q = M.tr_vectors(h["x"], np.ones(12), active, "tr")
            f64 = f[0].astype(np.float64).reshape(1, -1)
            fp = M.blk_combine(q, M.blk_gram(q, f64), f64, True)             # P F: the projection's NumPy statement
            assert DC.same_bits(np.float64(e[0]), np.float64(h["energy"])), (i, t)
            assert DC.same_bits(np.float64(D.row_absmax(fp)[0]), np.float64(h["max_force"])), (i, t)
            hv, curv = eng.hvp(h["x"], h["n"], scheme="forward", return_curvature=True)
            bound = 2.0 * np.abs(q @ hv.reshape(-1)).max()
            print(f"candidate {i} cycle {t}: curv_probe {h['curv_probe']:.9f}, independent {curv[0]:.9f}, bound {bound:.3e}")
            assert abs(h["curv_probe"] - curv[0]) <= bound, (i, t)
    res = eng.refine_saddles(six["x0"][0], six["n0"][0], project="none", max_cycles=3, thresh=NEVER)[0]
    for t, h in enumerate(res.history):
        e, f = eng.energy_forces(h["x"][None], double_positions=True)
        assert DC.same_bits(np.float64(e[0]), np.float64(h["energy"])) and DC.same_bits(np.float64(np.abs(f[0]).max()), np.float64(h["max_force"])), t
        _, curv = eng.hvp(h["x"], h["n"], scheme="forward", return_curvature=True)
        assert abs(h["curv_probe"] - curv[0]) <= 1e-9 * max(1.0, abs(curv[0])), t


# ---- an analytic evaluator on the device ------------------------------------------------------------------------------------------------
class _View:
    """A device buffer as torch can wrap it without a copy."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(int(s) for s in shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


class TorchSurfaceA:
    """Surface A of tests/dimer_cases.py in torch float64 on the GPU behind an ``hvp_dev``-shaped method: forward scheme, float32 forces,
    float64 difference -- what ``umx_hvp_dev`` does, on torch's current stream."""

    def __init__(self, q, dev):
        import torch

        a, base = HC.quadratic(30, 5)
        self.t, self.dev, self.q = torch, dev, q
        self.a, self.base = torch.as_tensor(a, device=dev), torch.as_tensor(base, device=dev)
        self.calls = []

    def _view(self, ptr, shape, typestr="<f8"):
        return self.t.as_tensor(_View(ptr, shape, typestr), device=self.dev)

    def _ef(self, x):
        d = x - self.base[None, :]
        return 0.5 * ((d @ self.a) * d).sum(dim=1) + self.q * (d ** 4).sum(dim=1), -(d @ self.a + 4.0 * self.q * d ** 3)

    def hvp_dev(self, n_bases, d_base, n_dirs, d_dirs, d_hv, base_of=None, step=1e-3, scheme="central", pin=True, d_curv=0, d_e0=0, d_f0=0, stream=0,
                given_f0=False):
        assert scheme == "forward" and n_bases == n_dirs and list(base_of) == list(range(n_dirs)) and d_f0
        self.calls.append((n_bases, given_f0))
        x, d, hv = self._view(d_base, (n_bases, 30)), self._view(d_dirs, (n_dirs, 30)), self._view(d_hv, (n_dirs, 30))
        f0 = self._view(d_f0, (n_bases, 30), "<f4")
        if not given_f0:
            e, f = self._ef(x)
            self._view(d_e0, (n_bases,)).copy_(e)
            f0.copy_(f.to(self.t.float32))
        fp = self._ef(x + step * d)[1].to(self.t.float32)
        hv.copy_(-(fp.to(self.t.float64) - f0.to(self.t.float64)) / step)


def test_the_device_backend_converges_on_an_analytic_evaluator(eng):
    import torch

    _, saddle, a = DC.surface_a(0.5)
    lam = np.linalg.eigvalsh(a)
    max_f, rms_f = D.force_thresholds("gau")
    rng = np.random.default_rng(0)
    x0 = saddle[None] + 0.18 * rng.standard_normal((6, 10, 3))
    n0 = rng.standard_normal((6, 10, 3))
    surf = TorchSurfaceA(0.5, torch.device("cuda", 0))
    res = D.refine_saddles(D.DeviceBackend(eng, evaluator=surf), x0, n0, project="none")
    assert surf.calls[0] == (6, False) and any(given for _, given in surf.calls)
    for i, r in enumerate(res):
        dist, bound = np.abs(r.x - saddle).max(), max_f / np.abs(lam).min()
        print(f"start {i}: {r.reason}, {r.cycles} cycles, {r.images} images, C {r.curvature:.4f} (exact {lam[0]:.4f}), max|x - x*| {dist:.3e} (bound {bound:.3e})")
        assert r.converged and r.cycles <= 40
        assert abs(r.curvature / lam[0] - 1.0) <= 0.02
        assert dist <= bound
    with pytest.raises(ValueError, match="modes0 is needed"):
        D.refine_saddles(D.DeviceBackend(eng, evaluator=surf), x0, None, project="none")


# ---- convergence on the engine ----------------------------------------------------------------------------------------------------------
def test_five_noisy_starts_converge_to_the_fixture_without_a_start_direction(eng, six):
    bind(eng)
    x0 = np.stack([DC.start(s) for s in range(DC.N_STARTS)])
    res = eng.refine_saddles(x0)                                             # one K = 5 call, modes0=None, defaults
    assert eng.pinned_graph() is None
    max_f, rms_f = D.force_thresholds("gau")
    for s, r in enumerate(res):
        dist = np.abs(r.x - DC.X).max()
        e, f = eng.energy_forces(r.x[None], double_positions=True)
        _, curv = eng.hvp(r.x, r.mode, scheme="central", return_curvature=True)
        f = f[0].astype(np.float64)
        print(f"start {s}: {r.reason}, {r.cycles} cycles, {r.images} images, max|x - X| {dist:.4f}, C {r.curvature:.4f}, central {curv[0]:.4f}, "
              f"max|F| {np.abs(f).max():.3e}, rms {np.sqrt((f * f).mean()):.3e}, |mode . fixture's| {abs((r.mode * six['mode']).sum()):.5f}")
        assert r.converged and r.reason == "converged" and r.cycles <= 15
        assert dist <= 0.1 and -0.9 <= r.curvature <= -0.4
        assert np.abs(f).max() <= max_f and np.sqrt((f * f).mean()) <= rms_f   # an independent evaluation meets the thresholds
        assert curv[0] < 0.0                                                 # an independent central product along the mode is negative
        assert DC.same_bits(np.float64(e[0]), np.float64(r.energy)) and DC.same_bits(f.astype(np.float32), r.forces)


def test_verify_reports_one_imaginary_mode(eng, six):
    bind(eng)
    res = eng.refine_saddles(DC.start(0), six["n0"][0], masses=MC.masses_of(DC.Z), verify=True)[0]
    print(f"verify: {res.cycles} cycles, freqs {res.freqs_cm}")
    assert res.converged and res.n_imaginary == 1 and res.freqs_cm.shape == (2,) and res.freqs_cm[0] < 0.0 < res.freqs_cm[1]


def test_refusals_on_the_engine(eng, six):
    bind(eng)
    with eng.pinned(DC.X, double_positions=True):
        with pytest.raises(ValueError, match="a graph is pinned"):
            eng.refine_saddles(six["x0"], six["n0"], **SIX)
    assert eng.pinned_graph() is None
    with pytest.raises(ValueError, match="65 candidates"):
        eng.refine_saddles(np.zeros((65, 12, 3)), np.ones((65, 12, 3)))


# ---- the calculators --------------------------------------------------------------------------------------------------------------------
class FakeAtoms:
    """Minimal ASE-Atoms-like object (as in tests/test_gpu_calculator.py), with masses, a cell and a copy."""

    def __init__(self, z, pos, cell=None, pbc=None):
        self.numbers, self._p, self.info, self.calc = np.asarray(z), np.array(pos, dtype=float), {"charge": 0, "spin": 1}, None
        self.cell, self.pbc = cell, pbc

    def get_positions(self):
        return self._p

    def set_positions(self, p):
        self._p = np.array(p, dtype=float)

    def get_atomic_numbers(self):
        return self.numbers

    def get_masses(self):
        return MC.masses_of(self.numbers)

    def copy(self):
        return FakeAtoms(self.numbers, self._p, self.cell, self.pbc)


def _facades_against_the_engine(eng, z, x, n0, frozen, cell, pbc, max_neigh, monkeypatch, **kw):
    import importlib

    from pdb2reaction_amd import hessian as H, synth
    from pdb2reaction_amd._calculator_base import ANG2BOHR, BOHR2ANG
    from pdb2reaction_amd.ase_calculator import UMXCalculator

    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    bind(eng, cell, pbc, z=z, max_neigh=max_neigh)
    want = eng.refine_saddles(x, n0, frozen=frozen, **kw)[0]
    calc = UMXCalculator(model="synthetic", task_name="omol", max_neigh=max_neigh)
    try:
        atoms = FakeAtoms(z, x, cell, pbc)
        new, got = calc.refine_saddle(atoms, n0, frozen=frozen, **kw)
    finally:
        calc.close()
    assert DC.same_result(got, want) is None, DC.same_result(got, want)
    assert DC.same_bits(new.get_positions(), want.x) and DC.same_bits(atoms.get_positions(), np.array(x, dtype=float))
    U = importlib.import_module("pdb2reaction_amd.uma_pysis")
    up = U.uma_pysis(model="synthetic", max_neigh=max_neigh, freeze_atoms=list(frozen), **({} if cell is None else {"cell": cell, "pbc": pbc}))
    try:
        elem = [synth.SYMBOLS[int(a)] for a in z]
        out = up.get_ts(elem, (x * ANG2BOHR).reshape(-1), n0.reshape(-1), **kw)
    finally:
        up.close()
    bind(eng, cell, pbc, z=z, max_neigh=max_neigh)
    x_in = (x * ANG2BOHR).reshape(-1, 3) * BOHR2ANG                           # the geometry exactly as the facade forms it: then the same bits
    ref = eng.refine_saddles(x_in, n0, frozen=frozen, **kw)[0]
    assert (out["converged"], out["cycles"], out["images"]) == (ref.converged, ref.cycles, ref.images)
    assert DC.same_bits(out["coords"], (ref.x * ANG2BOHR).reshape(-1)) and DC.same_bits(out["mode"], ref.mode.reshape(-1))
    assert DC.same_bits(np.float64(out["energy"]), np.float64(ref.energy * H.EV_TO_HARTREE))
    assert DC.same_bits(np.float64(out["curvature"]), np.float64(ref.curvature * H.EV_PER_ANG2_TO_AU))
    assert DC.same_bits(out["forces"], (H.mask_frozen(ref.forces.astype(np.float64), list(frozen)) * H.EV_PER_ANG_TO_AU).reshape(-1))
    if frozen:
        assert DC.same_bits(want.x[list(frozen)], np.asarray(x)[list(frozen)]) and not want.mode[list(frozen)].any()
        assert DC.same_bits(ref.x[list(frozen)], x_in[list(frozen)])          # (out["coords"] is ref.x in Bohr: held above)
        assert np.abs(want.x - x).max() > 1e-4                               # the others did move
    return want


def test_the_calculators_give_the_engines_result(eng, six, monkeypatch):
    want = _facades_against_the_engine(eng, DC.Z, six["x0"][0], six["n0"][0], (), None, None, DC.MAX_NEIGH, monkeypatch)
    assert want.converged and np.abs(want.x - DC.X).max() <= 0.1


def test_the_calculators_with_two_frozen_atoms(eng, six, monkeypatch):
    _facades_against_the_engine(eng, DC.Z, six["x0"][1], six["n0"][1], (3, 9), None, None, DC.MAX_NEIGH, monkeypatch, **SIX)


def test_the_calculators_in_the_triclinic_cell(eng, weights, monkeypatch):
    c = HC.bases(weights)["triclinic"]
    assert M.resolve_project("auto", True, False) == "t"
    n0 = np.random.default_rng(3).standard_normal((12, 3))
    want = _facades_against_the_engine(eng, c["z"], c["x"], n0, (), c["cell"], c["pbc"], c["max_neigh"], monkeypatch, **SIX)
    assert want.reason == "max_cycles" and not want.converged and want.cycles == 6 and np.isfinite(want.curvature)
    q = M.tr_vectors(c["x"], np.ones(12), np.ones(12, dtype=bool), "t")
    assert len(q) == 3 and np.abs(q @ want.history[0]["n"].reshape(-1)).max() < 1e-12          # the start direction left the translations


def test_a_pool_of_two_engines_on_one_device(weights, six, monkeypatch):
    from pdb2reaction_amd.engine import Engine
    from pdb2reaction_amd.parallel import LocalEnginePool, local_devices_for

    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,0")
    pool = LocalEnginePool.create(local_devices_for(2), weights, engine_factory=Engine)
    try:
        pool.set_system(DC.Z, max_neigh=DC.MAX_NEIGH)
        pool.set_cell(None, None)
        res = pool.refine_saddles(six["x0"], six["n0"], **SIX)
        assert pool.pinned_graph() is None
    finally:
        pool.close()
    for i in range(3):                                                       # the host backend over the pool = the device backend, bit for bit
        assert DC.same_result(res[i], six["res"][i]) is None, (i, DC.same_result(res[i], six["res"][i]))
