"""The block Davidson solver on the engine (``Engine.lowest_modes``, pdb2reaction_amd/modes.py): the three bases of tests/hvp_cases.py,
k = 2, block = 2, max_subspace = 8 -- small enough that restarts must happen --, step 1e-3 A, central, the masses of tests/modes_cases.py.

Yardstick.  The dense matrix B = W H_fd W whose columns are ``Engine.hvp(base, e_k)`` under the same pin, projected in NumPy float64
and symmetrised; its sorted eigenpairs on range(P) are the reference.  Its own noise is measured here: asym = ||(B - B^T) / 2||_2 -- a
true Hessian is symmetric, so the antisymmetric part of the finite-difference one estimates the error of its symmetric part.  The solver
runs with tol = 4 asym and is held to |theta_i - lambda_i| <= tol + 4 asym and, for the subspace (the first two eigenvalues of
``triclinic`` are 0.04 apart: single vectors are not determined), sin(largest principal angle) <= 2 (tol + 4 asym) / (lambda_{k+1} -
lambda_k) (Davis-Kahan).  The yardstick bites only when lambda_{k+1} - lambda_k > 4 (tol + 4 asym): asserted for every base.
Figures: profiles/lowest_modes.txt.  Synthetic weights seed 0; 12 atoms; a dense matrix is 72 images, a solve a few hundred."""
import numpy as np
import pytest

import hvp_cases as HC
import modes_cases as MC
from pdb2reaction_amd import modes as M

pytestmark = pytest.mark.gpu

KW = dict(block=MC.BLOCK, max_subspace=MC.MAX_SUBSPACE, step=MC.STEP, scheme="central")
K_OF = {"swap": MC.K, "odd47": MC.K, "triclinic": MC.K}                      # lowered for a base only where its gap condition fails


def new_engine(weights):
    from pdb2reaction_amd.engine import Engine

    e = Engine(0)
    e.load_weights(weights)
    return e


def bind(e, c):
    e.set_system(c["z"], max_neigh=c["max_neigh"])
    e.set_cell(c["cell"], c["pbc"])


@pytest.fixture(scope="module")
def eng(weights):
    e = new_engine(weights)
    yield e
    e.close()


@pytest.fixture(scope="module")
def solved(weights, eng):
    """Computed once and left unchanged: name -> dict(case, masses, project, dense eigenpairs, Q, asym, tol, the device backend's result)."""
    out = {}
    for name, c in HC.bases(weights).items():
        bind(eng, c)
        n = 3 * len(c["z"])
        masses = MC.masses_of(c["z"])
        how = M.resolve_project("auto", c["cell"] is not None, False)
        with eng.pinned(c["x"], double_positions=True):
            h = eng.hvp(c["x"], np.eye(n).reshape(n, -1, 3), step=MC.STEP).reshape(n, n).T      # column k = hvp(e_k)
        w = MC.weights_vector(masses)
        b = w[:, None] * h * w[None, :]
        asym = float(np.linalg.norm(0.5 * (b - b.T), 2))
        lam, vec, q, _ = MC.dense_reference(h, c["x"], masses, project=how)
        res = eng.lowest_modes(c["x"], masses, K_OF[name], tol=4.0 * asym, **KW)
        pin_after = eng.pinned_graph()
        out[name] = dict(c=c, masses=masses, how=how, h=h, lam=lam, vec=vec, q=q, asym=asym, tol=4.0 * asym, res=res, pin_after=pin_after)
    return out


@pytest.mark.parametrize("name", ["swap", "odd47", "triclinic"])
def test_the_lowest_pairs_against_the_dense_finite_difference_matrix(eng, solved, name):
    s = solved[name]
    res, lam, vec, asym, tol, k = s["res"], s["lam"], s["vec"], s["asym"], s["tol"], K_OF[name]
    bound = tol + 4.0 * asym
    gap = lam[k] - lam[k - 1]
    err = np.abs(res.eigenvalues - lam[:k])
    sin = MC.sin_largest_angle(res.modes_mw, vec[:k])
    print(f"{name}: asym {asym:.3e}, tol {tol:.3e}, lambda {lam[:k + 1]}, gap {gap:.4f} (needs > {4 * bound:.3e}); {res.iterations} iterations, "
          f"{res.restarts} restarts, {res.images} images; residuals {res.residuals}; |theta - lambda| {err} (bound {bound:.3e}); sin {sin:.3e} "
          f"(bound {2 * bound / gap:.3e})")
    assert s["how"] == ("t" if name == "triclinic" else "tr") and len(s["q"]) == (3 if name == "triclinic" else 6)
    assert gap > 4.0 * bound                                                 # the gap condition: the yardstick bites
    assert res.converged.all() and res.reason == "converged" and (res.residuals <= tol).all()
    assert res.restarts >= 1
    assert (err <= bound).all()
    assert sin <= 2.0 * bound / gap
    assert s["pin_after"] is None                                            # the solver's own pin is gone
    assert np.abs(res.modes_mw @ s["q"].T).max() <= 1e-12                    # the zero modes are not among the results
    assert res.images == 2 * res.products and res.iterations < res.products <= MC.BLOCK * res.iterations


@pytest.mark.parametrize("name", ["swap", "odd47", "triclinic"])
def test_an_independent_residual(eng, solved, name):
    """One ``Engine.hvp`` plus NumPy per returned pair: ||A u - theta u|| <= 2 tol."""
    s = solved[name]
    c, res, q = s["c"], s["res"], s["q"]
    bind(eng, c)
    w = MC.weights_vector(s["masses"])
    proj = lambda u: u - (u @ q.T) @ q                                       # noqa: E731
    u = proj(res.modes_mw)
    hv = eng.hvp(c["x"], (w[None, :] * u).reshape(len(u), -1, 3), step=MC.STEP).reshape(len(u), -1)
    au = proj(w[None, :] * hv)
    rn = np.linalg.norm(au - res.eigenvalues[:, None] * res.modes_mw, axis=1)
    print(f"{name}: independent residuals {rn}, reported {res.residuals}, 2 tol = {2 * s['tol']:.3e}")
    assert (rn <= 2.0 * s["tol"]).all()


def test_both_backends_give_the_same_bits(eng, solved):
    s = solved["swap"]
    bind(eng, s["c"])
    host = M.lowest_modes(M.HostBackend(eng.hvp, pinner=eng), s["c"]["x"], s["masses"], K_OF["swap"], tol=s["tol"], **KW)
    assert eng.pinned_graph() is None
    assert MC.same_result(host, s["res"])


def test_the_pin_on_every_way_out_and_under_a_callers_pin(eng, solved, monkeypatch):
    s = solved["swap"]
    c = s["c"]
    bind(eng, c)
    with eng.pinned(c["x"], double_positions=True):                          # a caller's pin is used and left in place
        before = eng.pinned_graph()
        res = eng.lowest_modes(c["x"], s["masses"], K_OF["swap"], tol=s["tol"], **KW)
        assert eng.pinned_graph() == before and before is not None
    assert eng.pinned_graph() is None and MC.same_result(res, s["res"])       # the same graph: the same bits
    calls = []

    def boom(*a, **kw):
        calls.append(eng.pinned_graph())
        raise RuntimeError("boom")

    monkeypatch.setattr(eng, "hvp_dev", boom)
    with pytest.raises(RuntimeError, match="boom"):
        eng.lowest_modes(c["x"], s["masses"], K_OF["swap"], tol=s["tol"], **KW)
    assert calls and calls[0] is not None and eng.pinned_graph() is None      # pinned when the product was asked for, unpinned after the raise


def test_a_pool_of_two_engines_on_one_device(weights, solved, monkeypatch):
    from pdb2reaction_amd.engine import Engine
    from pdb2reaction_amd.parallel import LocalEnginePool, local_devices_for

    s = solved["swap"]
    c = s["c"]
    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,0")
    pool = LocalEnginePool.create(local_devices_for(2), weights, engine_factory=Engine)
    try:
        pool.set_system(c["z"], max_neigh=c["max_neigh"])
        pool.set_cell(c["cell"], c["pbc"])
        res = pool.lowest_modes(c["x"], s["masses"], K_OF["swap"], tol=s["tol"], **KW)
        assert pool.pinned_graph() is None and pool.last_route in ("batch", "single")
    finally:
        pool.close()
    assert MC.same_result(res, s["res"])                                     # the host backend over the pool = the device backend, bit for bit


class FakeAtoms:
    """Minimal ASE-Atoms-like object (as in tests/test_gpu_calculator.py), with masses."""

    def __init__(self, z, pos, masses):
        self.numbers, self._p, self._m, self.info, self.calc = np.asarray(z), np.asarray(pos, dtype=float), masses, {"charge": 0, "spin": 1}, None

    def get_positions(self):
        return self._p

    def get_atomic_numbers(self):
        return self.numbers

    def get_masses(self):
        return self._m


def test_the_calculators(eng, solved, monkeypatch):
    """``UMXCalculator.lowest_modes`` and ``uma_pysis.get_lowest_modes`` on engines of their own against ``Engine.lowest_modes``."""
    import importlib

    from pdb2reaction_amd import hessian as H, synth
    from pdb2reaction_amd._calculator_base import ANG2BOHR, BOHR2ANG
    from pdb2reaction_amd.ase_calculator import UMXCalculator

    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    s = solved["swap"]
    c, masses, tol = s["c"], s["masses"], s["tol"]
    calc = UMXCalculator(model="synthetic", task_name="omol")
    try:
        got = calc.lowest_modes(FakeAtoms(c["z"], c["x"], masses), 1, tol=tol, block=2, max_subspace=8)
    finally:
        calc.close()
    eng.set_system(c["z"])                                                   # the calculator's defaults: no cap
    eng.set_cell(None, None)
    assert MC.same_result(got, eng.lowest_modes(c["x"], masses, 1, tol=tol, block=2, max_subspace=8))
    U = importlib.import_module("pdb2reaction_amd.uma_pysis")
    frozen = [1, 4]
    up = U.uma_pysis(model="synthetic", max_neigh=c["max_neigh"], freeze_atoms=frozen)
    try:
        elem = [synth.SYMBOLS[int(a)] for a in c["z"]]
        out = up.get_lowest_modes(elem, (c["x"] * ANG2BOHR).reshape(-1), 1, masses, tol=tol * H.EV_PER_ANG2_TO_AU, block=2, max_subspace=8)
    finally:
        up.close()
    bind(eng, c)
    # the geometry and the threshold exactly as the facade forms them (Bohr -> A, Hartree/Bohr^2 -> eV/A^2): then the same bits
    want = eng.lowest_modes((c["x"] * ANG2BOHR).reshape(-1, 3) * BOHR2ANG, masses, 1, frozen=frozen, tol=float(tol * H.EV_PER_ANG2_TO_AU) / H.EV_PER_ANG2_TO_AU,
                            block=2, max_subspace=8)
    assert want.converged.all() and out["converged"].all() and out["images"] == want.images
    assert MC.same_bits(out["eigenvalues"], want.eigenvalues * H.EV_PER_ANG2_TO_AU) and MC.same_bits(out["freqs_cm"], want.freqs_cm)
    assert MC.same_bits(out["modes"], want.modes.reshape(1, -1)) and MC.same_bits(out["residuals"], want.residuals * H.EV_PER_ANG2_TO_AU)
    assert not out["modes"].reshape(1, -1, 3)[:, frozen, :].any() and out["modes"].any()
