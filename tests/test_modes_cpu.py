"""The block Davidson solver of pdb2reaction_amd/modes.py on exact operators, without a GPU: the host backend (the NumPy statements of
the three block kernels) over dense matrices.  With a linear operator the residual is exact, so the eigenvalue error is bounded by the
residual norm and ``tol`` is the bound."""
import math
import os
import re

import numpy as np
import pytest

import hvp_cases as HC
import modes_cases as MC
from pdb2reaction_amd import engine as E
from pdb2reaction_amd import modes as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_AT = 10                                                                    # the 30-dimensional matrices as ten atoms of unit mass
ONES = np.ones(N_AT)
BASE = np.random.default_rng(1).standard_normal((N_AT, 3))
TOL = 1e-9


def solve(a, k, **kw):
    kw.setdefault("project", "none")
    kw.setdefault("tol", TOL)
    return M.lowest_modes(M.HostBackend(M.dense_hvp(a)), BASE, kw.pop("masses", ONES), k, **kw)


MATRICES = {"quadratic": HC.quadratic()[0], "near_degenerate": MC.near_degenerate()}


# ---- the C ABI and its bindings -----------------------------------------------------------------------------------------------------------
def test_the_three_exports_and_their_owners():
    from pdb2reaction_amd import build, parallel as P
    import importlib

    U = importlib.import_module("pdb2reaction_amd.uma_pysis")
    from pdb2reaction_amd.ase_calculator import UMXCalculator

    lib = E.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "umx.h")).read(), flags=re.S)
    for sym, nargs in (("umx_blk_gram_dev", 8), ("umx_blk_combine_dev", 10), ("umx_blk_scale_dev", 7)):
        assert re.search(r"int\s+" + sym + r"\s*\(\s*umx_engine\s*\*", txt), sym
        assert hasattr(lib, sym) and sym in E.EXPORTED_SYMBOLS and len(getattr(lib, sym).argtypes) == nargs
    assert lib.umx_blk_gram_dev(None, 1, None, 1, None, 3, None, None) != 0  # no engine: refused, not a crash
    assert lib.umx_blk_combine_dev(None, 1, None, 1, None, 3, None, 1, None, None) != 0
    assert lib.umx_blk_scale_dev(None, 1, None, None, 3, None, None) != 0
    assert lib.umx_abi_version() == 10                                       # additive: no version bump
    for owner in (E.Engine, P.LocalEnginePool, U.UMAcore, UMXCalculator):
        assert callable(getattr(owner, "lowest_modes")), owner
    assert callable(U.uma_pysis.get_lowest_modes)
    for name in ("blk_gram_dev", "blk_combine_dev", "blk_scale_dev"):
        assert callable(getattr(E.Engine, name))
    assert any(os.path.basename(d) == "umx_rowblocks.h" for d in build.dependencies())


# ---- the NumPy statements of the kernels --------------------------------------------------------------------------------------------------
def test_the_numpy_statements_are_the_sums_they_say():
    x, y = MC.kernel_data(3, 771, 0), MC.kernel_data(5, 771, 1)
    g = M.blk_gram(x, y)
    assert np.abs(g - x @ y.T).max() < 1e-12 and g.shape == (3, 5)
    for a in range(3):                                                       # the order, written out element by element
        part = [0.0] * 256
        for c in range(771):
            part[c % 256] = part[c % 256] + x[a, c] * y[2, c]
        s = 128
        while s:
            for t in range(s):
                part[t] = part[t] + part[t + s]
            s >>= 1
        assert part[0] == g[a, 2]
    gs = M.blk_gram(x, x)
    assert MC.same_bits(gs, gs.T.copy())
    c = np.random.default_rng(2).standard_normal((3, 5))
    out = M.blk_combine(x, c, y, True)
    assert np.abs(out - (y - c.T @ x)).max() < 1e-12
    acc = y[4, 7]
    for i in range(3):
        acc = acc - c[i, 4] * x[i, 7]
    assert acc == out[4, 7]
    assert MC.same_bits(M.blk_combine(x, c, None, False), M.blk_combine(x, c, np.zeros((5, 771)), False))
    w = np.random.default_rng(3).standard_normal(771)
    assert MC.same_bits(M.blk_scale(x, w), w[None, :] * x)


# ---- eigenvalues, residuals, restarts, endings --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("k", [1, 2, 3])
def test_eigenvalues_to_tol_and_honest_residuals(name, k):
    a = MATRICES[name]
    lam, vec = np.linalg.eigh(a)
    res = solve(a, k)
    assert res.converged.all() and res.reason == "converged" and res.eigenvalues.shape == (k,)
    assert np.abs(np.sort(res.eigenvalues) - lam[:k]).max() <= TOL
    again = np.linalg.norm(res.modes_mw @ a.T - res.eigenvalues[:, None] * res.modes_mw, axis=1)
    assert np.abs(again - res.residuals).max() <= 1e-12 and (res.residuals <= TOL).all()
    assert np.abs(np.linalg.norm(res.modes_mw, axis=1) - 1.0).max() < 1e-14
    assert res.images == 2 * res.products and res.iterations >= 1
    if name == "quadratic":
        assert res.n_imaginary == 1 and res.freqs_cm[0] < 0.0
        assert abs(res.freqs_cm[0] + math.sqrt(-res.eigenvalues[0]) * M.FREQ_CM) < 1e-9
    else:                                                                    # the split pair: the SUBSPACE is what is determined
        if k >= 2:
            assert MC.sin_largest_angle(res.modes_mw[:2], vec[:, :2].T) < 1e-6


@pytest.mark.parametrize("name", list(MATRICES))
def test_small_subspace_restarts_and_still_converges(name):
    a = MATRICES[name]
    res = solve(a, 2, block=2, max_subspace=8, max_iter=400)
    assert res.restarts >= 1 and res.converged.all()
    assert np.abs(res.eigenvalues - np.linalg.eigvalsh(a)[:2]).max() <= TOL
    assert res.iterations < res.products <= 2 * res.iterations               # one product call per iteration, of at most `block` directions
    print(f"{name}: {res.iterations} iterations, {res.restarts} restarts")


def test_max_iter_is_reported_not_raised():
    a = MATRICES["quadratic"]
    res = solve(a, 2, block=2, max_subspace=8, max_iter=2)
    assert res.iterations == 2 and not res.converged.any() and res.reason == "max_iter"
    again = np.linalg.norm(res.modes_mw @ a.T - res.eigenvalues[:, None] * res.modes_mw, axis=1)
    assert np.abs(again - res.residuals).max() <= 1e-12 and (res.residuals > TOL).all()


def test_exact_start_vector_converges_in_one_iteration():
    a = MATRICES["quadratic"]
    lam, vec = np.linalg.eigh(a)
    res = solve(a, 1, v0=vec[:, 0][None, :])
    assert res.iterations == 1 and res.converged.all() and abs(res.eigenvalues[0] - lam[0]) <= TOL
    res3 = solve(a, 1, v0=vec[:, 0].reshape(1, N_AT, 3), block=1, max_subspace=4)
    assert res3.iterations == 1 and res3.products == 1 and res3.images == 2


def test_forward_scheme_counts_the_base_once_when_the_callable_takes_it_back():
    a = MATRICES["quadratic"]
    calls = []

    def hvp(base, dirs, step=1e-3, scheme="central", return_base=False, base_forces=None):
        d = np.asarray(dirs)
        calls.append((scheme, return_base, base_forces))
        hv = (d.reshape(len(d), -1) @ a.T).reshape(d.shape)
        return (hv, np.zeros(1), "f0") if return_base else hv

    res = M.lowest_modes(M.HostBackend(hvp), BASE, ONES, 1, project="none", tol=TOL, scheme="forward", block=2, max_subspace=8)
    assert res.converged.all() and res.images == res.products + 1
    assert calls[0] == ("forward", True, None) and all(c == ("forward", False, "f0") for c in calls[1:])
    plain = M.lowest_modes(M.HostBackend(M.dense_hvp(a)), BASE, ONES, 1, project="none", tol=TOL, scheme="forward", block=2, max_subspace=8)
    assert plain.images == plain.products + plain.iterations                # a callable without base_forces pays for the base every time


# ---- projection ----------------------------------------------------------------------------------------------------------------------------
def spring_hessian(x, pairs):
    """The Hessian of sum 1/2 (|xi - xj| - d0)^2 at its minimum: translation and rotation invariant, so six (five) exact zero modes."""
    n = len(x)
    h = np.zeros((3 * n, 3 * n))
    for i, j in pairs:
        e = (x[i] - x[j]) / np.linalg.norm(x[i] - x[j])
        blk = np.outer(e, e)
        for a, b, s in ((i, i, 1), (j, j, 1), (i, j, -1), (j, i, -1)):
            h[3 * a:3 * a + 3, 3 * b:3 * b + 3] += s * blk
    return h


def test_zero_modes_are_absent_and_results_are_orthogonal_to_q():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((6, 3)) * 1.5
    masses = np.array([12.011, 1.008, 15.999, 1.008, 14.007, 12.011])
    h = spring_hessian(x, [(i, j) for i in range(6) for j in range(i)])
    lam, vec, q, _ = MC.dense_reference(h, x, masses)
    assert q.shape == (6, 18) and len(lam) == 12 and lam[0] > 1e-3
    res = M.lowest_modes(M.HostBackend(M.dense_hvp(h)), x, masses, 3, tol=TOL)
    assert res.converged.all() and np.abs(res.eigenvalues - lam[:3]).max() <= TOL          # the six zero modes do not appear
    assert np.abs(res.modes_mw @ q.T).max() <= 1e-12
    # without the projection the zero modes ARE the lowest: the projector is what keeps them out
    raw = M.lowest_modes(M.HostBackend(M.dense_hvp(h)), x, masses, 3, tol=TOL, project="none")
    assert np.abs(raw.eigenvalues).max() < 1e-8
    # the Cartesian modes: w * u normalised
    w = MC.weights_vector(masses)
    cart = w[None, :] * res.modes_mw
    assert np.abs(res.modes.reshape(3, -1) - cart / np.linalg.norm(cart, axis=1)[:, None]).max() < 1e-14


def test_linear_molecule_has_rank_five():
    x = np.array([[0.0, 0.0, -1.16], [0.0, 0.0, 0.0], [0.0, 0.0, 1.16]])
    masses = np.array([15.999, 12.011, 15.999])
    assert M.tr_vectors(x, masses, np.ones(3, dtype=bool), "tr").shape == (5, 9)
    assert M.tr_vectors(x, masses, np.ones(3, dtype=bool), "t").shape == (3, 9)
    assert M.tr_vectors(x, masses, np.ones(3, dtype=bool), "none").shape == (0, 9)
    h = spring_hessian(x, [(0, 1), (1, 2)])
    lam, _, q, _ = MC.dense_reference(h, x, masses)
    assert len(q) == 5 and len(lam) == 4
    res = M.lowest_modes(M.HostBackend(M.dense_hvp(h)), x, masses, 2, tol=TOL)
    assert res.converged.all() and np.abs(res.eigenvalues - lam[:2]).max() <= TOL and np.abs(res.modes_mw @ q.T).max() <= 1e-12


def test_frozen_rows_are_exactly_zero():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((7, 3)) * 1.5
    masses = rng.uniform(1.0, 16.0, size=7)
    h = spring_hessian(x, [(i, j) for i in range(7) for j in range(i)]) + 0.05 * np.eye(21)
    frozen = [2, 5]
    for project, periodic in (("auto", False), ("auto", True), ("t", True)):
        how = M.resolve_project(project, periodic, True)
        lam, _, q, _ = MC.dense_reference(h, x, masses, frozen, how)
        res = M.lowest_modes(M.HostBackend(M.dense_hvp(h)), x, masses, 2, frozen=frozen, project=project, periodic=periodic, tol=TOL)
        assert res.converged.all() and np.abs(res.eigenvalues - lam[:2]).max() <= TOL, (project, periodic)
        assert not res.modes[:, frozen, :].any() and not res.modes_mw.reshape(2, 7, 3)[:, frozen, :].any()
        assert not q.reshape(len(q), 7, 3)[:, frozen, :].any()              # Q lives on the active atoms
    assert (M.resolve_project("auto", False, True), M.resolve_project("auto", True, False), M.resolve_project("auto", True, True)) == ("tr", "t", "none")


def test_refusals():
    a = MATRICES["quadratic"]
    for kw, pattern in ((dict(project="rt"), "project must be"), (dict(scheme="backward"), "scheme must be"), (dict(step=0.0), "step must be"),
                        (dict(block=2, max_subspace=2), "max_subspace"), (dict(max_subspace=65), "max_subspace"), (dict(frozen=[10]), "frozen atom"),
                        (dict(masses=np.ones(9)), "masses must be"), (dict(v0=np.ones(7)), "v0 must be")):
        with pytest.raises(ValueError, match=pattern):
            solve(a, 1, **kw)
    with pytest.raises(ValueError, match="k = 40"):
        solve(a, 40)


# ---- the pin --------------------------------------------------------------------------------------------------------------------------------
class Pinner:
    def __init__(self, pinned=None):
        self.state, self.log = pinned, []

    def pinned_graph(self):
        return self.state

    def pin_graph(self, x, double_positions=False):
        self.log.append(("pin", np.array(x), double_positions))
        self.state = (1, 1)

    def unpin_graph(self):
        self.log.append(("unpin",))
        self.state = None


def test_the_solver_pins_once_and_unpins_on_every_way_out():
    a = MATRICES["quadratic"]
    p = Pinner()
    M.lowest_modes(M.HostBackend(M.dense_hvp(a), pinner=p), BASE, ONES, 1, project="none", tol=TOL)
    assert [e[0] for e in p.log] == ["pin", "unpin"] and p.log[0][2] is True and np.array_equal(p.log[0][1], BASE) and p.state is None

    def broken(base, dirs, step=1e-3, scheme="central"):
        raise RuntimeError("boom")

    p = Pinner()
    with pytest.raises(RuntimeError, match="boom"):
        M.lowest_modes(M.HostBackend(broken, pinner=p), BASE, ONES, 1, project="none")
    assert [e[0] for e in p.log] == ["pin", "unpin"] and p.state is None
    held = Pinner(pinned=(48, 4))                                            # a caller's pin is used and left in place
    M.lowest_modes(M.HostBackend(M.dense_hvp(a), pinner=held), BASE, ONES, 1, project="none", tol=TOL)
    assert held.log == [] and held.state == (48, 4)


# ---- the constant ---------------------------------------------------------------------------------------------------------------------------
def test_the_wavenumber_constant_against_its_derivation():
    # sqrt(eV / (A^2 amu)) as an angular frequency, over 2 pi c in cm/s -- CODATA-2018, written out here a second time
    ev, amu, c_cm = 1.602176634e-19, 1.66053906660e-27, 2.99792458e10
    omega = math.sqrt(ev / (1e-20 * amu))
    assert abs(M.FREQ_CM / (omega / (2.0 * math.pi * c_cm)) - 1.0) < 1e-12
    assert f"{M.FREQ_CM:.2f}" == "521.47" and abs(M.FREQ_CM / 521.47 - 1.0) < 1e-5
