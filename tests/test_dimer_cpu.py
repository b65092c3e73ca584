"""The batched dimer of pdb2reaction_amd/dimer.py without a GPU: the host backend (the NumPy statements of the row kernels) over
analytic surfaces and over the float64 checker of the synthetic model, whose forces are rounded to float32 as the engine's are.

Bounds.  Convergence within 40 cycles on the analytic surfaces: three times what was measured when the algorithm was first run (<= 10 on
surface A, <= 12 on surface B), because the step rule may round differently in another statement of it.  The curvature within 2 % of the
exact one.  Distance to the saddle: near a stationary point F = -H (x - x*), so a force component of at most max_force leaves a coordinate
at most max_force / min|lambda| away along an eigenvector; the largest coordinate difference is held to that figure.  On the checker: 15 cycles,
0.1 A, C in [-0.9, -0.4] -- the checker's own figures (3-4 cycles here, 0.037 A, -0.70 ... -0.57; tests/dimer_cases.py) with a three- to
five-fold margin."""
import numpy as np
import pytest

import dimer_cases as DC
from pdb2reaction_amd import dimer as D
from pdb2reaction_amd import modes as M


# ---- the NumPy statements of the kernels ------------------------------------------------------------------------------------------------
def test_the_numpy_statements_are_the_sums_they_say():
    import modes_cases as MC

    x, y = MC.kernel_data(5, 771, 0), MC.kernel_data(5, 771, 1)
    d = D.row_dot(x, y)
    assert d.shape == (5,) and np.abs(d - (x * y).sum(axis=1)).max() < 1e-12
    assert DC.same_bits(d, np.diag(M.blk_gram(x, y)).copy())                  # the diagonal of the block kernel's statement
    for r in (0, 4):                                                         # the order, written out element by element
        part = [0.0] * 256
        for c in range(771):
            part[c % 256] = part[c % 256] + x[r, c] * y[r, c]
        s = 128
        while s:
            for t in range(s):
                part[t] = part[t] + part[t + s]
            s >>= 1
        assert part[0] == d[r]
    a, b = np.array([1.5, -0.0, 2.0, -3.0, 0.1]), np.array([0.3, 1.0, -0.0, 7.0, -0.1])
    out = D.row_axpby(a, x, b, y)
    assert out[3, 5] == (a[3] * x[3, 5]) + (b[3] * y[3, 5]) and DC.same_bits(D.row_axpby(a, x), a[:, None] * x)
    with pytest.raises(ValueError):
        D.row_axpby(a, x, b, None)
    m = D.row_absmax(x)
    assert DC.same_bits(m, np.abs(x).max(axis=1)) and m[1] == 0.0
    x[2, 700] = np.nan
    assert np.isnan(D.row_absmax(x)[2]) and np.isfinite(D.row_absmax(x)[[0, 1, 3, 4]]).all()


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(weights):
    """Computed once and left unchanged: the checker's surface, its forces and Hessian eigenpairs at the fixture."""
    from pdb2reaction_amd import synth

    ef, orc = DC.checker_surface(weights)
    assert list(synth.make_cluster(12, seed=4)[0]) == DC.Z and orc.max_neigh is None and DC.MAX_NEIGH >= len(DC.Z) - 1
    e, f = ef(DC.X)
    lam, vec = np.linalg.eigh(DC.fd_hessian(ef, DC.X))
    return dict(ef=ef, f=f, lam=lam, mode=vec[:, 0].reshape(12, 3))


def test_the_fixture_is_a_first_order_saddle_of_the_checker(checker):
    lam = checker["lam"]
    print(f"max|F| {np.abs(checker['f']).max():.3e}; eigenvalues {lam[:9]} ... {lam[-1]:.3f}")
    assert np.abs(checker["f"]).max() <= 3e-3
    assert (lam < -0.1).sum() == 1 and not ((lam > -0.1) & (lam < -1e-3)).any()


# ---- analytic surfaces ------------------------------------------------------------------------------------------------------------------
def held_to_the_saddle(res, saddle, hess, max_f, rms_f, what):
    lam = np.linalg.eigvalsh(hess)
    n = saddle.size
    assert res.converged and res.reason == "converged" and res.cycles <= 40, (what, res.reason, res.cycles)
    assert abs(res.curvature / lam[0] - 1.0) <= 0.02, (what, res.curvature, lam[0])
    assert res.max_force <= max_f and res.rms_force <= rms_f and res.curvature < 0.0
    assert res.cycles == len(res.history) and res.images >= 2 * res.cycles
    assert abs(np.linalg.norm(res.mode) - 1.0) < 1e-12
    dist = np.abs(res.x - saddle).max()
    bound = max_f / np.abs(lam).min()
    print(f"{what}: {res.cycles} cycles, {res.images} images, C {res.curvature:.4f} (exact {lam[0]:.4f}), max|x - x*| {dist:.3e} (bound {bound:.3e})")
    assert dist <= bound, (what, dist, bound)
    return n


@pytest.mark.parametrize("q", [0.0, 0.5])
def test_surface_a_converges_from_random_starts_and_random_directions(q):
    ef, saddle, a = DC.surface_a(q)
    max_f, rms_f = D.force_thresholds("gau")
    assert abs(max_f - 2.314e-2) < 1e-5 and abs(rms_f - 1.543e-2) < 1e-5 and np.allclose((max_f, rms_f), DC.GAU, rtol=1e-12)
    for s in range(12):
        rng = np.random.default_rng(s)
        x0 = saddle + 0.18 * rng.standard_normal((10, 3))
        res = D.refine_saddles(D.HostBackend(DC.fd_hvp(ef)), x0, rng.standard_normal((10, 3)), project="none")[0]
        held_to_the_saddle(res, saddle, a, max_f, rms_f, f"A q={q} start {s}")


def test_surface_b_converges():
    ef, saddle, hess = DC.surface_b()
    max_f, rms_f = D.force_thresholds("gau")
    for s in range(4):
        rng = np.random.default_rng(s)
        x0 = saddle + 0.1 * rng.standard_normal((12, 3))
        res = D.refine_saddles(D.HostBackend(DC.fd_hvp(ef)), x0, rng.standard_normal((12, 3)), project="none")[0]
        held_to_the_saddle(res, saddle, hess, max_f, rms_f, f"B start {s}")


def test_a_batch_is_its_singles_bit_for_bit_and_costs_what_it_says():
    ef, saddle, _ = DC.surface_a(0.5)
    rng = np.random.default_rng(9)
    x0 = saddle[None] + 0.18 * rng.standard_normal((3, 10, 3))
    n0 = rng.standard_normal((3, 10, 3))
    log = []
    batch = D.refine_saddles(D.HostBackend(DC.fd_hvp(ef, log)), x0, n0, project="none")
    assert len({r.cycles for r in batch}) > 1                                # candidates leave the batch at different cycles
    for i in range(3):
        single = D.refine_saddles(D.HostBackend(DC.fd_hvp(ef)), x0[i], n0[i], project="none")[0]
        assert DC.same_result(batch[i], single) is None, i
        rot = sum(h["rotations"] for h in batch[i].history)
        assert batch[i].images == 2 * batch[i].cycles + rot                  # a base and a probe per cycle, one image per rotation
        assert all(0 <= h["rotations"] <= 2 and 0.0 <= h["step_max"] <= 0.1 for h in batch[i].history)
        assert batch[i].history[-1]["step_max"] == 0.0                       # no step after the converged evaluation
    assert all(bases == dirs for bases, dirs, _ in log)                      # one base per direction: base_of = arange
    assert max(b for b, _, _ in log) == 3 and any(given for _, _, given in log) and not log[0][2]


def test_endings_are_reported_per_candidate():
    ef, saddle, _ = DC.surface_a(0.5)
    rng = np.random.default_rng(3)
    x0 = saddle[None] + 0.18 * rng.standard_normal((2, 10, 3))
    n0 = rng.standard_normal((2, 10, 3))
    res = D.refine_saddles(D.HostBackend(DC.fd_hvp(ef)), x0, n0, project="none", max_cycles=2)
    assert [r.reason for r in res] == ["max_cycles", "max_cycles"] and not any(r.converged for r in res) and all(r.cycles == 2 for r in res)

    def poisoned(x):                                                         # not a number beyond a wall that only candidate 1 starts behind
        e, f = ef(x)
        return (np.nan, f * np.nan) if x[0, 0] > saddle[0, 0] + 5.0 else (e, f)

    x0[1, 0, 0] = saddle[0, 0] + 6.0
    res = D.refine_saddles(D.HostBackend(DC.fd_hvp(poisoned)), x0, n0, project="none")
    assert res[1].reason == "non_finite" and not res[1].converged and res[1].cycles == 1
    assert res[0].converged                                                  # the other candidate goes on


def test_frozen_rows_never_move_and_the_projection_is_kept():
    ef, saddle, a = DC.surface_a(0.0)
    rng = np.random.default_rng(5)
    x0 = saddle + 0.05 * rng.standard_normal((10, 3))
    res = D.refine_saddles(D.HostBackend(DC.fd_hvp(ef)), x0, rng.standard_normal((10, 3)), frozen=[2, 7], project="none", max_cycles=5, thresh=(1e-9, 1e-9))[0]
    assert DC.same_bits(res.x[[2, 7]], x0[[2, 7]]) and not res.mode[[2, 7]].any() and res.cycles == 5
    assert all(not h["n"][[2, 7]].any() for h in res.history)
    res = D.refine_saddles(D.HostBackend(DC.fd_hvp(ef)), x0, rng.standard_normal((10, 3)), project="tr", max_cycles=3, thresh=(1e-9, 1e-9))[0]
    q = M.tr_vectors(x0, np.ones(10), np.ones(10, dtype=bool), "tr")         # the start direction leaves the translations and rotations of x0
    assert len(q) == 6 and np.abs(q @ res.history[0]["n"].reshape(-1)).max() < 1e-12 and DC.same_bits(res.history[0]["x"], x0)
    assert abs(np.linalg.norm(res.history[0]["n"]) - 1.0) < 1e-12


# ---- the checker's surface --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1, 2])
def test_the_checker_surface_reconverges_to_the_fixture(checker, s):
    res = D.refine_saddles(D.HostBackend(DC.fd_hvp(checker["ef"])), DC.start(s), DC.noisy_mode(checker["mode"], s))[0]
    dist = np.abs(res.x - DC.X).max()
    print(f"start {s}: {res.reason}, {res.cycles} cycles, {res.images} images, max|x - X| {dist:.4f}, C {res.curvature:.4f}, "
          f"|mode . exact| {abs((res.mode * checker['mode']).sum()):.5f}")
    assert res.converged and res.cycles <= 15
    assert dist <= 0.1 and -0.9 <= res.curvature <= -0.4


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
class Pinner:
    def __init__(self, pinned=None):
        self.state = pinned

    def pinned_graph(self):
        return self.state


def test_refusals():
    ef, saddle, _ = DC.surface_a(0.0)
    hvp = DC.fd_hvp(ef)
    n0 = np.ones((10, 3))
    go = lambda x0, m0=n0, be=None, **kw: D.refine_saddles(be or D.HostBackend(hvp), x0, m0, project="none", **kw)   # noqa: E731
    with pytest.raises(ValueError, match="65 candidates"):
        go(np.zeros((65, 10, 3)), np.ones((65, 10, 3)))
    with pytest.raises(ValueError, match="a graph is pinned"):
        go(saddle, be=D.HostBackend(hvp, pinner=Pinner((48, 4))))
    bad = np.stack([saddle, saddle, saddle])
    bad[2, 4, 1] = np.inf
    with pytest.raises(ValueError, match=r"non-finite position \(candidate 2\)"):
        go(bad, np.ones((3, 10, 3)))
    m0 = np.ones((3, 10, 3))
    m0[1, 0, 0] = np.nan
    with pytest.raises(ValueError, match=r"modes0 \(candidate 1\)"):
        go(np.stack([saddle] * 3), m0)
    for kw, pattern in ((dict(step=0.0), "step must be"), (dict(thresh="loose"), "thresh must be"), (dict(frozen=[10]), "frozen atom"),
                        (dict(max_step=-1.0), "max_step"), (dict(verify=True), "needs masses")):
        with pytest.raises(ValueError, match=pattern):
            go(saddle, **kw)
    with pytest.raises(ValueError, match="modes0 must hold"):
        go(saddle, np.ones((2, 10, 3)))
    with pytest.raises(ValueError, match="vanishes under the projection"):
        go(saddle, np.zeros((10, 3)))
    with pytest.raises(ValueError, match="project must be"):
        D.refine_saddles(D.HostBackend(hvp), saddle, n0, project="rt")
