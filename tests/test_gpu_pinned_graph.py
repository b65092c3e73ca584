"""The pinned neighbour graph on the GPU (``umx_pin_graph``): evaluate displaced geometries on the edge set of one reference image.

Two yardsticks.  Exact: pinned at a reference, an evaluation of that reference is the unpinned one in every bit of E, F, W and of the
graph buffers; a pinned plan stands to the pinned one-piece plan as the unpinned plan stands to the unpinned one-piece plan.  Float64:
``PeriodicOracle.model_energy(graph=...)`` (tests/pinned_cases.py) -- the checker on the reference's graph held fixed -- at the project's
bounds |dE| <= 1e-4 eV, max|dF| <= 1e-3 eV/A; where a test differences energies its bound is the checker's own error doing the same
difference plus 2 TOL_E / (2 h) for the engine's energy error, computed in the test and printed (profiles/pinned_graph.txt records them).

Synthetic weights seed 0, default precision.  Every case is a handful of evaluations of at most 48 atoms."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import pinned_cases as PC
from stress_oracle import make_case, strain_derivative
from test_gpu_periodic import TOL_E, TOL_F
from pdb2reaction_amd import hessian as H
from pdb2reaction_amd import synth
from pdb2reaction_amd.engine import UmxError

pytestmark = pytest.mark.gpu

U = importlib.import_module("pdb2reaction_amd.uma_pysis")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_efw(a, b):
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


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


def lib_pinned(e):
    """(edges, max degree) straight from ``umx_pinned_graph``: zeros when nothing is pinned."""
    ne, md = C.c_int64(-1), C.c_int32(-1)
    assert e.lib.umx_pinned_graph(e._h, C.byref(ne), C.byref(md)) == 0
    return int(ne.value), int(md.value)


def cluster(n, seed):
    z, pos = synth.make_cluster(n, seed=seed)
    return z, pos.astype(np.float32)


# ---- 1. pinned at the reference is the unpinned evaluation -----------------------------------------------------------------------------
@pytest.mark.parametrize("double", [False, True], ids=["float", "double"])
@pytest.mark.parametrize("name,max_neigh", [("open", None), ("open", 6), ("triclinic", None), ("triclinic", 7), ("slab", None)])
def test_pinned_at_the_reference_is_the_unpinned_evaluation(eng, name, max_neigh, double):
    if name == "open":
        (z, x), cell, pbc = cluster(20, 3), None, None
    else:
        z, imgs, cell, pbc = make_case(name)
        x = imgs[0]
    if double:      # float64 positions that float32 does not hold: the double entry's own differences
        x = x.astype(np.float64) + 1e-6 * np.random.default_rng(1).standard_normal(x.shape)
    kw = {"double_positions": True} if double else {}
    x3 = np.stack([x, x, x])
    eng.set_system(z, max_neigh=max_neigh)
    eng.set_cell(cell, pbc)
    eng.debug_keep(True)

    def run():
        out = eng.energy_forces_virial(x3, **kw)
        return out, (eng.debug_fetch("src", np.int32), eng.debug_fetch("dst", np.int32), eng.debug_fetch("evec", np.float32)), eng.graph_stats()

    free, g_free, stats = run()
    assert eng.pinned_graph() is None and lib_pinned(eng) == (0, 0)
    eng.pin_graph(x, **kw)
    assert stats[0] % 3 == 0 and eng.pinned_graph() == (stats[0] // 3, stats[1]) == lib_pinned(eng)
    if max_neigh is not None:
        assert stats[1] == max_neigh                                         # the cap binds: the truncating fill built the reference
    pinned, g_pin, stats_pin = run()
    assert stats_pin == stats and len(g_free[0]) == stats[0] and len(g_free[2]) == 4 * stats[0]
    assert same_efw(pinned, free), (name, max_neigh, double)
    for a, b, what in zip(g_pin, g_free, ("src", "dst", "evec")):
        assert same_bits(a, b), (what, name, max_neigh, double)
    eng.unpin_graph()
    assert eng.pinned_graph() is None and lib_pinned(eng) == (0, 0)
    again, g_again, _ = run()
    assert same_efw(again, free) and all(same_bits(a, b) for a, b in zip(g_again, g_free))
    eng.debug_keep(False)


# ---- 2. the rank swap, 3. a difference across it ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def swaps(weights):
    """Both swap cases with the checker's figures, computed once: name -> dict."""
    out = {}
    for name in ("cluster", "triclinic"):
        if name == "cluster":
            z, orc, x0, xm, xs, u, j = PC.cluster_swap(weights)
            cell = pbc = None
        else:
            z, orc, cell, pbc, x0, xm, xs, u, j = PC.triclinic_swap(weights)
        g0, gm = PC.graph_of(orc, x0), PC.graph_of(orc, xm)
        fixed, rebuilt = PC.energy_forces_on(orc, z, xm, g0), PC.energy_forces_on(orc, z, xm, None)
        h = PC.FD_H
        xp, xn = xs.copy(), xs.copy()
        xp[j] += h * u
        xn[j] -= h * u
        fd = (PC.energy_on(orc, z, xp, g0) - PC.energy_on(orc, z, xn, g0)) / (2 * h)
        analytic = -float(PC.energy_forces_on(orc, z, xs, g0)[1][j] @ u)
        out[name] = dict(z=z, orc=orc, cell=cell, pbc=pbc, x0=x0, xm=xm, xs=xs, xp=xp, xn=xn, u=u, j=j, g0=g0, gm=gm, fixed=fixed,
                         rebuilt=rebuilt, fd=fd, analytic=analytic)
    return out


@pytest.mark.parametrize("name", ["cluster", "triclinic"])
def test_the_rank_swap(eng, swaps, name):
    s = swaps[name]
    # preconditions (asserted, not skipped): the rebuilt graph at the moved geometry is another one, and it matters
    assert not PC.same_graph(s["g0"], s["gm"])
    de_graphs, df_graphs = abs(s["fixed"][0] - s["rebuilt"][0]), float(np.abs(s["fixed"][1] - s["rebuilt"][1]).max())
    print(f"[swap {name}] the two checkers differ by |dE| = {de_graphs:.4f} eV  max|dF| = {df_graphs:.4f} eV/A")
    assert de_graphs > 100 * TOL_E and df_graphs > 100 * TOL_F
    eng.set_system(s["z"], max_neigh=PC.MAX_NEIGH)
    eng.set_cell(s["cell"], s["pbc"])
    eng.pin_graph(s["x0"])
    assert eng.pinned_graph() == (len(s["g0"][0]), PC.MAX_NEIGH)
    e, f = eng.energy_forces(s["xm"])
    de, df = abs(e[0] - s["fixed"][0]), float(np.abs(f[0] - s["fixed"][1]).max())
    print(f"[swap {name}] pinned against the checker on the start graph: |dE| = {de:.3e} eV  max|dF| = {df:.3e} eV/A")
    assert de <= TOL_E and df <= TOL_F
    eng.unpin_graph()
    e, f = eng.energy_forces(s["xm"])
    de, df = abs(e[0] - s["rebuilt"][0]), float(np.abs(f[0] - s["rebuilt"][1]).max())
    print(f"[swap {name}] unpinned against the checker on the rebuilt graph: |dE| = {de:.3e} eV  max|dF| = {df:.3e} eV/A")
    assert de <= TOL_E and df <= TOL_F


@pytest.mark.parametrize("name", ["cluster", "triclinic"])
def test_a_difference_across_the_swap(eng, swaps, name):
    s = swaps[name]
    h = PC.FD_H
    own = abs(s["fd"] - s["analytic"])                                       # the float64 checker doing the same difference on the fixed graph
    bound = own + 2 * TOL_E / (2 * h)
    eng.set_system(s["z"], max_neigh=PC.MAX_NEIGH)
    eng.set_cell(s["cell"], s["pbc"])
    with eng.pinned(s["x0"]):
        e, f = eng.energy_forces(np.stack([s["xp"], s["xn"], s["xs"]]))
    fd, analytic = (e[0] - e[1]) / (2 * h), -float(f[2][s["j"]].astype(np.float64) @ s["u"])
    e_free, _ = eng.energy_forces(np.stack([s["xp"], s["xn"]]))
    print(f"[difference {name}] checker: fd {s['fd']:.7f} analytic {s['analytic']:.7f} |diff| = {own:.2e} eV/A;  bound {bound:.4f} eV/A")
    print(f"[difference {name}] engine pinned: fd {fd:.7f} -F.u {analytic:.7f} |diff| = {abs(fd - analytic):.3e} eV/A;"
          f"  rebuilt graph: fd {(e_free[0] - e_free[1]) / (2 * h):.4f} eV/A")
    assert abs(fd - analytic) <= bound
    assert abs((e_free[0] - e_free[1]) / (2 * h) - analytic) > 10 * bound       # what the pin is for: unpinned, the difference straddles the swap


# ---- 4. Hessian ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hessian_case(weights):
    z, pos = synth.make_cluster(8, seed=5)
    x0 = pos.astype(np.float32).astype(np.float64)
    orc = PC.checker(weights)
    return dict(z=z, x0=x0, orc=orc, g0=PC.graph_of(orc, x0), ref={})


def elements(z):
    return [synth.SYMBOLS[int(a)] for a in z]


@pytest.mark.parametrize("path", ["host", "device"])
def test_the_hessian_on_the_pinned_graph(hessian_case, monkeypatch, path):
    c = hessian_case
    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    calc = U.uma_pysis(model="synthetic", max_neigh=PC.MAX_NEIGH, hessian_pin_graph=True)
    try:
        elem = elements(c["z"])
        core = calc._ensure_core(elem)
        seen = []                                                            # (positions (K,8,3) float64, forces (K,8,3) float32) of every batch call
        if path == "host":
            monkeypatch.setattr(core, "compute_batch_dev", None)             # fd_hessian then takes the host form
            inner = core.compute_batch

            def batch(coords, *, forces=True):
                assert core.engine.pinned_graph() is not None
                out = inner(coords, forces=forces)
                seen.append((np.array(coords, dtype=np.float64), np.array(out["forces"])))
                return out

            monkeypatch.setattr(core, "compute_batch", batch)
        else:
            inner = core.compute_batch_dev

            def batch_dev(pos32):
                assert core.engine.pinned_graph() is not None
                f = inner(pos32)
                seen.append((pos32.detach().cpu().numpy().astype(np.float64), f.detach().cpu().numpy().copy()))
                return f

            monkeypatch.setattr(core, "compute_batch_dev", batch_dev)
        hess = calc._fd_hessian_ev(elem, c["x0"])["hessian"]
        assert core.engine.pinned_graph() is None and lib_pinned(core.engine) == (0, 0)      # unpinned afterwards
        pos = np.concatenate([p for p, _ in seen])
        frc = np.concatenate([f for _, f in seen])
        assert pos.shape == (48, 8, 3)
        worst = 0.0
        for k in range(48):                                                  # every displaced image against the checker on the pinned graph
            key = pos[k].tobytes()
            if key not in c["ref"]:
                c["ref"][key] = PC.energy_forces_on(c["orc"], c["z"], pos[k], c["g0"])[1]
            worst = max(worst, float(np.abs(frc[k] - c["ref"][key]).max()))
        print(f"[hessian {path}] 48 displaced images on the pinned graph: max|dF| = {worst:.3e} eV/A")
        assert worst <= TOL_F
        # the returned matrix is, bit for bit, what fd_hessian assembles from exactly those forces
        replay = iter(seen)
        if path == "host":
            again = H.fd_hessian(lambda cc: next(replay)[1], c["x0"], calc.freeze_atoms, device=core.device, double=calc.hessian_double,
                                 partial=calc.return_partial_hessian, batch=U.FD_BATCH)
        else:
            again = H.fd_hessian(None, c["x0"], calc.freeze_atoms, device=core.device, double=calc.hessian_double, partial=calc.return_partial_hessian,
                                 batch=U.FD_BATCH, batch_forces_dev=lambda t: torch.as_tensor(next(replay)[1], device=t.device))
        assert torch.equal(hess, again)
        assert float((hess.reshape(24, 24) - hess.reshape(24, 24).T).abs().max()) < 0.05      # (a Hessian, not noise: FD asymmetry of float32 forces)

        # ... and also when the batch call raises
        def broken(*a, **k):
            raise RuntimeError("the batch call failed")

        monkeypatch.setattr(core, "compute_batch" if path == "host" else "compute_batch_dev", broken)
        with pytest.raises(RuntimeError, match="the batch call failed"):
            calc.get_hessian(elem, c["x0"].reshape(-1) * U.ANG2BOHR)
        assert core.engine.pinned_graph() is None and lib_pinned(core.engine) == (0, 0)
    finally:
        calc.close()


# ---- 5. strain on a fixed graph ---------------------------------------------------------------------------------------------------------
def test_the_strain_difference_on_the_fixed_graph(eng, weights):
    z, imgs, cell, pbc = make_case("triclinic")
    x0 = imgs[0].astype(np.float64)
    h = PC.FD_H
    orc = PC.checker(weights, cell=cell, pbc=pbc, max_neigh=300)
    g0 = PC.graph_of(orc, x0)
    w_ad = strain_derivative(orc, z, x0, graph=g0)
    eps = []
    for a, b in ((0, 0), (1, 2)):
        for sign in (1.0, -1.0):
            e = np.zeros((3, 3))
            e[a, b] = sign * h
            eps.append(np.eye(3) + e)
    cells = np.stack([cell @ d for d in eps])
    xs = np.stack([x0 @ d for d in eps])
    # the checker's own error doing this difference on the fixed graph (translations: the same integer triples in the strained cell)
    e_ref = [PC.energy_on(orc, z, xs[k], PC.graph_in_cell(orc, g0, cells[k])) for k in range(4)]
    own = max(abs((e_ref[0] - e_ref[1]) / (2 * h) - w_ad[0, 0]), abs((e_ref[2] - e_ref[3]) / (2 * h) - w_ad[1, 2]))
    bound = 2 * own + 2 * TOL_E / (2 * h)                                     # factor 2: float32 edge vectors
    eng.set_system(z)
    eng.set_cell(cell, pbc)
    _, _, w = eng.energy_forces_virial(x0)
    eng.pin_graph(x0)
    eng.set_cells(cells, pbc)                                                # the same flags: the pin stays, the translations follow the cells
    assert lib_pinned(eng) == (len(g0[0]), eng.pinned_graph()[1])
    e, _ = eng.energy_forces(xs)
    eng.unpin_graph()
    d_xx, d_yz = (e[0] - e[1]) / (2 * h), (e[2] - e[3]) / (2 * h)
    print(f"[strain] checker: own error {own:.3e} eV;  bound {bound:.4f} eV")
    print(f"[strain] engine: dE/deps_xx fd {d_xx:.6f} W {w[0, 0, 0]:.6f};  dE/deps_yz fd {d_yz:.6f} W {w[0, 1, 2]:.6f}")
    for k in range(4):
        assert abs(e[k] - e_ref[k]) <= TOL_E, (k, e[k], e_ref[k])             # each strained image on the fixed graph, against the checker
    assert abs(d_xx - w[0, 0, 0]) <= bound and abs(d_yz - w[0, 1, 2]) <= bound


# ---- 6. plans ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_case(weights):
    """40 atoms, a binding cap, three moved geometries; the one-piece results pinned at the reference, and unpinned at the reference."""
    z, x0 = cluster(40, 9)
    rng = np.random.default_rng(2)
    moved = np.stack([x0 + 0.05 * rng.standard_normal(x0.shape).astype(np.float32) for _ in range(3)])
    e_ = new_engine(weights)
    try:
        e_.set_system(z, max_neigh=12)
        with e_.pinned(x0):
            whole = e_.energy_forces_virial(moved)
            assert (e_.last_partitions(), e_.last_recompute(), e_.last_lanes()) == (0, 0, 1)
        free_moved = e_.energy_forces_virial(moved)
        assert not same_bits(whole[0], free_moved[0])                        # the moved geometries do have another graph: the pin matters here
    finally:
        e_.close()
    return dict(z=z, x0=x0, moved=moved, whole=whole)


@pytest.mark.parametrize("setting", ["parts2", "parts3", "lanes", "recompute2"])
def test_pinned_plans(weights, plan_case, monkeypatch, setting):
    c = plan_case
    parts = int(setting[-1]) if setting.startswith("parts") else 0
    if parts:
        monkeypatch.setenv("UMX_FORCE_PARTS", str(parts))
    if setting == "lanes":
        monkeypatch.setenv("UMX_STREAMS", "2")
        monkeypatch.setenv("UMX_MAX_CHUNK_IMAGES", "1")
    e_ = new_engine(weights, **({"recompute": 2} if setting == "recompute2" else {}))
    rc = new_engine(weights, recompute=2) if parts else None
    try:
        e_.set_system(c["z"], max_neigh=12)
        e_.pin_graph(c["x0"])
        out = e_.energy_forces_virial(c["moved"])            # (first: a workspace sized by a one-image call would keep the engine on one lane)
        assert e_.last_partitions() == parts and e_.last_recompute() == (1 if setting == "recompute2" else 0)
        assert e_.last_lanes() == (2 if setting == "lanes" else 1)
        assert e_.graph_stats() == (3 * e_.pinned_graph()[0], e_.pinned_graph()[1])
        # the plan at the reference itself: bitwise the same plan unpinned
        ref3 = np.stack([c["x0"]] * 3)
        at_ref_pinned = e_.energy_forces_virial(ref3)
        e_.unpin_graph()
        assert same_efw(at_ref_pinned, e_.energy_forces_virial(ref3))
        assert e_.last_partitions() == parts and e_.last_lanes() == (2 if setting == "lanes" else 1)
        if parts:
            # partitions differ from one piece at float32 summation order (tests/test_gpu_parity.py: 2e-5), and are bitwise the recompute
            # plan of the same partition count (tests/test_gpu_recompute.py) -- pinned as unpinned
            de, df = np.abs(out[0] - c["whole"][0]).max(), np.abs(out[1] - c["whole"][1]).max()
            print(f"[plans {setting}] against the pinned one-piece plan: max|dE| = {de:.3e} eV  max|dF| = {df:.3e} eV/A")
            assert de <= 2e-5 and df <= 2e-5
            rc.set_system(c["z"], max_neigh=12)
            rc.pin_graph(c["x0"])
            assert same_efw(rc.energy_forces_virial(c["moved"]), out) and rc.last_partitions() == parts and rc.last_recompute() == 1
        else:
            assert same_efw(out, c["whole"]), setting                        # chunks on two lanes, the recompute plan: bitwise the one-piece plan
    finally:
        e_.close()
        if rc is not None:
            rc.close()


# ---- 7. rules ------------------------------------------------------------------------------------------------------------------------------
def test_the_rules(eng, weights, monkeypatch):
    z, imgs, cell, pbc = make_case("triclinic", k=2)
    x0, x1 = imgs[0], imgs[1]
    with pytest.raises(UmxError, match="bind a system first") as ei:
        eng.pin_graph(np.zeros((0, 3)))
    assert ei.value.status == -1 and eng.pinned_graph() is None
    eng.set_system(z, max_neigh=PC.MAX_NEIGH)
    eng.set_cell(cell, pbc)
    free = eng.energy_forces(x1)
    eng.pin_graph(x0)
    n_edges = lib_pinned(eng)[0]
    assert n_edges == PC.MAX_NEIGH * len(z)
    pinned = eng.energy_forces(x1)
    # a failed pin leaves the previous state
    bad = x0.copy()
    bad[3, 1] = np.nan
    with pytest.raises(UmxError, match="non-finite"):
        eng.pin_graph(bad)
    assert lib_pinned(eng)[0] == n_edges and same_efw(eng.energy_forces(x1), pinned)
    # a strained cell with the same flags keeps the pin; other flags unpin
    eng.set_cell(cell * 1.01, pbc)
    assert lib_pinned(eng)[0] == n_edges and eng.pinned_graph() is not None
    eng.set_cell(cell, pbc)
    assert same_efw(eng.energy_forces(x1), pinned)
    eng.set_cell(cell, (True, True, False))
    assert lib_pinned(eng) == (0, 0) and eng.pinned_graph() is None
    eng.set_cell(cell, pbc)
    assert same_efw(eng.energy_forces(x1), free)
    # set_system unpins
    eng.pin_graph(x0)
    eng.set_system(z, max_neigh=PC.MAX_NEIGH)
    assert lib_pinned(eng) == (0, 0) and eng.pinned_graph() is None and same_efw(eng.energy_forces(x1), free)
    # the graph-parallel entry refuses a pinned engine, naming the pin
    eng.pin_graph(x0)
    pos = torch.tensor(x1, device="cuda")
    e_t = torch.zeros(1, dtype=torch.float64, device="cuda")
    f_t = torch.zeros(len(z), 3, dtype=torch.float32, device="cuda")
    with pytest.raises(UmxError, match=r"umx_gp_begin.*pinned") as ei:
        eng.gp_begin(pos.data_ptr(), 0, len(z), e_t.data_ptr(), f_t.data_ptr())
    assert ei.value.status == -1                                             # UMX_ERR_ARG
    # the with block unpins on an exception
    eng.unpin_graph()
    with pytest.raises(KeyError):
        with eng.pinned(x0):
            assert lib_pinned(eng)[0] == n_edges
            raise KeyError("inside")
    assert lib_pinned(eng) == (0, 0) and eng.pinned_graph() is None


class _Atoms:
    def __init__(self, z, pos, cell, pbc):
        self.numbers, self._pos, self.cell, self.pbc, self.info = z, np.asarray(pos, dtype=np.float64), cell, pbc, {}

    def get_positions(self):
        return self._pos


def test_the_pool_and_the_facade(eng, weights, monkeypatch):
    from pdb2reaction_amd.engine import Engine
    from pdb2reaction_amd.parallel import LocalEnginePool

    z, imgs, cell, pbc = make_case("triclinic", k=3)
    eng.set_system(z, max_neigh=PC.MAX_NEIGH)
    eng.set_cell(cell, pbc)
    with eng.pinned(imgs[0]):
        one = eng.energy_forces(imgs[1])
        three = eng.energy_forces(imgs)
    pool = LocalEnginePool.create([0, 0], weights, engine_factory=Engine)
    try:
        pool.set_system(z, max_neigh=PC.MAX_NEIGH)
        pool.set_cell(cell, pbc)
        with pool.pinned(imgs[0]):
            assert pool.pinned_graph() == (PC.MAX_NEIGH * len(z), PC.MAX_NEIGH)
            out = pool.energy_forces(imgs[1])
            assert pool.last_route == "single" and same_efw(out, one)       # a single geometry: engine 0 alone
            assert same_efw(pool.energy_forces(imgs), three) and pool.last_route == "batch"
        assert pool.pinned_graph() is None and all(lib_pinned(e_) == (0, 0) for e_ in pool.engines)
    finally:
        pool.close()
    A = importlib.import_module("pdb2reaction_amd.ase_calculator")
    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    calc = A.UMXCalculator(model="synthetic", max_neigh=PC.MAX_NEIGH)
    try:
        atoms = [_Atoms(z, p, cell, pbc) for p in imgs]
        with calc.pinned(atoms[0]):
            e, f = calc.calculate_images(atoms)
        assert same_bits(e, three[0]) and same_bits(f, three[1].astype(np.float64))
        assert lib_pinned(calc._engine) == (0, 0)
    finally:
        calc.close()
