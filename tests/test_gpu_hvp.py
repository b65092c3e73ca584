"""Hessian-vector products on the GPU (``umx_hvp`` / ``umx_hvp_dev``): pinned, float64, batched.

Two yardsticks (tests/hvp_cases.py).  Exact: ``Engine.hvp`` is, bit for bit, the NumPy float64 formula applied to the float32 forces of
single evaluations ``energy_forces(x[None], double_positions=True)`` under ``pin_graph(base, double_positions=True)`` -- in every plan
(chunks, two lanes, recompute, a pool; partitions against partitioned singles) and precision mode.  Float64: the checker's central
difference of its own forces at the same step on the base's fixed graph; the elementwise bound is derived, (t+ + t-) / (2 step) with
t+- = TOL_F, the force tolerance tests/test_gpu_pinned_graph.py applies to displaced geometries on a pinned graph (1e-3 eV/A): 1 eV/A^2
at step 1e-3 A.  Measured maxima are printed and recorded in profiles/hvp.txt.

Synthetic weights seed 0; every case is a handful of evaluations of at most 12 atoms."""
import ctypes as C

import numpy as np
import pytest
import torch

import hvp_cases as HC
import pinned_cases as PC
from test_gpu_periodic import TOL_F
from pdb2reaction_amd import hessian as H
from pdb2reaction_amd.engine import UmxError

pytestmark = pytest.mark.gpu

DP = {"double_positions": True}


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


def bind(e, c):
    e.set_system(c["z"], max_neigh=c["max_neigh"])
    e.set_cell(c["cell"], c["pbc"])


def lib_pinned(e):
    ne, md = C.c_int64(-1), C.c_int32(-1)
    assert e.lib.umx_pinned_graph(e._h, C.byref(ne), C.byref(md)) == 0
    return int(ne.value), int(md.value)


def single_forces(e, c, xs, base=None):
    """Forces (K,N,3) float32 of every image evaluated ALONE under pin_graph(base) with float64 positions."""
    with e.pinned(c["x"] if base is None else base, **DP):
        return np.concatenate([e.energy_forces(x[None], **DP)[1] for x in xs])


def by_hand(e, c, dirs, step, scheme):
    xs = HC.images(c["x"], dirs, step, scheme)
    return HC.combine(single_forces(e, c, xs), step, scheme)


@pytest.fixture(scope="module")
def cases(weights):
    cs = HC.bases(weights)
    for c in cs.values():
        c["dirs"] = HC.directions(len(c["z"]))
    return cs


@pytest.fixture(scope="module")
def plain(weights, cases):
    """Computed once on a default engine and left unchanged: (base, step, scheme) -> (hv by hand from single evaluations, curv of
    ``Engine.hvp``)."""
    e = new_engine(weights)
    out = {}
    try:
        for name, c in cases.items():
            bind(e, c)
            for step in HC.STEPS:
                for scheme in HC.SCHEMES:
                    hand = by_hand(e, c, c["dirs"], step, scheme)
                    _, curv = e.hvp(c["x"], c["dirs"], step=step, scheme=scheme, return_curvature=True)
                    out[(name, step, scheme)] = (hand, curv)
    finally:
        e.close()
    return out


# ---- 1. composition, bit for bit; 9. precision modes ---------------------------------------------------------------------------------------
SETTINGS = {
    # name: (environment, Engine keywords, compare with the default engine's singles (else: singles under the setting itself))
    "plain": ({}, {}, True),
    "chunk3": ({"UMX_MAX_CHUNK_IMAGES": "3"}, {}, True),           # 48-edge bases: a chunk seam between +v and -v of direction 1
    "streams2": ({"UMX_STREAMS": "2"}, {}, True),
    "recompute2": ({"UMX_RECOMPUTE": "2"}, {}, True),               # read at umx_create
    "parts2": ({"UMX_FORCE_PARTS": "2"}, {}, False),                # partitions differ from one piece at float32 summation order (README)
    "fp32": ({}, {"precision": "fp32"}, False),
    "split-bf16": ({}, {"precision": "split-bf16"}, False),
}


ONCE = ("fp32", "split-bf16")                                              # the precision modes run case 1 once: they take the same plan


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_hvp_is_the_formula_on_single_pinned_evaluations(weights, cases, plain, monkeypatch, setting):
    env, kw, against_plain = SETTINGS[setting]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    e = new_engine(weights, **kw)
    try:
        for name, c in cases.items():
            bind(e, c)
            for step in (HC.STEPS[:1] if setting in ONCE else HC.STEPS):
                for scheme in HC.SCHEMES:
                    hv, curv = e.hvp(c["x"], c["dirs"], step=step, scheme=scheme, return_curvature=True)
                    assert hv.dtype == np.float64 and hv.shape == c["dirs"].shape
                    assert e.pinned_graphs() is None and lib_pinned(e) == (0, 0)          # the entry's own pin is gone
                    want, want_curv = plain[(name, step, scheme)] if against_plain else (by_hand(e, c, c["dirs"], step, scheme), None)
                    assert same_bits(hv, want), (setting, name, step, scheme, float(np.abs(hv - want).max()))
                    if against_plain:
                        assert same_bits(curv, want_curv), (setting, name, step, scheme)    # 6: curv does not depend on the plan
        if setting == "chunk3":
            assert e.last_lanes() == 1
        if setting == "streams2":
            assert e.last_lanes() == 2
        if setting == "recompute2":
            assert e.last_recompute() == 1
        if setting == "parts2":
            assert e.last_partitions() == 2
    finally:
        e.close()


def test_a_pool_of_two_engines_on_one_device(weights, cases, plain, monkeypatch):
    from pdb2reaction_amd.engine import Engine
    from pdb2reaction_amd.parallel import LocalEnginePool, local_devices_for

    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,0")
    pool = LocalEnginePool.create(local_devices_for(2), weights, engine_factory=Engine)
    try:
        for name, c in cases.items():
            pool.set_system(c["z"], max_neigh=c["max_neigh"])
            pool.set_cell(c["cell"], c["pbc"])
            for step in HC.STEPS:
                for scheme in HC.SCHEMES:
                    hv, curv = pool.hvp(c["x"], c["dirs"], step=step, scheme=scheme, return_curvature=True)
                    assert pool.last_route == "batch" and pool.last_blocks == [(0, 2), (2, 3)]
                    want, want_curv = plain[(name, step, scheme)]
                    assert same_bits(hv, want) and same_bits(curv, want_curv), (name, step, scheme)
            one = pool.hvp(c["x"], c["dirs"][1])                               # a single direction: engine 0 alone
            assert pool.last_route == "single" and same_bits(one[0], plain[(name, 1e-3, "central")][0][1])
    finally:
        pool.close()


# ---- 2. a column of the finite-difference Hessian ------------------------------------------------------------------------------------------
def test_a_unit_vector_gives_the_fd_hessian_column(eng, cases):
    c = cases["swap"]                                                         # 48 edges: every image of fd_hessian's batches starts at an even row
    bind(eng, c)
    n = len(c["z"])
    with eng.pinned(c["x"], **DP):
        assert eng.pinned_graph()[0] % 2 == 0
        hess = H.fd_hessian(lambda x: eng.energy_forces(x, **DP)[1], c["x"], [], device="cpu", double=True, partial=False, double_positions=True)
    cols = hess.reshape(3 * n, 3 * n).numpy()
    ks = (0, 3 * 5 + 1, 3 * n - 1)
    unit = np.zeros((len(ks), 3 * n))
    unit[np.arange(len(ks)), ks] = 1.0
    hv = eng.hvp(c["x"], unit.reshape(len(ks), n, 3), step=H.FD_STEP_ANG)
    for m, k in enumerate(ks):
        assert same_bits(hv[m].reshape(-1), np.ascontiguousarray(cols[:, k])), k


# ---- 3. several bases, the caller's pin ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def swap(weights):
    z, orc, x0, xm, xs, u, j = PC.cluster_swap(weights)
    return dict(z=z, orc=orc, x0=x0, xm=xm, u=u, j=j, g0=PC.graph_of(orc, x0), gm=PC.graph_of(orc, xm), max_neigh=PC.MAX_NEIGH, cell=None, pbc=None)


@pytest.mark.parametrize("scheme", HC.SCHEMES)
def test_several_bases(eng, swap, scheme):
    s = swap
    bind(eng, s)
    dirs, base_of = HC.directions(len(s["z"]), seed=12), [1, 0, 1]
    both = np.stack([s["x0"], s["xm"]])
    hv, curv = eng.hvp(both, dirs, base_of, scheme=scheme, return_curvature=True)
    assert eng.pinned_graphs() is None and lib_pinned(eng) == (0, 0)
    for m, b in enumerate(base_of):
        one, c1 = eng.hvp(both[b], dirs[m], scheme=scheme, return_curvature=True)
        assert same_bits(hv[m], one[0]) and same_bits(curv[m: m + 1], c1), (scheme, m)
    # the bases pinned by the caller, R references: direction m replays reference base_of[m]; pin and assignment stay the caller's
    eng.pin_graphs(both, assign=[1, 1, 0], **DP)
    before = eng.pinned_graphs()
    assert same_bits(eng.hvp(both, dirs, base_of, scheme=scheme), hv)
    assert eng.pinned_graphs() == before and lib_pinned(eng) == (sum(before[0]), before[1])
    three = np.stack([s["xm"], s["xm"], s["x0"]])
    e3, f3 = eng.energy_forces(three, **DP)                                   # the assignment of three images still holds ...
    with pytest.raises(UmxError, match="umx_pin_assign"):
        eng.energy_forces(both, **DP)                                         # ... for exactly three
    eng.unpin_graph()
    for k, ref in enumerate((s["xm"], s["xm"], s["x0"])):
        with eng.pinned(ref, **DP):
            assert same_bits(eng.energy_forces(three[k][None], **DP)[1], f3[k: k + 1])


def test_a_callers_pin_at_another_geometry_is_used(eng, swap):
    s = swap
    bind(eng, s)
    assert not PC.same_graph(s["g0"], s["gm"])
    dirs, step = HC.directions(len(s["z"]), seed=13), 1e-3
    want = HC.checker_hv(s["orc"], s["z"], s["xm"], dirs, step, s["g0"])      # the checker on the graph of x_start, probed at x_moved
    other = HC.checker_hv(s["orc"], s["z"], s["xm"], dirs[:1], step, s["gm"])
    bound = (TOL_F + TOL_F) / (2 * step)
    eng.pin_graph(s["x0"], **DP)
    hv = eng.hvp(s["xm"], dirs, step=step)
    assert eng.pinned_graph() == (len(s["g0"][0]), PC.MAX_NEIGH)              # still the caller's
    err = float(np.abs(hv - want).max())
    print(f"[caller's pin] max|Hv - checker on graph(x_start)| = {err:.3e} eV/A^2 (bound {bound:.3f}); the two graphs' products differ by "
          f"{float(np.abs(want[0] - other[0]).max()):.3f}")
    assert err <= bound
    assert float(np.abs(want[0] - other[0]).max()) > 10 * err                 # the graphs differ by far more than the engine's error
    # bitwise: the images alone under the same pin
    assert same_bits(hv, HC.combine(np.concatenate([eng.energy_forces(x[None], **DP)[1] for x in HC.images(s["xm"], dirs, step, "central")]), step, "central"))
    # "do not pin" is refused under a pin, and the pin survives the refusal
    with pytest.raises(UmxError, match=r"umx_hvp.*pinned") as ei:
        eng.hvp(s["xm"], dirs, pin=False)
    assert ei.value.status == -1 and eng.pinned_graph() == (len(s["g0"][0]), PC.MAX_NEIGH)
    # another number of references than bases (and than one) is refused
    eng.pin_graphs(np.stack([s["x0"], s["xm"], s["x0"]]), **DP)
    with pytest.raises(UmxError, match=r"umx_hvp: 3 graphs are pinned and 2 bases") as ei:
        eng.hvp(np.stack([s["x0"], s["xm"]]), dirs, [0, 1, 0])
    assert ei.value.status == -1 and len(eng.pinned_graphs()[0]) == 3


# ---- 4. against the float64 checker; what the pin is for --------------------------------------------------------------------------------
def test_against_the_checker(eng, cases, weights):
    step = 1e-3
    bound = (TOL_F + TOL_F) / (2 * step)
    for name, c in cases.items():
        orc = PC.checker(weights, cell=c["cell"], pbc=c["pbc"], max_neigh=c["max_neigh"])
        want = HC.checker_hv(orc, c["z"], c["x"], c["dirs"], step, PC.graph_of(orc, c["x"]))
        bind(eng, c)
        hv = eng.hvp(c["x"], c["dirs"], step=step)
        err = float(np.abs(hv - want).max())
        print(f"[checker {name}] max|Hv_engine - Hv_checker| = {err:.3e} eV/A^2 (bound {bound:.3f}, max|Hv| = {float(np.abs(want).max()):.3f})")
        assert err <= bound, name


def test_the_rank_swap_breaks_the_unpinned_product(eng, swap):
    s = swap
    bind(eng, s)
    step = 2 * PC.INSIDE                                                      # larger than INSIDE: x_moved + step v is back outside the M-th neighbour
    v = np.zeros((1, len(s["z"]), 3))
    v[0, s["j"]] = s["u"]
    assert not PC.same_graph(PC.graph_of(s["orc"], s["xm"] + step * v[0]), PC.graph_of(s["orc"], s["xm"] - step * v[0]))
    want = HC.checker_hv(s["orc"], s["z"], s["xm"], v, step, s["gm"])
    bound = (TOL_F + TOL_F) / (2 * step)
    pinned, free = eng.hvp(s["xm"], v, step=step), eng.hvp(s["xm"], v, step=step, pin=False)
    ep, ef = float(np.abs(pinned - want).max()), float(np.abs(free - want).max())
    print(f"[rank swap] step {step} A: pinned max|Hv - checker| = {ep:.3e}, unpinned {ef:.3e} eV/A^2 (bound {bound:.3f})")
    assert ep <= bound
    assert ef > bound                                                         # the defect the entry removes
    # unpinned is the reference's semantics, kept for A/B: the same formula on unpinned single evaluations
    xs = HC.images(s["xm"], v, step, "central")
    assert same_bits(free, HC.combine(np.concatenate([eng.energy_forces(x[None], **DP)[1] for x in xs]), step, "central"))


# ---- 5. frame independence ------------------------------------------------------------------------------------------------------------------
def test_a_translation_changes_no_bit(eng, cases):
    """Base (float32-representable) and direction (float32-representable) with step 2^-10: base + step * dir is exact in float64, and
    stays exact 64 A away -- so every float64 difference the graph kernels form is the same number, and every bit must be too."""
    c = cases["odd47"]
    bind(eng, c)
    x = c["x"].astype(np.float32).astype(np.float64)
    dirs = c["dirs"].astype(np.float32).astype(np.float64)
    step, shift = 2.0 ** -10, np.array([64.0, 64.0, 64.0])
    assert np.array_equal((x + shift) - shift, x)
    here = eng.hvp(x, dirs, step=step, return_curvature=True)
    there = eng.hvp(x + shift, dirs, step=step, return_curvature=True)
    assert same_bits(here[0], there[0]) and same_bits(here[1], there[1])
    with eng.pinned(x + shift, **DP):                                        # the pin reference translated as well
        there = eng.hvp(x + shift, dirs, step=step, return_curvature=True)
    assert same_bits(here[0], there[0]) and same_bits(here[1], there[1])


# ---- 6. curv ----------------------------------------------------------------------------------------------------------------------------------
def test_the_curvature(eng, cases):
    for name, c in cases.items():
        bind(eng, c)
        hv, curv = eng.hvp(c["x"], c["dirs"], return_curvature=True)
        want, bound = HC.curvature_exact(c["dirs"], hv)
        print(f"[curv {name}] {curv}  max|curv - exact| = {float(np.abs(curv - want).max()):.2e} (bound {float(bound.min()):.2e})")
        assert (np.abs(curv - want) <= bound).all(), name


# ---- 7. edges of the domain ---------------------------------------------------------------------------------------------------------------------
def test_no_edges_one_direction_zero_direction(eng, cases):
    z = np.array([8, 1], dtype=np.int64)
    x = np.array([[0.0, 0.0, 0.0], [20.0, 0.0, 0.0]])
    eng.set_system(z)
    eng.set_cell(None, None)
    d = HC.directions(2, m=1)
    for scheme in HC.SCHEMES:
        hv, curv = eng.hvp(x, d[0], scheme=scheme, return_curvature=True)      # M = 1, (N,3) in
        assert hv.shape == (1, 2, 3) and not hv.any() and curv[0] == 0.0
    assert eng.graph_stats()[0] == 0
    c = cases["odd47"]
    bind(eng, c)
    dirs = c["dirs"].copy()
    dirs[1] = 0.0
    hv, curv = eng.hvp(c["x"], dirs, return_curvature=True)
    assert not hv[1].any() and curv[1] == 0.0 and np.isfinite(curv).all() and hv[0].any() and hv[2].any()
    e0, f0 = eng.hvp(c["x"], dirs, scheme="forward", return_base=True)[1:]
    with eng.pinned(c["x"], **DP):
        ref = eng.energy_forces(c["x"][None], **DP)
    assert same_bits(e0, ref[0]) and same_bits(f0, ref[1])
    # the bases' forces handed back in: the same bits, one image less
    again = eng.hvp(c["x"], dirs, scheme="forward", base_forces=f0)
    assert eng.graph_stats()[0] == 3 * 47
    assert same_bits(again, eng.hvp(c["x"], dirs, scheme="forward")) and eng.graph_stats()[0] == 4 * 47


def refused(e, call, pattern):
    with pytest.raises(UmxError, match=pattern) as ei:
        call()
    assert ei.value.status == -1, ei.value                                    # UMX_ERR_ARG
    assert lib_pinned(e) == (0, 0)                                            # nothing pinned before, nothing after


def test_refusals(weights, cases):
    c = cases["odd47"]
    n = len(c["z"])
    x, dirs = c["x"], c["dirs"]
    e = new_engine(weights)
    try:
        dp = C.POINTER(C.c_double)
        hv = np.empty_like(dirs)
        raw = lambda: e._chk(e.lib.umx_hvp(e._h, 1, x.ctypes.data_as(dp), 1, dirs.ctypes.data_as(dp), None, 1e-3, 0, hv.ctypes.data_as(dp), None, None, None), "umx_hvp")
        refused(e, raw, r"umx_hvp: bind a system first")
        bind(e, c)
        want = e.hvp(x, dirs)
        for bad in (0.0, -1e-3, float("nan"), float("inf")):
            refused(e, lambda: e.hvp(x, dirs, step=bad), r"umx_hvp: the step must be finite and positive")
        two = np.stack([x, x])
        refused(e, lambda: e.hvp(two, dirs, [0, 2, 1]), r"umx_hvp: direction 1 names base 2, but 2 were given")
        refused(e, lambda: e.hvp(two, dirs, [0, -1, 1]), r"umx_hvp: direction 1 names base -1")
        xb = two.copy()
        xb[1, 3, 2] = np.nan
        refused(e, lambda: e.hvp(xb, dirs, [0, 0, 1]), r"umx_hvp: non-finite position \(base 1\)")
        db = dirs.copy()
        db[2, 0, 0] = np.inf
        refused(e, lambda: e.hvp(x, db), r"umx_hvp: non-finite component \(direction 2\)")
        e0 = np.empty(1)
        central_e0 = lambda: e._chk(e.lib.umx_hvp(e._h, 1, x.ctypes.data_as(dp), 1, dirs.ctypes.data_as(dp), None, 1e-3, 0, hv.ctypes.data_as(dp), None,
                                                  e0.ctypes.data_as(dp), None), "umx_hvp")
        refused(e, central_e0, r"umx_hvp: e0 and f0 .* forward scheme")
        fp = C.POINTER(C.c_float)
        f0 = np.zeros((1, n, 3), dtype=np.float32)

        def raw_call(flags, e0_=None, f0_=None, bases=1, bof=None):
            xb_ = np.ascontiguousarray(np.stack([x] * bases))
            return lambda: e._chk(e.lib.umx_hvp(e._h, bases, xb_.ctypes.data_as(dp), 1, dirs.ctypes.data_as(dp), bof, 1e-3, flags, hv.ctypes.data_as(dp), None,
                                                 e0_.ctypes.data_as(dp) if e0_ is not None else None, f0_.ctypes.data_as(fp) if f0_ is not None else None), "umx_hvp")

        refused(e, raw_call(0, f0_=f0), r"umx_hvp: e0 and f0 .* forward scheme")                    # f0 alone with the central scheme
        refused(e, raw_call(4, f0_=f0), r"umx_hvp: flags bit 2 hands the bases' forces IN")         # bit 2 without bit 0
        refused(e, raw_call(5), r"umx_hvp: flags bit 2 hands the bases' forces IN")                 # bit 2 without f0
        refused(e, raw_call(5, e0_=e0, f0_=f0), r"umx_hvp: flags bit 2 hands the bases' forces IN")  # e0 beside a given f0
        refused(e, raw_call(8), r"umx_hvp: bad arguments")                                          # an unknown flag
        refused(e, raw_call(0, bases=2), r"umx_hvp: base_of may be NULL only with one base, 2 were given")
        # per-image cells: with several bases (the rule of umx_pin_graphs), and with one base and as many cells as images -- +v and -v
        # would each take another cell
        t = cases["triclinic"]
        bind(e, t)
        e.set_cells(np.stack([t["cell"], t["cell"]]), t["pbc"])
        refused(e, lambda: e.hvp(np.stack([t["x"], t["x"]]), t["dirs"], [0, 1, 0]), r"umx_hvp: per-image cells are bound")
        refused(e, lambda: e.hvp(t["x"], t["dirs"][0]), r"umx_hvp: per-image cells are bound")
        # a graph-parallel evaluation in progress
        bind(e, c)
        pos = torch.tensor(x.astype(np.float32), device="cuda")
        e_t, f_t = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(n, 3, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        e.gp_begin(pos.data_ptr(), 0, n, e_t.data_ptr(), f_t.data_ptr())
        refused(e, lambda: e.hvp(x, dirs), r"umx_hvp: a graph-parallel evaluation is in progress")
        while not e.gp_step()[2]:
            pass
        e.synchronize()
        assert same_bits(e.hvp(x, dirs), want)                                # the engine is usable afterwards
    finally:
        e.close()


# ---- 8. the device entry --------------------------------------------------------------------------------------------------------------------
def test_the_device_entry(eng, cases, monkeypatch):
    c = cases["odd47"]
    bind(eng, c)
    n, dev = len(c["z"]), torch.device("cuda", 0)
    two = np.stack([c["x"], c["x"] + 0.01 * HC.directions(n, m=1, seed=5)[0]])
    base_of = [1, 0, 1]
    b_t, d_t = torch.from_numpy(two).to(dev), torch.from_numpy(c["dirs"]).to(dev)
    for scheme in HC.SCHEMES:
        want = eng.hvp(two, c["dirs"], base_of, scheme=scheme, return_curvature=True, **({"return_base": True} if scheme == "forward" else {}))
        hv_t, cv_t = torch.full((3, n, 3), float("nan"), dtype=torch.float64, device=dev), torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
        e_t, f_t = torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros(2, n, 3, dtype=torch.float32, device=dev)
        fwd = scheme == "forward"
        for pinned in (False, True):
            if pinned:
                eng.pin_graphs(two, **DP)
            hv_t.fill_(float("nan"))
            eng.hvp_dev(2, b_t.data_ptr(), 3, d_t.data_ptr(), hv_t.data_ptr(), base_of=base_of, scheme=scheme, d_curv=cv_t.data_ptr(),
                        d_e0=e_t.data_ptr() if fwd else 0, d_f0=f_t.data_ptr() if fwd else 0, stream=torch.cuda.current_stream(dev).cuda_stream)
            got = (hv_t.cpu().numpy(), cv_t.cpu().numpy()) + ((e_t.cpu().numpy(), f_t.cpu().numpy()) if fwd else ())
            assert not eng.take_range_error()
            assert len(got) == len(want) and all(same_bits(a, b) for a, b in zip(got, want)), (scheme, pinned)
            if pinned:
                assert len(eng.pinned_graphs()[0]) == 2
                eng.unpin_graph()
            else:
                assert lib_pinned(eng) == (0, 0)


def test_the_device_entry_reads_nothing_back_under_a_pin(eng, cases):
    """With a caller's pin in force the call only enqueues: it returns while a long kernel queued in front of it on the same stream is
    still running, so nothing in it waited for the stream (no device-to-host read).  Without a pin the bases are read back once."""
    c = cases["swap"]
    bind(eng, c)
    n, dev = len(c["z"]), torch.device("cuda", 0)
    b_t, d_t = torch.from_numpy(c["x"]).to(dev), torch.from_numpy(c["dirs"]).to(dev)
    hv_t = torch.empty(3, n, 3, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev)
    eng.pin_graph(c["x"], **DP)
    eng.hvp_dev(1, b_t.data_ptr(), 3, d_t.data_ptr(), hv_t.data_ptr(), stream=stream.cuda_stream)      # buffers grown, workspace allocated
    torch.cuda.synchronize(dev)
    want = hv_t.cpu().numpy().copy()
    big = torch.randn(8192, 8192, device=dev)
    torch.cuda.synchronize(dev)
    done = torch.cuda.Event()
    for _ in range(20):
        big = big @ big * 1e-4                                              # tens of milliseconds of queued work
    done.record(stream)
    eng.hvp_dev(1, b_t.data_ptr(), 3, d_t.data_ptr(), hv_t.data_ptr(), stream=stream.cuda_stream)
    returned_early = not done.query()
    torch.cuda.synchronize(dev)
    assert returned_early, "umx_hvp_dev waited for the stream although a pin was in force"
    assert same_bits(hv_t.cpu().numpy(), want)
    eng.unpin_graph()


# ---- 10. the layers above the engine ---------------------------------------------------------------------------------------------------------
def test_the_string_evaluator(eng, cases):
    """``EngineStringEvaluator.hvp`` -- what ``climb_lanczos_hvp`` drives -- is ``Engine.hvp`` at x0 * BOHR2ANG with step dx * BOHR2ANG
    times the unit factor, frozen rows zeroed in q and in the result, bit for bit; in the forward scheme the base's forces come back on
    the device and, handed back in (``umx_hvp_dev`` flags bit 2), give the same bits from one image; pinned once for a recursion, the same."""
    from pdb2reaction_amd._calculator_base import ANG2BOHR, BOHR2ANG
    from pdb2reaction_amd.parallel import EngineStringEvaluator

    c = cases["odd47"]
    bind(eng, c)
    n, dev, frozen, dx = len(c["z"]), torch.device("cuda", 0), [2, 7], 5e-3
    ev = EngineStringEvaluator(eng, n, dev, frozen=frozen)
    x_bohr = (c["x"] * ANG2BOHR).reshape(-1)
    x0 = torch.as_tensor(x_bohr, device=dev)
    qs = HC.directions(n, m=2, seed=21).reshape(2, -1)
    qs /= np.linalg.norm(qs, axis=1)[:, None]
    base, step = x_bohr.reshape(n, 3) * float(BOHR2ANG), float(dx) * float(BOHR2ANG)

    def want(q, scheme, **kw):
        d = q.reshape(1, n, 3).copy()
        d[:, frozen] = 0.0
        out = eng.hvp(base, d, step=step, scheme=scheme, **kw)
        hv = (out[0] if kw else out)[0] * float(H.EV_PER_ANG2_TO_AU)
        hv[frozen] = 0.0
        return (hv.reshape(-1),) + (tuple(out[1:]) if kw else ())

    def run(q, *a, **kw):
        out = ev.hvp(x0, torch.as_tensor(q, device=dev), dx, *a, **kw)
        assert not eng.take_range_error()
        return out

    for pin_once in (False, True):
        if pin_once:
            ev.hvp_pin(x0)
            assert lib_pinned(eng) == (47, PC.MAX_NEIGH)
        got = run(qs[0], "central")
        assert ev.images_last == 2 and got.shape == (3 * n,) and not got.reshape(n, 3)[frozen].any() and got.any()
        hv1, f0 = run(qs[0], "forward", return_base=True)
        assert ev.images_last == 2 and f0.dtype == torch.float32 and f0.shape == (n, 3)
        hv2 = run(qs[1], "forward", base=f0)
        assert ev.images_last == 1 and eng.graph_stats()[0] == 47                    # one image: the base was not evaluated again
        if pin_once:
            ev.hvp_unpin()
        assert lib_pinned(eng) == (0, 0)
        w1, e0, wf0 = want(qs[0], "forward", return_base=True)
        assert same_bits(got.cpu().numpy(), want(qs[0], "central")[0]), pin_once
        assert same_bits(hv1.cpu().numpy(), w1) and same_bits(f0.cpu().numpy(), wf0[0]), pin_once
        assert same_bits(hv2.cpu().numpy(), want(qs[1], "forward")[0]), pin_once


class FakeAtoms:
    """Minimal ASE-Atoms-like object (as in tests/test_gpu_calculator.py)."""

    def __init__(self, z, pos):
        self.numbers, self._p, self.info, self.calc = np.asarray(z), np.asarray(pos, dtype=float), {"charge": 0, "spin": 1}, None

    def get_positions(self):
        return self._p

    def get_atomic_numbers(self):
        return self.numbers


def test_the_calculators(eng, cases, monkeypatch):
    """``UMXCalculator.hvp`` (eV/A^2) and ``uma_pysis.get_hvp`` / ``UMAcore.hvp`` (Bohr in, Hartree/Bohr^2 out, frozen rows) on real engines
    against ``Engine.hvp`` on an engine of this test's own."""
    import importlib

    from pdb2reaction_amd import synth
    from pdb2reaction_amd._calculator_base import ANG2BOHR, BOHR2ANG
    from pdb2reaction_amd.ase_calculator import UMXCalculator

    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    c = cases["swap"]
    n, dirs = len(c["z"]), cases["swap"]["dirs"]
    calc = UMXCalculator(model="synthetic", task_name="omol")
    try:
        hv, curv = calc.hvp(FakeAtoms(c["z"], c["x"]), dirs, step=2e-3, scheme="forward", return_curvature=True)
    finally:
        calc.close()
    eng.set_system(c["z"])                                                   # the calculator's defaults: no cap
    eng.set_cell(None, None)
    want = eng.hvp(c["x"], dirs, step=2e-3, scheme="forward", return_curvature=True)
    assert same_bits(hv, want[0]) and same_bits(curv, want[1])
    U = importlib.import_module("pdb2reaction_amd.uma_pysis")
    frozen = [1, 4]
    up = U.uma_pysis(model="synthetic", max_neigh=c["max_neigh"], freeze_atoms=frozen)
    try:
        elem = [synth.SYMBOLS[int(a)] for a in c["z"]]
        x_bohr = (c["x"] * ANG2BOHR).reshape(-1)
        out = up.get_hvp(elem, x_bohr, dirs.reshape(3, -1), step_bohr=4e-3)["hvp"]
        full = up._ensure_core(elem).hvp(x_bohr.reshape(n, 3) * BOHR2ANG, dirs[:1])      # UMAcore.hvp: the full Hessian's product, eV/A^2
    finally:
        up.close()
    bind(eng, c)
    d = dirs.copy()
    d[:, frozen] = 0.0
    want = eng.hvp(x_bohr.reshape(n, 3) * BOHR2ANG, d, step=4e-3 * BOHR2ANG) * H.EV_PER_ANG2_TO_AU
    want[:, frozen] = 0.0
    assert out.shape == (3, 3 * n) and same_bits(out, want.reshape(3, -1)) and out.any()
    assert same_bits(full, eng.hvp(x_bohr.reshape(n, 3) * BOHR2ANG, dirs[:1])) and full[0, frozen].any()
