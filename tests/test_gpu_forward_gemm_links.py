"""The forward GEMMs, link by link, against float64 and the matrix-core model -- at the edge counts where their kernels change shape, on
every row of the dispatch table, and across the `fills` seam of a batch.

Every product is replayed on the CPU from the engine's OWN captured input, exactly as the GEMM read it, and compared with the engine's
captured output.  The float64 references are built from the forward weight dict (bias included, the complex rule y_re = x_re.Wa^T - x_im.Wb^T,
y_im = x_im.Wa^T + x_re.Wb^T spelled here); the radial column that modulates an m-primary column of the fp32 mode's conv-1 operand follows
oracle/staged.py (`radx`).

    bf16x3   a2q.* -> rad.*      y1q.i -> hg.i              hidq.i -> msg.i     (float32 quad-row blocks, odd rows negated)
    fp32     a2.*  -> rad.*      (xrot.i * rad.i) -> hg.i   hid.i  -> msg.i

Per output part: |C - C64| <= kappa_fwd * (sum_k |a_k b_k| + |bias|) per element and the precision statistic below t24(K)
(tests/test_forward_gemm_precision_cpu.py); in bf16x3 every output bit equals tools/mfma_model.py's `gemm_bf16x3`, with the accumulation
scheme and the alignment of A's leading plane read from the launch log ("gemm:launches": ls, wide, al of that product), the two halves of
a complex part joined by one float32 subtract / add.  Which instantiation ran is asserted from the log, never from a copy of choose_pl.

Cases (edge counts asserted from graph_stats()):
    T1  17 atoms, max_neigh 3    51 edges   odd count, one partial tile, 4-row padding, the row-group clamp
    T2  13 atoms, max_neigh 5    65 edges   one row past the 64-edge complex half tile
    S   40 atoms               1142 edges   1142 % 4 = 2; 5 plain / 9 complex row tiles; complex products narrow; all layers + edge-degree MLP
    W  540 atoms              33042 edges   ceil(33042 / 128) = 259 >= 256: every complex forward product on wide tiles; 259 % 8 = 3;
                                            layer 0 and the edge-degree MLP (UMX_DEBUG_ONLY); float64 on all rows, the model on the first tile,
                                            64 rows of the tiles either side of an 8-tile group boundary and the last partial tile
The model replays a row subset wherever all rows would take minutes (a row's output depends on its own A row and its parity only): every
row at T1 / T2, the first 256-row tile and the last partial tile at S, the tiles named above at W; float64 holds every row.

Switch cases (bf16x3): one case for every table row that only UMX_LOW_SEP / UMX_ALIGN_PLANES / UMX_GEMM_HALF reach; their reverse conv^T
GEMMs go through tests/test_gpu_reverse_links.py's checker.  The ledger test requires the keys launched AND checked here, with those of
test_gpu_reverse_links and test_gpu_forward_links (tests/gemm_ledger.py), to be exactly "gemm:table".
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest
import torch

from pdb2reaction_amd import synth, weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gemm_ledger as GL  # noqa: E402
import mfma_model as MM  # noqa: E402
import test_gpu_reverse_links as RL  # noqa: E402
from test_forward_gemm_precision_cpu import LOW_ORDER, kappa_fwd, scheme_without  # noqa: E402
from test_reverse_precision_cpu import link_stats, t24  # noqa: E402
from test_gpu_reverse_links import _sign, _unblock  # noqa: E402

pytestmark = pytest.mark.gpu

ROW, HG, XROT, RAD, RH = 1152, 1408, 2304, 1536, 128
CASES = {"T1": (17, 3, 51), "T2": (13, 5, 65), "S": (40, None, 1142), "W": (540, None, 33042)}     # atoms, max_neigh, directed edges
LAYERS = {"T1": (0, 1, 2, 3), "T2": (0, 1, 2, 3), "S": (0, 1, 2, 3), "W": (0,)}

# (name, cplx, A columns re / im, C columns re / im, weight, bias, N (of one half), K (of one half))
CONV1 = (("conv-1 m0", 0, 0, None, 0, None, "so2_conv_1.fc_m0.weight", "so2_conv_1.fc_m0.bias", 640, 768),
         ("conv-1 m1", 1, 768, 1280, 640, 896, "so2_conv_1.so2_m_conv.0.fc.weight", None, 256, 512),
         ("conv-1 m2", 1, 1792, 2048, 1152, 1280, "so2_conv_1.so2_m_conv.1.fc.weight", None, 128, 256))
CONV2 = (("conv-2 m0", 0, 0, None, 0, None, "so2_conv_2.fc_m0.weight", "so2_conv_2.fc_m0.bias", 384, 384),
         ("conv-2 m1", 1, 384, 640, 384, 640, "so2_conv_2.so2_m_conv.0.fc.weight", None, 256, 256),
         ("conv-2 m2", 1, 896, 1024, 896, 1024, "so2_conv_2.so2_m_conv.1.fc.weight", None, 128, 128))
FC3 = ("fc3", 0, 0, None, 0, None, "so2_conv_1.rad_func.fc3.weight", "so2_conv_1.rad_func.fc3.bias", RAD, RH)
FC3_DEG = ("fc3 deg", 0, 0, None, 0, None, "rad_func.fc3.weight", "rad_func.fc3.bias", 384, RH)

# the table rows that only the documented switches reach, one case each (the issue's list); S unless the wide non-LS forms need W's M
SWITCH_CASES = [("S", dict(LOW_SEP=0, ALIGN=0, HALF=0)), ("S", dict(LOW_SEP=0, ALIGN=2, HALF=0)), ("S", dict(LOW_SEP=0, ALIGN=2, HALF=5)),
                ("S", dict(LOW_SEP=3, ALIGN=0, HALF=3)), ("S", dict(LOW_SEP=3, ALIGN=2, HALF=3)), ("S", dict(ALIGN=1, HALF=0)),
                ("S", dict(ALIGN=1, HALF=5)), ("S", dict(LOW_SEP=2, ALIGN=0, HALF=0)), ("S", dict(LOW_SEP=2, ALIGN=0, HALF=3)),
                ("S", dict(LOW_SEP=2, ALIGN=1, HALF=0)), ("S", dict(LOW_SEP=2, ALIGN=1, HALF=3)),
                ("W", dict(LOW_SEP=0, ALIGN=1, HALF=0)), ("W", dict(LOW_SEP=0, ALIGN=1, HALF=3))]
ENV = {"LOW_SEP": "UMX_LOW_SEP", "ALIGN": "UMX_ALIGN_PLANES", "HALF": "UMX_GEMM_HALF"}

HELD = {}            # key -> the first case of this file that launched it AND checked its output
DONE = set()         # the cases that have been checked
_RUNS = {}


def _sw_id(sw):
    return "-".join(f"{k}{v}" for k, v in sw.items()) or "default"


def _capture_names(mode, layers, rev):
    q = "q" if mode == "bf16x3" else ""
    keep = [f"a2{q}.deg", "rad.deg"]
    for i in layers:
        keep += [f"a2{q}.{i}", f"rad.{i}", f"hg.{i}", f"msg.{i}"]
        keep += [f"y1q.{i}", f"hidq.{i}"] if mode == "bf16x3" else [f"xrot.{i}", f"hid.{i}"]
        if rev:
            keep += [f"gmsgq.{i}", f"g_hid.{i}", f"ghgq.{i}", f"g_y1.{i}"]
    return keep


def _run(mode, case, sw, rev, monkeypatch):
    """one evaluation: (weights, captures, ne, launches), shared by the tests below and left unchanged"""
    k = (mode, case, _sw_id(sw), rev)
    if k in _RUNS:
        return _RUNS[k]
    from pdb2reaction_amd.engine import Engine

    n_atoms, max_neigh, ne_want = CASES[case]
    layers = LAYERS[case] if not sw else (0,)
    keep = _capture_names(mode, layers, rev)
    monkeypatch.setenv("UMX_DEBUG_ONLY", ",".join(keep))
    for name, v in sw.items():
        monkeypatch.setenv(ENV[name], str(v))
    w = W.make_synthetic_weights(0)
    z, pos = synth.make_cluster(n_atoms)
    eng = Engine(0, precision=mode)
    try:
        eng.load_weights(w)
        eng.set_system(z, max_neigh=max_neigh)
        eng.debug_keep(True)
        e, _ = eng.energy_forces(pos.astype(np.float32), forces=rev)
        assert np.all(np.isfinite(e))
        ne = eng.graph_stats()[0]
        assert ne == ne_want, (case, ne)                        # the edge count this case is about (module docstring)
        cap = {name: eng.debug_fetch(name) for name in keep}
        log, table = GL.launches(eng), GL.table(eng)
    finally:
        eng.close()
    _RUNS[k] = (w, cap, ne, log, table, layers, str(sw.get("ALIGN", 2)) != "0")       # (..., the weights' planes are aligned)
    return _RUNS[k]


def _product(log, fwd, cplx, N, K):
    """the launch-log key of one product: every launch of that shape (one per layer) must have taken the same instantiation"""
    hit = {x.key for x in log if x.fwd == fwd and GL.field(x.key, "cplx") == cplx and x.N == N and x.K == K}
    assert len(hit) == 1, (fwd, cplx, N, K, hit)
    return hit.pop()


def _scheme(key):
    return "plain" if not GL.field(key, "ls") else ("ls1" if GL.field(key, "wide") else "ls2")


def refs(A, Wf, bias, spec):
    """float64 {part: (C64, sum|ab| + |bias|, sum (ab)^2 + bias^2, K)} of one forward product from the forward weights"""
    name, cplx, ar, ai, _, _, _, _, N, K = spec
    aa, sq = np.abs, np.square
    if not cplx:
        a, b = A[:, ar:ar + K], (np.zeros(N) if bias is None else bias)[None, :]
        return {name: (a @ Wf.T + b, aa(a) @ aa(Wf).T + aa(b), sq(a) @ sq(Wf).T + sq(b), K)}
    are, aim, wa, wb = A[:, ar:ar + K], A[:, ai:ai + K], Wf[:N], Wf[N:]
    return {name + " re": (are @ wa.T - aim @ wb.T, aa(are) @ aa(wa).T + aa(aim) @ aa(wb).T, sq(are) @ sq(wa).T + sq(aim) @ sq(wb).T, 2 * K),
            name + " im": (aim @ wa.T + are @ wb.T, aa(aim) @ aa(wa).T + aa(are) @ aa(wb).T, sq(aim) @ sq(wa).T + sq(are) @ sq(wb).T, 2 * K)}


class Dem:
    """the model's plane alignment (tools/mfma_emul.c gemm_dem_*): A's leading plane, the weights' first and second planes"""

    def __init__(self):
        lib = MM.load_lib()
        self.v = [C.c_int.in_dll(lib, n) for n in ("gemm_dem_a", "gemm_dem_w", "gemm_dem_w2")]

    def set(self, a, w):
        self.v[0].value, self.v[1].value, self.v[2].value = a, w, w


def model(a32, Wf, bias, spec, rows, scheme, dem, al, alw):
    """the bit-exact model of one forward product on a row subset (contiguous pieces that start even, so the model's row parity is the
    engine's): the scheme and A's alignment as the launch log names them, the weights' planes aligned unless UMX_ALIGN_PLANES=0"""
    name, cplx, ar, ai, _, _, _, _, N, K = spec
    dem.set(12 if al else 0, 12 if alw else 0)
    try:
        run = lambda a, wt, b: MM.gemm_bf16x3(np.ascontiguousarray(a[rows]), np.ascontiguousarray(wt, np.float32), b, scheme, alt_rows=True)  # noqa: E731
        if not cplx:
            return {name: run(a32[:, ar:ar + K], Wf, None if bias is None else np.asarray(bias, np.float32))}
        are, aim = a32[:, ar:ar + K], a32[:, ai:ai + K]
        ra, rb, ia, ib = run(are, Wf[:N], None), run(are, Wf[N:], None), run(aim, Wf[:N], None), run(aim, Wf[N:], None)
        return {name + " re": ra - ib, name + " im": ia + rb}           # the epilogue's one float32 subtract / add
    finally:
        dem.set(0, 0)


def check(mode, form, staged, c, ref, rows=slice(None)):
    """the per-element gross bound and the precision statistic of one forward output part -> (failures, gross, stat)"""
    c64, abs_sum, sq_sum = (x[rows] for x in ref[:3])
    K = ref[3]
    try:
        gross, stat = link_stats(c[rows], c64, abs_sum, sq_sum)
    except AssertionError as e:
        return [str(e)], np.inf, np.inf
    bad = []
    if gross > kappa_fwd(mode, K, form, staged):
        bad.append(f"gross {gross:.2e} > kappa {kappa_fwd(mode, K, form, staged):.2e}")
    if stat > t24(K):
        bad.append(f"stat {stat:.2e} > T24 {t24(K):.2e}")
    return bad, gross, stat


def _even_pieces(pieces):
    for p in pieces[:-1]:
        assert p[0] % 2 == 0 and len(p) % 2 == 0, (p[0], len(p))
    assert pieces[-1][0] % 2 == 0
    return np.concatenate(pieces)


def model_rows(case, ne, cplx, light=False):
    """the rows the model replays (module docstring); light (switch cases): the first 64-row half tile in place of the first tile"""
    if case in ("T1", "T2"):
        return np.arange(ne)
    if case == "S":
        return _even_pieces([np.arange(0, 64 if light else 256), np.arange((1088 if light else 1024), ne)])
    t = 128 if cplx else 256                 # W: the row tile of the kind; 8-tile groups: 64 rows either side of the first group boundary
    return _even_pieces([np.arange(0, 64 if light else t), np.arange(8 * t - 64, 8 * t + 64), np.arange(ne // t * t, ne)])


def radx(rad):
    """the radial weight of every m-primary column of xrot, as oracle/staged.py spells it: [m0: 3 l | m1 re: 2 l | m1 im: the same 2 |
    m2 re: 1 | m2 im: the same 1] x 2C columns"""
    c2 = 2 * W.SPHERE_CHANNELS
    return np.concatenate([rad[:, :3 * c2], rad[:, 3 * c2:5 * c2], rad[:, 3 * c2:5 * c2], rad[:, 5 * c2:], rad[:, 5 * c2:]], axis=1)


def operands(mode, cap, i, ne):
    """{link: (A float64 un-negated, A float32 for the model | None)} of layer i (or "deg") as the GEMMs read them"""
    if mode == "bf16x3":
        sg = _sign(ne).astype(np.float32)
        get = lambda n, cols: _unblock(cap[n], cols)[:ne] * sg   # noqa: E731
        if i == "deg":
            a = get("a2q.deg", RH)
            return {"fc3": (a.astype(np.float64), a)}
        a, y1, hid = get(f"a2q.{i}", RH), get(f"y1q.{i}", XROT), get(f"hidq.{i}", ROW)
        return {"fc3": (a.astype(np.float64), a), "conv1": (y1.astype(np.float64), y1), "conv2": (hid.astype(np.float64), hid)}
    f8 = lambda n, cols: cap[n].astype(np.float64).reshape(ne, cols)   # noqa: E731
    if i == "deg":
        return {"fc3": (f8("a2.deg", RH), None)}
    return {"fc3": (f8(f"a2.{i}", RH), None), "conv1": (f8(f"xrot.{i}", XROT) * radx(f8(f"rad.{i}", RAD)), None), "conv2": (f8(f"hid.{i}", ROW), None)}


def check_forward(mode, case, run, light=False, tag=""):
    """every forward product of one run -> (report lines, failures, bit failures, kept for the mutations, keys checked)"""
    w, cap, ne, log, _, layers, alw = run
    dem = Dem() if mode == "bf16x3" else None
    lines, failures, exact_fail, kept, keys = [], [], [], {}, set()
    for i in ("deg",) + tuple(layers):
        prefix = "edge_degree_embedding" if i == "deg" else f"blocks.{i}.edge_wise"
        ops = operands(mode, cap, i, ne)
        outs = {"fc3": cap[f"rad.{i}"].reshape(ne, -1)}
        links = [("fc3", FC3_DEG if i == "deg" else FC3)]
        if i != "deg":
            outs.update(conv1=cap[f"hg.{i}"].reshape(ne, HG), conv2=cap[f"msg.{i}"].reshape(ne, ROW))
            links += [("conv1", s) for s in CONV1] + [("conv2", s) for s in CONV2]
        for link, spec in links:
            name, cplx, _, _, cre, cim, wname, bname, N, K = spec
            A, a32 = ops[link]
            Wf = np.asarray(w[f"{prefix}.{wname}"], np.float64)
            bias = None if bname is None else np.asarray(w[f"{prefix}.{bname}"], np.float64)
            rf = refs(A, Wf, bias, spec)
            key, form, mo = None, "plain", None
            if mode == "bf16x3":
                key = _product(log, True, cplx, N, K)
                form = _scheme(key)
                if i in ("deg", layers[0]):
                    rows = model_rows(case, ne, cplx, light)
                    mo = model(a32, Wf, bias, spec, rows, form, dem, GL.field(key, "al"), alw)
            staged = mode == "fp32" and link == "conv1"
            for part, ref in rf.items():
                c0 = cim if part.endswith(" im") else cre
                c = outs[link][:, c0:c0 + N]
                bad, gross, stat = check(mode, form, staged, c, ref)
                line = (f"  {tag}L{i} {part:13s} K {ref[3]:4d} {form:5s}: max |err|/(sum|ab|+|b|) {gross:.2e} (kappa {kappa_fwd(mode, ref[3], form, staged):.1e}), "
                        f"stat {stat:.2e} (T24 {t24(ref[3]):.2e})")
                if mo is not None:
                    nd = int((np.ascontiguousarray(mo[part]).view(np.uint32) != np.ascontiguousarray(c[rows]).view(np.uint32)).sum())
                    line += f", {nd} of {mo[part].size} differ from the model [{key}]"
                    if nd:
                        exact_fail.append((i, part, nd))
                    kept[part if i != "deg" else part + " deg"] = dict(spec=spec, ref=ref, c=c, rows=rows, mo=mo[part], A=A, a32=a32, Wf=Wf, bias=bias, form=form, key=key)
                elif mode == "fp32" and i == layers[0]:
                    kept[part] = dict(spec=spec, ref=ref, c=c, A=A, Wf=Wf, bias=bias, form=form)
                lines.append(line)
                failures += [(i, part, x) for x in bad]
            if key is not None:
                keys.add(key)
    return lines, failures, exact_fail, kept, keys


def check_reverse(run, case, tag=""):
    """the conv^T GEMMs of a bf16x3 run with forces through tests/test_gpu_reverse_links.py's checker: float64 on all rows, the model
    (plain scheme, plain planes: the reverse weights are not aligned) on the light row subset"""
    w, cap, ne, log, _, layers, _ = run
    i = layers[0]
    b = f"blocks.{i}.edge_wise"
    outs = {"conv2": cap[f"g_hid.{i}"].reshape(ne, ROW), "conv1": cap[f"g_y1.{i}"].reshape(ne, XROT)}
    lines, failures, exact_fail, keys = [], [], [], set()
    Dem().set(0, 0)
    for link, specs, widths in (("conv2", RL.CONV2, (384, 256, 128)), ("conv1", RL.CONV1, (768, 512, 256))):
        A, a32 = RL._conv_operand(cap, "bf16x3", link, i, ne)
        for spec, N in zip(specs, widths):
            rf = RL._conv_refs(A, w, b, spec)
            K = next(iter(rf.values()))[3] // (2 if spec[1] else 1)
            key = _product(log, False, spec[1], N, K)
            assert GL.field(key, "fam") == "Q_BF16" and not GL.field(key, "ls") and not GL.field(key, "al"), key
            rows = model_rows(case, ne, spec[1], light=True)
            mo = RL._model(a32, w, b, spec, rows)
            for part, ref in rf.items():
                c0 = RL._out_cols(spec, part)
                c = outs[link][:, c0:c0 + ref[0].shape[1]]
                bad, gross, stat = RL.check_part("bf16x3", ref[3], c, ref)
                nd = int((np.ascontiguousarray(mo[part]).view(np.uint32) != np.ascontiguousarray(c[rows]).view(np.uint32)).sum())
                lines.append(f"  {tag}L{i} {part:13s} K {ref[3]:4d}: max |err|/sum|ab| {gross:.2e}, stat {stat:.2e} (T24 {t24(ref[3]):.2e}), {nd} of {mo[part].size} differ "
                             f"from the model [{key}]")
                failures += [(i, part, x) for x in bad]
                if nd:
                    exact_fail.append((i, part, nd))
            keys.add(key)
    return lines, failures, exact_fail, keys


def _hold(keys, who):
    DONE.add(who)
    for k in keys:
        HELD.setdefault(k, who)


def _regime_asserts(mode, case, log):
    """coverage preconditions, from the launch log (a change to synth or to choose_pl must not drop them silently)"""
    if mode != "bf16x3":
        assert not log, log                                    # the fp32 mode launches no plane GEMM
        return
    fwd = [x for x in log if x.fwd]
    assert len(fwd) == 1 + 7 * W.NUM_LAYERS and all(x.M == CASES[case][2] for x in fwd), fwd      # one chunk, every product on all the edges
    cw = {(x.N, x.K): GL.field(x.key, "wide") for x in fwd if GL.field(x.key, "cplx")}
    assert len(cw) == 4, cw
    if case == "W":
        assert all(cw.values()), cw                            # every complex forward product on 256-wide tiles
    else:
        assert not any(cw.values()), cw
    for x in fwd:                                              # default switches: LS on the plain products, its tile from N alone
        if not GL.field(x.key, "cplx"):
            assert GL.field(x.key, "ls") == 1 and GL.field(x.key, "wide") == (x.N % 256 == 0), x


@pytest.mark.parametrize("case", ["T1", "T2", "S", "W"])
@pytest.mark.parametrize("mode", ["bf16x3", "fp32"])
def test_forward_gemms_against_float64_and_the_model(mode, case, monkeypatch):
    """Measured on the MI355X (profiles/forward_gemm_links.txt; thresholds from tests/test_forward_gemm_precision_cpu.py):
    * bf16x3: every replayed output bit equals the model (51 and 65 rows: all; 1142: 374 rows; 33042: 402 / 274 rows per plain / complex
      product), narrow and wide tiles, LS = 1 and LS = 2; statistic 0.28 ... 0.39 of T24, gross <= 5.7e-7 against kappa >= 6.3e-6
    * fp32: statistic 0.35 ... 0.65 of T24 (the largest: conv-1 m0, K 768, operand modulated while staged), gross <= 1.3e-6 against
      kappa >= 8.1e-6
    * time per case: T1 5 s (builds the model library), T2 2.5 s, S 8 s, W 8 s in bf16x3; 0.2 / 0.2 / 0.5 / 4 s in fp32"""
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    t0 = time.time()
    run = _run(mode, case, {}, False, monkeypatch)
    w, cap, ne, log, table, layers, _ = run
    print(f"\n[{mode} {case}] ne = {ne} (ne % 4 = {ne % 4}, plain / complex row tiles {(ne + 255) // 256} / {(ne + 127) // 128})")
    _regime_asserts(mode, case, log)
    lines, failures, exact_fail, kept, keys = check_forward(mode, case, run)
    print("\n".join(lines))
    assert not failures, failures
    assert not exact_fail, exact_fail
    _hold(keys, f"{mode} {case}")
    if case in ("S", "T1"):
        _mutations(mode, run, kept)
    print(f"  [{mode} {case}] {time.time() - t0:.1f} s")


@pytest.mark.parametrize("case,sw", SWITCH_CASES, ids=[f"{c}-{_sw_id(s)}" for c, s in SWITCH_CASES])
def test_switch_rows_against_float64_and_the_model(case, sw, monkeypatch):
    """The table rows that only UMX_LOW_SEP / UMX_ALIGN_PLANES / UMX_GEMM_HALF reach: forward and reverse conv^T GEMMs of layer 0 (and the
    edge-degree fc3) of a run with forces.  Measured on the MI355X: no differing bit in any of the 13 cases, forward or reverse; the largest
    forward statistic 0.52 of T24 (conv-1 m0 without LS); 4 - 5 s per case at S, 13 s at W (the float64 products of 33042 rows, both passes)."""
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    t0 = time.time()
    run = _run("bf16x3", case, sw, True, monkeypatch)
    tag = f"[{_sw_id(sw)}] "
    print(f"\n[bf16x3 {case} {_sw_id(sw)}] ne = {run[2]}; keys launched: {sorted({x.key for x in run[3]})}")
    lines, failures, exact_fail, _, keys = check_forward("bf16x3", case, run, light=(case == "S"), tag=tag)
    rl, rf, re_, rkeys = check_reverse(run, case, tag=tag)
    print("\n".join(lines + rl))
    assert not failures and not rf, (failures, rf)
    assert not exact_fail and not re_, (exact_fail, re_)
    _hold(keys | rkeys, f"bf16x3 {case} {_sw_id(sw)}")
    print(f"  [bf16x3 {case} {_sw_id(sw)}] {time.time() - t0:.1f} s")


def _mutations(mode, run, kept):
    """Host-side mutations of captured outputs (no kernel changes): the checker must reject each."""
    cap, ne, i0 = run[1], run[2], run[5][0]
    staged = lambda k: mode == "fp32" and k.startswith("conv-1")   # noqa: E731
    rej = []
    # (1) the bias missing from one 32-column block of a plain product: the gross bound sees it
    k = kept["conv-1 m0"]
    cm = k["c"].copy()
    cm[:, 32:64] -= k["bias"][32:64].astype(np.float32)
    bad, _, _ = check(mode, k["form"], staged("conv-1 m0"), cm, k["ref"])
    assert any("gross" in x for x in bad), bad
    rej.append("bias block")
    # (2) the re and im halves of one 32-column block of a complex product swapped
    kr, ki = kept["conv-2 m1 re"], kept["conv-2 m1 im"]
    cm = kr["c"].copy()
    cm[:, 64:96] = ki["c"][:, 64:96]
    bad, _, _ = check(mode, kr["form"], False, cm, kr["ref"])
    assert any("gross" in x for x in bad), bad
    rej.append("re / im swap")
    # (3) fp32: conv-1 m1 modulated with the m2 radial columns (SO2_RAD_M2 in place of SO2_RAD_M1)
    if mode == "fp32":
        k = kept["conv-1 m1 re"]
        spec = k["spec"]
        N, K = spec[8], spec[9]
        # the m1 block of xrot times the m2 radial columns (256 of them, met by both l of m = 1) instead of its own 512
        xr = cap[f"xrot.{i0}"].astype(np.float64).reshape(ne, XROT)
        r2 = np.tile(cap[f"rad.{i0}"].astype(np.float64).reshape(ne, RAD)[:, 1280:1536], 2)
        are, aim = xr[:, 768:1280] * r2, xr[:, 1280:1792] * r2
        wrong = (are @ k["Wf"][:N].T - aim @ k["Wf"][N:].T).astype(np.float32)
        bad, _, _ = check(mode, k["form"], True, wrong, k["ref"])
        assert any("gross" in x for x in bad), bad
        rej.append("m2 radial columns on m1")
    # (4) the last row of the partial tile replaced by the row before it; (5) a lost odd-row sign in one row
    k = kept["conv-2 m0"]
    for what, r, val in (("last row", ne - 1, k["c"][ne - 2]), ("row sign", ne - (2 if ne % 2 else 1) - 2, None)):
        cm = k["c"].copy()
        cm[r] = -cm[r] if val is None else val
        assert what != "row sign" or r % 2 == 1
        bad, _, _ = check(mode, k["form"], False, cm, k["ref"])
        assert any("gross" in x for x in bad), (what, bad)
        if mode == "bf16x3":
            sel = int(np.searchsorted(k["rows"], r))
            assert k["rows"][sel] == r and (np.ascontiguousarray(k["mo"][sel]).view(np.uint32) != np.ascontiguousarray(cm[r]).view(np.uint32)).any()
        rej.append(what)
    # (6) bf16x3: the model's five-product result written over the replayed rows: the precision statistic sees a lost plane product
    if mode == "bf16x3":
        dem = Dem()
        for name in ("conv-1 m0", "fc3"):
            k = kept[name]
            for drop in LOW_ORDER:
                sub = k["rows"][:64]
                c5 = model(k["a32"], k["Wf"], k["bias"], k["spec"], sub, scheme_without(k["form"], drop), dem, GL.field(k["key"], "al"), True)[name]
                cm = k["c"].copy()
                cm[sub] = c5
                bad, _, stat = check(mode, k["form"], False, cm, k["ref"], sub)
                assert any("stat" in x for x in bad), (name, drop, stat, bad)
        rej.append("five products")
    print(f"  mutations rejected: {', '.join(rej)}")


def test_every_table_row_is_launched_and_checked(monkeypatch):
    """The ledger: the keys this file's cases launched and checked, with those tests/test_gpu_reverse_links.py and
    tests/test_gpu_forward_links.py launch (asserted there against tests/gemm_ledger.py), are exactly the rows of `pl_kernels`."""
    for mode in ("bf16x3",):
        for case in ("T1", "T2", "S", "W"):
            run = _run(mode, case, {}, False, monkeypatch)
            if f"{mode} {case}" not in DONE:
                _, failures, exact_fail, _, keys = check_forward(mode, case, run)
                assert not failures and not exact_fail
                _hold(keys, f"{mode} {case}")
    for case, sw in SWITCH_CASES:
        who = f"bf16x3 {case} {_sw_id(sw)}"
        if who not in DONE:
            with monkeypatch.context() as mp:
                run = _run("bf16x3", case, sw, True, mp)
                _, failures, exact_fail, _, keys = check_forward("bf16x3", case, run, light=(case == "S"))
                _, rf, re_, rkeys = check_reverse(run, case)
            assert not failures and not rf and not exact_fail and not re_
            _hold(keys | rkeys, who)
    table = _run("bf16x3", "S", {}, False, monkeypatch)[4]
    assert len(table) == len(set(table)) == 39, table
    other = GL.held_elsewhere()
    print()
    for row in table:
        print(f"  {row:24s} {HELD.get(row) or ('test_gpu_reverse_links / test_gpu_forward_links' if row in other else 'NOT HELD')}")
    missing = [r for r in table if r not in HELD and r not in other]
    assert not missing, f"table rows that no case launches and checks: {missing}"
    assert (set(HELD) | other) == set(table), sorted((set(HELD) | other) ^ set(table))


# ---- batch independence across the tile-width seam -------------------------------------------------
BATCH_CAPS = ("rad", "hg", "msg", "g_hid", "g_y1")
BATCH_COLS = {"rad": RAD, "hg": HG, "msg": ROW, "g_hid": ROW, "g_y1": XROT}


def _batch_eval(mode, z, pos, layers, monkeypatch):
    from pdb2reaction_amd.engine import Engine

    keep = [f"{n}.{i}" for i in layers for n in BATCH_CAPS]
    monkeypatch.setenv("UMX_DEBUG_ONLY", ",".join(keep))
    eng = Engine(0, precision=mode)
    try:
        eng.load_weights(W.make_synthetic_weights(0))
        eng.set_system(z)
        eng.debug_keep(True)
        out = []
        for p in [pos] + [pos[k] for k in range(len(pos))]:
            e, f = eng.energy_forces(p.astype(np.float32), forces=True)
            out.append(dict(e=e, f=f, ne=eng.graph_stats()[0], log=GL.launches(eng), cap={n: eng.debug_fetch(n) for n in keep}))
        return out
    finally:
        eng.close()


def _batch_compare(out, layers):
    batch, singles = out[0], out[1:]
    assert batch["ne"] == sum(s["ne"] for s in singles)
    assert all(x.M == batch["ne"] for x in batch["log"]), "the batch ran in more than one chunk"
    r0, differ = 0, []
    for k, s in enumerate(singles):
        if not (batch["e"][k] == s["e"][0] and np.array_equal(batch["f"][k], s["f"][0])):
            differ.append((k, "E / F"))
        for i in layers:
            for n in BATCH_CAPS:
                cols = BATCH_COLS[n]
                b = batch["cap"][f"{n}.{i}"].reshape(-1, cols)[r0:r0 + s["ne"]]
                a = s["cap"][f"{n}.{i}"].reshape(-1, cols)
                nd = int((b.view(np.uint32) != a.view(np.uint32)).sum())
                if nd:
                    differ.append((k, f"{n}.{i}", nd))
        r0 += s["ne"]
    return differ


@pytest.mark.parametrize("mode", ["bf16x3", "split-bf16", "split"])
def test_two_image_batch_at_an_unaligned_seam_equals_single(mode, monkeypatch):
    """Image 1 starts at row 1142: inside a quad-row block (1142 % 4 = 2) and inside a tile.  rad, hg, msg, g_hid, g_y1, E and F of each
    image equal the image evaluated alone, bit for bit."""
    z, pos0 = synth.make_cluster(40)
    pos = np.stack([pos0, pos0 + 0.02 * np.random.default_rng(3).standard_normal(pos0.shape)])
    layers = (0, 1, 2, 3)
    out = _batch_eval(mode, z, pos, layers, monkeypatch)
    assert out[1]["ne"] == 1142 and out[1]["ne"] % 4 == 2 and out[1]["ne"] % 64 != 0, out[1]["ne"]
    differ = _batch_compare(out, layers)
    print(f"\n[{mode}] two images, {out[1]['ne']} + {out[2]['ne']} edges: captures / results that differ from the single runs: {differ}")
    assert not differ, differ


@pytest.mark.parametrize("mode", ["bf16x3", "split-bf16", "split"])
def test_three_image_batch_across_the_fills_seam_equals_single(mode, monkeypatch):
    """Three images of the 150-atom cluster: alone (7224 edges) every complex product runs on narrow tiles, in the batch (21672 edges) the
    N = 256 and N = 512 complex products of both passes run wide -- both regimes asserted from the launch log -- and every image gets the
    same bits.  Measured on the MI355X: no difference in any mode, although narrow and wide are different instantiations (Q_BF16 / Q_F16
    forward, Q_BF16 / PL2_M16 -> PL2_WIDE reverse)."""
    z, pos0 = synth.make_cluster(150)
    rng = np.random.default_rng(4)
    pos = np.stack([pos0] + [pos0 + 0.01 * rng.standard_normal(pos0.shape) for _ in range(2)])
    layers = (0, 3)
    out = _batch_eval(mode, z, pos, layers, monkeypatch)
    assert out[1]["ne"] == 7224, out[1]["ne"]
    wide = lambda o: {(x.fwd, x.N): GL.field(x.key, "wide") for x in o["log"] if GL.field(x.key, "cplx")}   # noqa: E731
    for s in out[1:]:
        assert not any(wide(s).values()), wide(s)
    wb = wide(out[0])
    assert {N for _, N in wb} == {128, 256, 512}, wb                    # (N = 512: conv-1^T m1 of the reverse pass)
    assert all(v == (N != 128) for (_, N), v in wb.items()), wb
    print(f"\n[{mode}] batch keys {sorted({x.key for x in out[0]['log']})}\n[{mode}] single keys {sorted({x.key for x in out[1]['log']})}")
    differ = _batch_compare(out, layers)
    print(f"[{mode}] three images of 7224 edges: captures / results that differ from the single runs: {differ}")
    assert not differ, differ
