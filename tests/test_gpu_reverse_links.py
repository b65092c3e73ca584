"""The analytic reverse pass (K10), link by link, against float64 -- at the edge counts where its kernels change shape.

Every link is replayed on the CPU from the engine's OWN captured input (exactly as the GEMM / kernel read it: float32 quad-row blocks or PL
bf16 planes, odd rows negated) and compared with the engine's captured output.  No oracle forward pass, so a 44 k-edge system is affordable.
The float64 references are built from the FORWARD weight dict (transposed and conjugated here, never the engine's transposed / plane copies):
a wrong transpose, packing, offset or conj sign shows.

    conv-2^T  m0 / m1 / m2    gmsgq.i | gmsgpl.i | g_msg.i   ->  g_hid.i
    conv-1^T  m0 / m1 / m2    ghgq.i  | ghgpl.i  | g_hg.i    ->  g_y1.i
    fc3^T     (layer)         gradq.i | gradpl.i | g_rad.i   ->  g_a2.i
    fc3^T     (edge degree)   gradpl.deg (PL planes)         ->  g_a2.deg
    radial tail               g_a2, h1pre, h2pre, evec       ->  dedd_rad (accumulated over the layers: differences of the captures)

Per link and element: |C - C64| <= kappa(mode, K) * sum_k |a_k b_k| (tests/test_reverse_precision_cpu.py); per GEMM the precision statistic
(RMS of (C - C64) / sqrt(sum_k (a_k b_k)^2)) below t24(K) in bf16x3 and fp32 and ABOVE it in split-bf16 (the check can see 16-bit products);
in bf16x3 the quad-row conv GEMMs are also replayed on the bit-exact matrix-core model (tools/mfma_model.py, scheme "plain", plain planes:
the reverse weights are not aligned) and every output bit must come out -- all rows at S, a row subset at L (every output row depends only
on its own A row and its parity).  Host-side mutations of captured outputs check that the checker rejects what it must.

Sizes (preconditions asserted from ne below): S = 40 atoms, 1142 directed edges; L = 700 atoms, 44404 edges.  Host memory: UMX_DEBUG_ONLY
keeps only the captures used here (layers 0 and 3 at L: ~1 GB per layer and mode); the six cases run in ~80 s on the GPU box.
"""
import os
import sys

import numpy as np
import pytest
import torch

from pdb2reaction_amd import synth, weights as W
from oracle import tables as OT
from oracle.staged import ln_silu_bwd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gemm_ledger as GL  # noqa: E402
import mfma_model as MM  # noqa: E402
from test_reverse_precision_cpu import TWO_PLANE, U, kappa, link_stats, t24  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = {"S": 40, "L": 700}
LAYERS = {"S": (0, 1, 2, 3), "L": (0, 3)}          # L: two layers keep the float64 replays (and the host memory of the captures) affordable
ROW, HG, XROT, RAD = 1152, 1408, 2304, 1536
ODD = -1.0                                         # the engine's default sign-alternating rows (UMX_ALT_ROWS)

# (name, cplx, A columns of the re / im parts, output columns re / im, forward weight suffix, half, K of the link)
CONV2 = [("conv-2T m0", 0, (0, None), (0, None), "so2_conv_2.fc_m0.weight", 0),
         ("conv-2T m1", 1, (384, 640), (384, 640), "so2_conv_2.so2_m_conv.0.fc.weight", 256),
         ("conv-2T m2", 1, (896, 1024), (896, 1024), "so2_conv_2.so2_m_conv.1.fc.weight", 128)]
CONV1 = [("conv-1T m0", 0, (0, None), (0, None), "so2_conv_1.fc_m0.weight", 0),
         ("conv-1T m1", 1, (640, 896), (768, 1280), "so2_conv_1.so2_m_conv.0.fc.weight", 256),
         ("conv-1T m2", 1, (1152, 1280), (1792, 2048), "so2_conv_1.so2_m_conv.1.fc.weight", 128)]


def tile_regime(ne: int, cplx: int, n_out: int):
    """gemm_pl's dispatch (umx_api.hip, gemm_pl): rows per tile bmr = 128 (complex) / 256; 'fills' = ceil(M / bmr) * (N / (128 | 256)) >= 256;
    wide (256 x 256 tiles) when N is a multiple of 128 (complex) / 256 and the grid fills (no LS on reverse products).  Returns
    (wide capable, wide, row tiles)."""
    bmr, bn = (128, 128) if cplx else (256, 256)
    n_m = (ne + bmr - 1) // bmr
    capable = n_out % bn == 0
    return capable, capable and n_m * (n_out // bn) >= 256, n_m


def _unblock(raw, cols):
    rows = raw.size // cols
    return raw.reshape(rows // 4, cols // 16, 4, 16).transpose(0, 2, 1, 3).reshape(rows, cols)


def _planes(raw16, ne, cols, P):
    """PL layout (umx_gemm_pl.h): per row, per 32 columns, P bf16 planes of 32 -> the float64 sum of the planes [ne, cols]"""
    v = (raw16.astype(np.uint32) << 16).view(np.float32).astype(np.float64).reshape(ne, cols // 32, P, 32)
    return v.sum(2).reshape(ne, cols)


def _sign(ne):
    return np.where(np.arange(ne) % 2 == 1, ODD, 1.0)[:, None]


def _engine_run(precision, n_atoms, layers, monkeypatch):
    from pdb2reaction_amd.engine import Engine

    keep = ["dedd_rad", "evec", "g_a2.deg", "gradpl.deg", "h1pre.deg", "h2pre.deg"]
    for i in layers:
        keep += [f"{n}.{i}" for n in ("gmsgq", "gmsgpl", "g_msg", "g_hid", "ghgq", "ghgpl", "g_hg", "g_y1", "gradq", "gradpl", "g_rad", "g_a2",
                                      "h1pre", "h2pre")]
    monkeypatch.setenv("UMX_DEBUG_ONLY", ",".join(keep))
    w = W.make_synthetic_weights(0)
    z, pos = synth.make_cluster(n_atoms)
    eng = Engine(0, precision=precision)
    try:
        eng.load_weights(w)
        eng.set_system(z)
        eng.debug_keep(True)
        eng.energy_forces(pos.astype(np.float32), forces=True)
        cap = {"gemm:keys": GL.keys(eng, fwd=False)}
        for name in keep:
            try:
                cap[name] = eng.debug_fetch(name)
            except Exception:       # a name of another mode / layer
                pass
        for i in range(5):          # dedd_rad.* come under one prefix
            for t in (str(i), "deg"):
                try:
                    cap[f"dedd_rad.{t}"] = eng.debug_fetch(f"dedd_rad.{t}")
                except Exception:
                    pass
        return w, cap
    finally:
        eng.close()


def _conv_operand(cap, mode, link, i, ne):
    """(A as the link's GEMMs read it, un-negated, float64 [ne, cols]; the raw float32 rows for the model (bf16x3) or None)"""
    cols = ROW if link == "conv2" else HG
    if mode == "bf16x3":
        a32 = _unblock(cap[f"{'gmsgq' if link == 'conv2' else 'ghgq'}.{i}"], cols)[:ne] * _sign(ne).astype(np.float32)
        return a32.astype(np.float64), a32
    if mode == "split-bf16":
        return _planes(cap[f"{'gmsgpl' if link == 'conv2' else 'ghgpl'}.{i}"].view(np.uint16), ne, cols, 2) * _sign(ne), None
    return cap[f"{'g_msg' if link == 'conv2' else 'g_hg'}.{i}"].astype(np.float64).reshape(ne, cols), None


def _conv_refs(A, w, prefix, spec):
    """float64 (C64, sum|ab|, sum (ab)^2, K) per output part of one SO(2) conv^T link, from the FORWARD weights"""
    name, cplx, (ar, ai), _, suffix, half = spec
    Wf = np.asarray(w[f"{prefix}.{suffix}"], np.float64)
    if not cplx:
        a = A[:, ar:ar + Wf.shape[0]]
        return {name: (a @ Wf, np.abs(a) @ np.abs(Wf), (a * a) @ (Wf * Wf), Wf.shape[0])}
    are, aim = A[:, ar:ar + half], A[:, ai:ai + half]
    wa, wb = Wf[:half], Wf[half:]                   # forward: y_re = x_re.Wa^T - x_im.Wb^T, y_im = x_im.Wa^T + x_re.Wb^T; reverse: the adjoint
    aa, sq = np.abs, np.square
    return {name + " re": (are @ wa + aim @ wb, aa(are) @ aa(wa) + aa(aim) @ aa(wb), sq(are) @ sq(wa) + sq(aim) @ sq(wb), 2 * half),
            name + " im": (aim @ wa - are @ wb, aa(aim) @ aa(wa) + aa(are) @ aa(wb), sq(aim) @ sq(wa) + sq(are) @ sq(wb), 2 * half)}


def _out_cols(spec, part):
    _, cplx, _, (cr, ci), _, half = spec
    return (cr, ci)[part.endswith(" im")]


def _model(a32, w, prefix, spec, rows):
    """bit-exact model of the quad-row reverse GEMM (plain planes, scheme 'plain', odd rows negated by the model) on a row subset"""
    name, cplx, (ar, ai), _, suffix, half = spec
    Wf = np.asarray(w[f"{prefix}.{suffix}"], np.float32)
    run = lambda a, bt: MM.gemm_bf16x3(np.ascontiguousarray(a[rows]), np.ascontiguousarray(bt), None, "plain", alt_rows=True)   # noqa: E731
    if not cplx:
        return {name: run(a32[:, ar:ar + Wf.shape[0]], Wf.T)}
    are, aim = a32[:, ar:ar + half], a32[:, ai:ai + half]
    bta, btb = Wf[:half].T, Wf[half:].T
    p_ra, p_rb, p_ia, p_ib = run(are, bta), run(are, btb), run(aim, bta), run(aim, btb)
    return {name + " re": p_ra - np.float32(-1.0) * p_ib, name + " im": p_ia + np.float32(-1.0) * p_rb}     # the epilogue, conj = -1


def check_part(mode, K, c, ref, rows=slice(None)):
    """the per-element gross bound and the precision statistic of one output part -> (failures, gross, stat)"""
    c64, abs_sum, sq_sum = (x[rows] for x in ref[:3])
    try:
        gross, stat = link_stats(c[rows], c64, abs_sum, sq_sum)
    except AssertionError as e:
        return [str(e)], np.inf, np.inf
    bad = []
    if gross > kappa(mode, K):
        bad.append(f"gross {gross:.2e} > kappa {kappa(mode, K):.2e}")
    if mode == "split-bf16":
        if stat <= t24(K):
            bad.append(f"split-bf16 stat {stat:.2e} <= T24 {t24(K):.2e}: the check cannot see 16-bit products")
    elif stat > t24(K):
        bad.append(f"stat {stat:.2e} > T24 {t24(K):.2e}")
    return bad, gross, stat


def _replay_rows(ne):
    """L: the first row tile, the tiles either side of an 8-tile group boundary (complex: 128-row tiles, 1024; plain: 256-row, 2048) and the
    last partial tile -- all starting at even rows, so the model's row parity is the engine's"""
    last = ne // 256 * 256
    return np.concatenate([np.arange(0, 256), np.arange(896, 1152), np.arange(1792, 2304), np.arange(last, ne)])


@pytest.mark.parametrize("size", ["S", "L"])
@pytest.mark.parametrize("mode", ["bf16x3", "fp32", "split-bf16"])
def test_reverse_links_against_float64(mode, size, monkeypatch):
    """Measured on the MI355X (S and L alike; thresholds from tests/test_reverse_precision_cpu.py):
    * precision statistic: bf16x3 1.6e-7 (K 256) ... 3.5e-7 (K 384 / 640), fc3^T 6.2e-7 - 7.0e-7; fp32 2.1e-7 ... 4.6e-7, fc3^T 9.1e-7 - 9.6e-7;
      split-bf16 3.6e-6 - 3.8e-6 at every K -- 4.1 - 6.5 x T24 on the conv links, 2.7 x on fc3^T (T24 = 5.7e-7 ... 1.4e-6)
    * gross bound: max |C - C64| / sum|ab| <= 1.0e-6 (bf16x3), 1.5e-6 (fp32), 3.0e-6 (split-bf16) against kappa 1.2e-5 ... 9.2e-5
    * bf16x3 quad-row conv^T GEMMs: every bit equals the matrix-core model (layer 0, all 1142 rows at S, 1140 rows at L, narrow and wide tiles)
    * radial tail: max |error| / per-edge scale 6e-8 - 1.2e-7 in every mode (bound 2e-6), including the second pass of the persistent loop at L"""
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    layers = LAYERS[size]
    w, cap = _engine_run(mode, SIZES[size], layers, monkeypatch)
    ne = cap[f"g_hid.{layers[0]}"].size // ROW
    assert cap["gemm:keys"] == GL.KEYS_REVERSE_LINKS[(mode, size)], sorted(cap["gemm:keys"])     # the table rows this case holds (the ledger)
    print(f"\n[{mode} {size}] ne = {ne} (ne % 256 = {ne % 256}, ne % 4 = {ne % 4}), radial tiles of 64 edges: {(ne + 63) // 64}")
    # ---- coverage preconditions (a change to synth or to gemm_pl's dispatch must not drop them silently)
    regimes = {}
    for spec, N in [(s, n) for s, n in zip(CONV2, (384, 256, 128))] + [(s, n) for s, n in zip(CONV1, (768, 512, 256))]:
        regimes[spec[0]] = tile_regime(ne, spec[1], N)
        print(f"  {spec[0]}: {'wide' if regimes[spec[0]][1] else 'narrow'} tiles, {regimes[spec[0]][2]} row tiles")
    if size == "S":
        assert not any(r[1] for r in regimes.values()), regimes
        assert ne % 4 == 2 and ne % 256 != 0, ne
        assert (ne + 63) // 64 <= 512
    else:
        assert all(r[1] for r in regimes.values() if r[0]), regimes
        assert sum(r[0] for r in regimes.values()) == 5
        assert ne % 256 != 0 and any(r[2] % 8 for r in regimes.values()), ne
        assert (ne + 63) // 64 > 512, ne            # k_radial_head / k_radial_tail: grid capped at 512 tiles -> a second pass
    failures, exact_fail = [], []
    kept = {}
    for i in layers:
        b = f"blocks.{i}.edge_wise"
        outs = {"conv2": cap[f"g_hid.{i}"].reshape(ne, ROW), "conv1": cap[f"g_y1.{i}"].reshape(ne, XROT)}
        for link, specs in (("conv2", CONV2), ("conv1", CONV1)):
            A, a32 = _conv_operand(cap, mode, link, i, ne)
            for spec in specs:
                refs = _conv_refs(A, w, b, spec)
                model = None
                if mode == "bf16x3" and i == layers[0]:
                    rows = np.arange(ne) if size == "S" else _replay_rows(ne)
                    model = (rows, _model(a32, w, b, spec, rows))
                for part, ref in refs.items():
                    c0 = _out_cols(spec, part)
                    c = outs[link][:, c0:c0 + ref[0].shape[1]]
                    bad, gross, stat = check_part(mode, ref[3], c, ref)
                    line = f"  L{i} {part:14s} K {ref[3]:4d}: max |err|/sum|ab| {gross:.2e} (kappa {kappa(mode, ref[3]):.1e}), stat {stat:.2e} (T24 {t24(ref[3]):.2e})"
                    if model is not None:
                        rows, mo = model
                        nd = int((np.ascontiguousarray(mo[part]).view(np.uint32) != np.ascontiguousarray(c[rows]).view(np.uint32)).sum())
                        line += f", {nd} of {mo[part].size} bits-differ-from-model elements"
                        if nd:
                            exact_fail.append((i, part, nd))
                        kept[part] = (spec, ref, c, rows, mo[part], A, a32, np.asarray(w[f"{b}.{spec[4]}"], np.float64))
                    print(line)
                    failures += [(i, part, x) for x in bad]
        # ---- fc3^T of the layer
        if mode == "bf16x3":
            g = cap[f"gradq.{i}"].astype(np.float64).reshape(ne, RAD) * _sign(ne)
        elif mode == "split-bf16":
            g = _planes(cap[f"gradpl.{i}"].view(np.uint16), ne, RAD, 2) * _sign(ne)
        else:
            g = cap[f"g_rad.{i}"].astype(np.float64).reshape(ne, RAD)
        w3 = np.asarray(w[f"{b}.so2_conv_1.rad_func.fc3.weight"], np.float64)
        ref = (g @ w3, np.abs(g) @ np.abs(w3), (g * g) @ (w3 * w3), RAD)
        bad, gross, stat = check_part(mode, RAD, cap[f"g_a2.{i}"].reshape(ne, -1), ref)
        print(f"  L{i} fc3T           K {RAD}: max |err|/sum|ab| {gross:.2e} (kappa {kappa(mode, RAD):.1e}), stat {stat:.2e} (T24 {t24(RAD):.2e})")
        failures += [(i, "fc3T", x) for x in bad]
    # ---- fc3^T of the edge-degree MLP (PL planes in the plane modes)
    if mode != "fp32":
        P = 3 if mode == "bf16x3" else 2
        g = _planes(cap["gradpl.deg"].view(np.uint16)[:ne * 384 * P], ne, 384, P) * _sign(ne)
        w3 = np.asarray(w["edge_degree_embedding.rad_func.fc3.weight"], np.float64)
        ref = (g @ w3, np.abs(g) @ np.abs(w3), (g * g) @ (w3 * w3), 384)
        bad, gross, stat = check_part(mode, 384, cap["g_a2.deg"].reshape(ne, -1), ref)
        print(f"  deg fc3T         K  384: max |err|/sum|ab| {gross:.2e} (kappa {kappa(mode, 384):.1e}), stat {stat:.2e} (T24 {t24(384):.2e})")
        failures += [("deg", "fc3T", x) for x in bad]
    # ---- radial tails: dedd_rad after each tail, layers NL-1 ... 0, then the edge-degree MLP
    dist = cap["evec"].reshape(ne, 4)[:, 3].astype(np.float64)
    nb = OT.NUM_DISTANCE_BASIS
    mu = np.linspace(0.0, OT.CUTOFF, nb)
    gcoef = -0.5 / (2.0 * (OT.CUTOFF / (nb - 1))) ** 2
    gauss = np.exp(gcoef * (dist[:, None] - mu[None, :]) ** 2)
    dgauss = gauss * (2.0 * gcoef) * (dist[:, None] - mu[None, :])
    order = ["3", "2", "1", "0", "deg"]
    tags = [t for t in order if (t == "deg" or int(t) in layers)]
    for t in tags:
        prev = order[order.index(t) - 1] if t != "3" else None
        cur = cap[f"dedd_rad.{t}"].astype(np.float64)
        base = cap[f"dedd_rad.{prev}"].astype(np.float64) if prev else np.zeros(ne)
        prefix = "edge_degree_embedding.rad_func" if t == "deg" else f"blocks.{t}.edge_wise.so2_conv_1.rad_func"
        p = {k: torch.as_tensor(np.asarray(w[f"{prefix}.{k}"], np.float64)) for k in ("ln1.weight", "ln1.bias", "ln2.weight", "ln2.bias", "fc2.weight", "fc1.weight")}
        h1 = torch.as_tensor(cap[f"h1pre.{t}"].astype(np.float64).reshape(ne, -1))
        h2 = torch.as_tensor(cap[f"h2pre.{t}"].astype(np.float64).reshape(ne, -1))
        g_a2 = torch.as_tensor(cap[f"g_a2.{t}"].astype(np.float64).reshape(ne, -1))
        g_h2 = ln_silu_bwd(g_a2, h2, p["ln2.weight"], p["ln2.bias"])
        g_h1 = ln_silu_bwd(g_h2 @ p["fc2.weight"], h1, p["ln1.weight"], p["ln1.bias"])
        w1 = p["fc1.weight"][:, :nb].numpy()
        g_h1 = g_h1.numpy()
        d64 = ((g_h1 @ w1) * dgauss).sum(1)
        scale = (np.abs(g_h1) @ np.abs(w1) * np.abs(dgauss)).sum(1)          # per-edge magnitude of the last link
        err = np.abs((cur - base) - d64)
        tol = 2e-6 * scale + 4 * U * (np.abs(cur) + np.abs(base))            # + the float32 accumulation of dedd_rad over the layers
        print(f"  tail {t:3s}: max |err| / scale {float((err / np.maximum(scale, 1e-300)).max()):.2e}, edges over the bound {int((err > tol).sum())}")
        if (err > tol).any():
            failures.append((t, "radial tail", int((err > tol).sum())))
    assert not failures, failures
    assert not exact_fail, exact_fail
    if mode == "bf16x3":
        _mutation_checks(mode, ne, kept)


def _mutation_checks(mode, ne, kept):
    """Host-side mutations of captured outputs (no kernel changes): the checker must reject each."""
    # (1) one row of the last partial tile scaled by (1 + 2^-18): the model replay sees it
    spec, ref, c, rows, mo, A, a32, wf = kept["conv-1T m0"]
    cm = c.copy()
    r = ne - 3
    cm[r] *= np.float32(1.0 + 2.0 ** -18)
    sel = np.searchsorted(rows, r)
    assert rows[sel] == r
    assert (np.ascontiguousarray(mo[sel]).view(np.uint32) != np.ascontiguousarray(cm[r]).view(np.uint32)).any()
    # (2) the conj sign of one complex block flipped (conv-2^T m1 re computed with +conj): the float64 gross bound sees it
    spec, ref, c, rows, mo, A, a32, wf = kept["conv-2T m1 re"]
    half = spec[5]
    flipped = (ref[0] - 2.0 * (A[:, 640:640 + half] @ wf[half:])).astype(np.float32)     # x_re.Wa - x_im.Wb instead of + x_im.Wb
    bad, _, _ = check_part(mode, ref[3], flipped, ref)
    assert any("gross" in x for x in bad), bad
    # (3) the output replaced by the model's three-product (two-plane) result on the replayed rows: the precision statistic sees it
    spec, ref, c, rows, mo, A, a32, wf = kept["conv-1T m0"]
    wt = wf.astype(np.float32)
    c3 = MM.gemm_bf16x3(np.ascontiguousarray(a32[rows, :wt.shape[0]]), np.ascontiguousarray(wt.T), None, TWO_PLANE, alt_rows=True)
    cm = c.copy()
    cm[rows] = c3
    bad, _, stat = check_part(mode, ref[3], cm, ref, rows)
    print(f"  mutations: scaled row rejected; conj flip rejected; three products on {len(rows)} rows: stat {stat:.2e} -> {bad}")
    assert any("stat" in x for x in bad), bad
