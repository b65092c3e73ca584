"""The radial head and the fp16 forward path of the fast mode, link by link, against float64.

tests/test_gpu_reverse_links.py, test_gpu_edge_links.py and test_gpu_node_links.py replay the reverse pass, the edge kernels between the GEMMs
and the node-level kernels; tests/test_gpu_mfma_model.py pins the bf16x3 forward GEMMs bit for bit.  They take h1pre / h2pre / a2q as given
and say nothing about the fast mode's fp16 operands.  Here, from the engine's OWN captured inputs, element by element, no oracle forward pass:

  Part A  k_radial_head, three links per radial MLP (edge degree + every layer), modes bf16x3 (a2q), fp32 (a2), split (a2h)
    A1  (d = evec[:, 3], Z[src], Z[dst])  -> h1pre      gaussians (double centres, exponent rounded once), fc1 on the fp32 MFMA, double tables
    A2  h1pre                             -> h2pre      hi + lo LayerNorm, SiLU, fc2 seeded with its bias
    A3  h2pre                             -> a2q | a2 | a2h   LayerNorm, SiLU, row sign, operand store
  Part B  the fp16 "Q2H" operand planes (split): y1h.i (k_gather_rotate_mod_q3<1>), hidh.i (k_gate_edge_fwd_q3<1>), a2h.* (k_radial_head<2>):
          decoded by the layout rule of umx_edge.h, against the float64 replays of tests/test_gpu_edge_links.py; the split law
  Part C  the fp16 forward GEMM umx_gemm_q_kernel<CPLX, WIDE, 2, 2, 1, 4, 3> (split): A exactly as captured (hi and lo planes apart), B planes
          rebuilt on the host from the float32 weight by the rule of umx_weights.h, float64 sum of exactly the four products; the projection
          statistic ("gain") of A_hi . B_lo2 and of A_lo . B_hi

Formulas: oracle.Oracle.edge_scalars, oracle.layer_norm / silu / radial_mlp's spelling, oracle.staged.silu_grad, oracle/tables.py, or written
plainly below (tests/test_forward_links_cpu.py asserts the plain ones equal the oracle's); none is transcribed from a kernel.

Sizes (SIZES of test_gpu_edge_links.py; preconditions asserted from the captured row_ptr / ne): T1 = 17 atoms, max_neigh 3, 51 edges (odd
count, one partial 64-edge tile, 4-row padding); S = 40 atoms, 1142 edges (ne % 64 = 54); L = 700 atoms, 44404 edges = 694 tiles > 512: the
persistent loop of k_radial_head takes a second pass (edge-degree MLP and layer 0 only).  Every system holds >= 3 elements and some element
pair occurs as (Z_src, Z_dst) in both orders with different source / target embedding rows: a src / dst swap is visible.

Bounds, per element, nothing relative to a tensor's maximum, no element excluded (u = 2^-24, gamma_k = k u / (1 - k u)); each k is derived
beside its link below.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import escn_md_oracle as O
from oracle import tables as OT
from oracle.staged import silu_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gemm_ledger as GL  # noqa: E402
import test_gpu_edge_links as EL  # noqa: E402
from test_gpu_edge_links import HG, RAD, ROW, SIZES, T64, U, XROT, Graph, Report, _t, gamma, host_ulps, ratio  # noqa: E402
from test_gpu_reverse_links import _unblock  # noqa: E402

pytestmark = pytest.mark.gpu

C, H, NL = OT.SPHERE_CHANNELS, OT.HIDDEN_CHANNELS, OT.NUM_LAYERS
RH, NG = OT.RADIAL_HIDDEN, OT.NUM_DISTANCE_BASIS
LAYERS = {"T1": (0, 1, 2, 3), "S": (0, 1, 2, 3), "L": (0,)}
TILE = 256                    # rows of one GEMM tile (Part C subsamples whole tiles at L)
MODES = {"bf16x3": "a2q", "fp32": "a2", "split": "a2h"}


def rad_prefix(tag):
    return "edge_degree_embedding.rad_func" if tag == "deg" else f"blocks.{tag}.edge_wise.so2_conv_1.rad_func"


class Radial:
    """the float64 parameters of one radial MLP, from the forward weight dict"""

    def __init__(self, p, prefix):
        g = lambda n: p[f"{prefix}.{n}"]     # noqa: E731
        self.W1, self.b1, self.W2, self.b2 = g("fc1.weight"), g("fc1.bias"), g("fc2.weight"), g("fc2.bias")
        self.ln1w, self.ln1b, self.ln2w, self.ln2b = g("ln1.weight"), g("ln1.bias"), g("ln2.weight"), g("ln2.bias")
        self.W3, self.b3 = g("fc3.weight"), g("fc3.bias")


# ---- Part A ------------------------------------------------------------------------------------------------------------------------------
def gauss_centres(cutoff=OT.CUTOFF):
    return torch.linspace(0.0, cutoff, NG, dtype=T64)


def gauss_exponent(d, mu=None, cutoff=OT.CUTOFF):
    """x_k = coeff (d - mu_k)^2, centres and coefficient as oracle.Oracle.edge_scalars spells them"""
    mu = gauss_centres(cutoff) if mu is None else mu
    coeff = -0.5 / (2.0 * (cutoff / (NG - 1))) ** 2
    return coeff * (d[:, None] - mu[None, :]) ** 2


def measure_k_exp(x):
    """the distance of numpy's float32 exp from float64 on the exponents the kernel rounds to float32, in u of the gaussian (normal range)"""
    x32 = x.numpy().astype(np.float32)
    g64 = np.exp(x32.astype(np.float64))
    live = g64 >= 2.0 ** -126
    return float((np.abs(np.exp(x32).astype(np.float64) - g64)[live] / (U * g64[live])).max())


def link_fc1(orc, R, d, zs, zd, k_exp, mu=None, bias=True):
    """A1.  h1pre = x_edge fc1.weight^T + fc1.bias, x_edge = oracle.edge_scalars.  The kernel: exponent x_k rounded to float32 once (|x_k| u
    relative on the gaussian), expf (k_exp u), a 64-term fma chain on the fp32 MFMA from 0 (gamma_64 on sum |W g|); the element tables are added
    in double and the sum is rounded once (u |ref|); gaussians below 2^-126 are on float32's subnormal grid (floor 2^-126 sum |W1g|).
    mu / bias: the mutations (float32 centres; fc1 bias omitted)."""
    x = gauss_exponent(d, mu, orc.cutoff)
    xe = orc.edge_scalars(d, zs, zd)
    if mu is not None:
        xe = torch.cat([torch.exp(x), xe[:, NG:]], dim=1)
    ref = xe @ R.W1.T + (R.b1 if bias else 0.0)
    W1g = R.W1[:, :NG].abs()
    bound = (xe[:, :NG] * ((x.abs() + k_exp) * U + gamma(64))) @ W1g.T + U * ref.abs() + 2.0 ** -126 * W1g.sum(1)[None, :]
    return ref, bound


def projection_gain(out, base, term):
    """the project's projection statistic: <out - base, term> / <term, term> -- 1 if `out` holds `term` on top of `base`, 0 if it does not"""
    return float(((out - base) * term).sum() / (term * term).sum())


def ln_parts(h, eps=OT.LN_EPS):
    """LayerNorm written plainly (oracle.layer_norm): centred row, 1 / sqrt(var + eps), normalised row"""
    v = h - h.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((v ** 2).mean(-1, keepdim=True) + eps)
    return v, rstd, v * rstd


def ln_silu(h, w, b, e_in, kh, eps=OT.LN_EPS):
    """a = SiLU(LayerNorm(h) w + b) in float64 and the bound of its float32 evaluation, e_in = what is not known about the input, per element.

    mean: pair sum + 6-level DPP wave sum of hi and of lo, their sum, x 1/128 (exact): 9 roundings, gamma_9 mean|h|;  centred value: formed in
    double, rounded once: u |v|.  These and e_in are perturbations e_j of the row; to first order they reach the normalised row through the
    Jacobian of the oracle's layer_norm, d xh_i / d h_j = rstd (delta_ij - 1/n - xh_i xh_j / n), bounded term by term:
        |d xh_i| <= rstd (e_i + mean e + |xh_i| mean(|xh| e)).
    rstd itself: var = 128 squares, pair sum, wave sum (all positive: relative gamma_8, halved by the power -1/2: 4), var + eps (1, its error
    carried along), sqrt and division (2), the fma that applies it (1): 8 u |xh_i|.  y = xh w + b: two roundings, 2 u (|xh w| + |b|).
    SiLU: y * (1 / (1 + expf(-y))) is one rounding longer than the formula host_ulps measures: (1 + 2 k_host) u |y| sigmoid(y), the convention
    of tests/test_gpu_edge_links.py; the perturbation of y goes through |SiLU'| (oracle.staged.silu_grad)."""
    v, rstd, xh = ln_parts(h, eps)
    e = e_in + gamma(9) * h.abs().mean(-1, keepdim=True) + U * v.abs()
    dxh = rstd * (e + e.mean(-1, keepdim=True) + xh.abs() * (xh.abs() * e).mean(-1, keepdim=True)) + 8 * U * xh.abs()
    y = xh * w + b
    dy = w.abs() * dxh + 2 * U * ((xh * w).abs() + b.abs())
    a = O.silu(y)
    return a, silu_grad(y).abs() * dy + (1 + 2 * kh) * U * y.abs() * torch.sigmoid(y), y


def link_fc2(R, h1, kh, eps=OT.LN_EPS, bias_last_sign=1.0):
    """A2.  h2pre = SiLU(LN(h1pre)) fc2.weight^T + fc2.bias.  The kernel normalises hi + lo and stores hi only: the input is known to u |h1_j|
    (e_in).  fc2: a 128-term fma chain started from the bias: gamma_128 (|b| + sum |W a|), and |W2| times the bound of a.
    eps / bias_last_sign: the mutations (LN eps omitted; the bias added last with the wrong sign)."""
    a, da, y = ln_silu(h1, R.ln1w, R.ln1b, U * h1.abs(), kh, eps)
    ref = a @ R.W2.T + bias_last_sign * R.b2
    return ref, gamma(128) * (R.b2.abs() + a.abs() @ R.W2.abs().T) + da @ R.W2.abs().T, y


def link_a2(R, h2, kh, eps=OT.LN_EPS):
    """A3.  The fc3 operand SiLU(LN(h2pre)): h2pre is stored as it is normalised (e_in = 0; the lo sums are absent: gamma_9 covers the 8
    roundings left).  The row sign is a product with +-1: exact."""
    a, da, y = ln_silu(h2, R.ln2w, R.ln2b, torch.zeros_like(h2), kh, eps)
    return a, da, y


def add(rep, name, k, out, ref, bound):
    """Report.add, and a failure for any non-finite captured value: a NaN compares False against its bound and would count as inside it"""
    bad = int((~torch.isfinite(out)).sum())
    if bad:
        rep.failures.append((name, f"{bad} non-finite values in the captured output"))
    return rep.add(name, k, out, ref, bound)


def asserted(muts):
    return {n: r for n, r in muts.items() if not n.startswith("info:")}


def silu_k_host(y):
    return host_ulps(y.numpy().astype(np.float32))["silu"]


# ---- Part B: the Q2H decoder, written from the layout comment of umx_edge.h ----------------------------------------------------------
def q2h_index(rows, cols, q, plane_bytes=32):
    """index, in halves, of element (r, k, plane q) of a `cols`-wide matrix: byte ((r/4)(cols/16) + k/16) 256 + (r%4) 64 + q 32 + (k%16) 2"""
    r, k = np.asarray(rows, np.int64)[:, None], np.arange(cols, dtype=np.int64)[None, :]
    return (((r // 4) * (cols // 16) + k // 16) * 256 + (r % 4) * 64 + q * plane_bytes + (k % 16) * 2) // 2


def q2h_decode(raw16, rows, cols, plane_bytes=32, swap=False, signed=True):
    """(hi, lo) of the rows `rows` as float64, in half units (value = (hi + lo) / 16), odd rows un-negated"""
    hi = raw16[q2h_index(rows, cols, 0, plane_bytes)].view(np.float16).astype(np.float64)
    lo = raw16[q2h_index(rows, cols, 1, plane_bytes)].view(np.float16).astype(np.float64)
    if swap:
        hi, lo = lo, hi
    sg = np.where(np.asarray(rows) % 2 == 1, -1.0, 1.0)[:, None] if signed else 1.0
    return hi * sg, lo * sg


def q2h_encode(x32, odd_sign=-1.0):
    """the host image of the producers' store: two RNE half planes of 16 x, rows padded to 4, odd rows negated"""
    rows, cols = x32.shape
    r4 = (rows + 3) // 4 * 4
    xs = np.float32(16.0) * (x32.astype(np.float32) * np.where(np.arange(rows) % 2 == 1, np.float32(odd_sign), np.float32(1.0))[:, None])
    with np.errstate(over="ignore", invalid="ignore"):
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(np.float32)).astype(np.float16)
    raw = np.zeros(r4 * cols * 2, np.uint16)
    raw[q2h_index(np.arange(rows), cols, 0)] = hi.view(np.uint16)
    raw[q2h_index(np.arange(rows), cols, 1)] = lo.view(np.uint16)
    return raw


def split_law(hi, lo):
    """violations of (no plane inf / NaN, |lo| <= ulp_half(hi) / 2, hi is the nearest half of hi + lo -- on an exact tie either neighbour is a
    nearest one)"""
    fin = np.isfinite(hi) & np.isfinite(lo)
    with np.errstate(over="ignore", invalid="ignore"):
        ulp = np.spacing(np.abs(hi).astype(np.float16)).astype(np.float64)
        far = np.abs(lo) > 0.5 * ulp
        s = hi + lo
        near = s.astype(np.float16).astype(np.float64)
        # a tie: hi + lo lies exactly between hi and the half the conversion chose
        off = (near != hi) & ~(np.abs(s - hi) == np.abs(s - near))
    return int((~fin).sum()), int((far & fin).sum()), int((off & fin).sum())


def q2h_check(rep, name, k, hi, lo, ref, bound):
    """one decoded operand against its float64 replay: the fmt-3 link's arithmetic bound + 2^-22 |ref| (the RNE residual of an RNE half) +
    2^-29 (the half-subnormal grid of 16 x); and the split law"""
    law = split_law(hi, lo)
    if any(law):
        rep.failures.append((name, f"split law: {law[0]} non-finite, {law[1]} |lo| > ulp / 2, {law[2]} hi not nearest"))
    with np.errstate(invalid="ignore"):
        val = torch.from_numpy(np.nan_to_num((hi + lo) / 16.0, nan=np.inf, posinf=np.inf, neginf=np.inf))
    return add(rep, name, k, val, ref, bound + 2.0 ** -22 * ref.abs() + 2.0 ** -29)


# ---- Part C: the B planes by the rule of umx_weights.h and the four-product float64 reference ----------------------------------------------
def f16_scale(w32):
    """the power of two that puts max |w| into [2^14, 2^15)"""
    _, ex = np.frexp(np.float32(np.abs(w32).max()))          # max = f 2^ex, f in [0.5, 1)
    return float(2.0 ** int(np.clip(15 - int(ex), -24, 40)))


def b_planes(w32):
    """(s, [w0, w1, w2]): three RNE half planes of s w with exact residuals, as float64"""
    s = f16_scale(w32)
    x = np.asarray(w32, np.float32) * np.float32(s)
    planes = []
    for _ in range(3):
        h = x.astype(np.float16)
        planes.append(h.astype(np.float64))
        x = x - h.astype(np.float32)
    return s, planes


def _cmul(X, B, half):
    """X = (re, im) rows, B (2 half, K) = [Wa; Wb]: y_re = Xre Wa^T - Xim Wb^T, y_im = Xim Wa^T + Xre Wb^T -> [rows, 2 half] = [re | im]"""
    pr, pi = X[0] @ B.T, X[1] @ B.T
    return np.concatenate([pr[:, :half] - pi[:, half:], pi[:, :half] + pr[:, half:]], axis=1)


def _cabs(X, B, half):
    pr, pi = np.abs(X[0]) @ np.abs(B).T, np.abs(X[1]) @ np.abs(B).T
    return np.concatenate([pr[:, :half] + pi[:, half:], pi[:, :half] + pr[:, half:]], axis=1)


def gemm_ref(Ahi, Alo, w32, bias, half=0, cscale_mul=1.0):
    """The float64 sum of exactly the four plane products hh, hl, lh and A_hi . B_lo2, times 1 / (16 s), plus bias.  Ahi / Alo: the decoded
    planes in half units, un-negated; complex (half > 0): tuples (re, im).  Returns ref, sum |a| |b|, and the two single products (A_hi . B_lo2,
    A_lo . B_hi) with the same scale, for the projection statistic."""
    s, (b0, b1, b2) = b_planes(w32)
    cs = cscale_mul / (16.0 * s)
    if half:
        mul, ab = (lambda a, b: _cmul(a, b, half)), (lambda a, b: _cabs(a, b, half))
    else:
        mul, ab = (lambda a, b: a @ b.T), (lambda a, b: np.abs(a) @ np.abs(b).T)
    t_h2, t_lh = cs * mul(Ahi, b2), cs * mul(Alo, b0)
    ref = cs * mul(Ahi, b0 + b1) + t_lh + t_h2
    if bias is not None:
        ref = ref + np.asarray(bias, np.float64)[None, :]
    sab = abs(cs) * (ab(Ahi, b0) + ab(Ahi, b1) + ab(Ahi, b2) + ab(Alo, b0))
    return ref, sab, t_h2, t_lh


def gemm_bound(ref, sab, K, cplx):
    """(n_mfma + 2) 2u sum|a||b| + 2u |ref|: n_mfma = 4 K / 16 accumulating MFMAs (x 2: a complex output joins two accumulators), each allowed
    a truncating float32 accumulate (2u: NOTES.md section 5 documents a flooring adder); + 2 for the join and the un-scaling"""
    n = 4 * K // 16 * (2 if cplx else 1)
    return (n + 2) * 2 * U * sab + 2 * U * np.abs(ref)


def gemm_check(rep, lo2, name, out, Ahi, Alo, w32, bias, K, half=0):
    """one product: the per-element bound and the two gains.  A gain of A_hi . B_lo2 outside 1 +- 0.25 goes to the list `lo2`, which
    test_fp16_gemm_carries_a_hi_b_lo2 asserts empty.  Returns (ratio, gain of A_hi . B_lo2, gain of A_lo . B_hi)"""
    ref, sab, t_h2, t_lh = gemm_ref(Ahi, Alo, w32, bias, half)
    r = add(rep, name, 4 * K // 16 * (2 if half else 1) + 2, torch.from_numpy(out), torch.from_numpy(ref), torch.from_numpy(gemm_bound(ref, sab, K, bool(half))))
    g2, glh = projection_gain(out, ref - t_h2, t_h2), projection_gain(out, ref - t_lh, t_lh)
    if not abs(glh - 1.0) <= 0.25:
        rep.failures.append((name, f"gain of A_lo.B_hi = {glh:.4f}"))
    if not abs(g2 - 1.0) <= 0.25:
        lo2.append((name, f"gain of A_hi.B_lo2 = {g2:.4f}"))
    return r, g2, glh


# (name, complex half, A capture, A columns, (re, im) column offsets in A, K, weight suffix, bias suffix, output capture, its columns, (re, im) offsets, N)
def products(i):
    c1, c2 = f"blocks.{i}.edge_wise.so2_conv_1", f"blocks.{i}.edge_wise.so2_conv_2"
    return [("radial fc3", 0, "a2h", RH, (0, None), RH, f"{c1}.rad_func.fc3.weight", f"{c1}.rad_func.fc3.bias", "rad", RAD, (0, None), RAD),
            ("conv-1 m0", 0, "y1h", XROT, (0, None), 768, f"{c1}.fc_m0.weight", f"{c1}.fc_m0.bias", "hg", HG, (0, None), 640),
            ("conv-1 m1", 256, "y1h", XROT, (768, 1280), 512, f"{c1}.so2_m_conv.0.fc.weight", None, "hg", HG, (640, 896), 256),
            ("conv-1 m2", 128, "y1h", XROT, (1792, 2048), 256, f"{c1}.so2_m_conv.1.fc.weight", None, "hg", HG, (1152, 1280), 128),
            ("conv-2 m0", 0, "hidh", ROW, (0, None), 384, f"{c2}.fc_m0.weight", f"{c2}.fc_m0.bias", "msg", ROW, (0, None), 384),
            ("conv-2 m1", 256, "hidh", ROW, (384, 640), 256, f"{c2}.so2_m_conv.0.fc.weight", None, "msg", ROW, (384, 640), 256),
            ("conv-2 m2", 128, "hidh", ROW, (896, 1024), 128, f"{c2}.so2_m_conv.1.fc.weight", None, "msg", ROW, (896, 1024), 128)]


DEG_PRODUCT = ("radial fc3", 0, "a2h", RH, (0, None), RH, "edge_degree_embedding.rad_func.fc3.weight", "edge_degree_embedding.rad_func.fc3.bias",
               "rad", 3 * C, (0, None), 3 * C)


def tile_rows(ne, limit=12, seed=0):
    """every row, or (past `limit` tiles) whole 256-row tiles: the first, the last (partial) one and limit - 2 others, fixed seed"""
    nt = (ne + TILE - 1) // TILE
    if nt <= limit:
        return np.arange(ne)
    pick = np.sort(np.concatenate([[0, nt - 1], 1 + np.random.default_rng(seed).choice(nt - 2, limit - 2, replace=False)]))
    return np.concatenate([np.arange(t * TILE, min((t + 1) * TILE, ne)) for t in pick])


def product_operands(spec, raw16, out32, rows, ne, **dec):
    """(output [rows, N or 2 half], A_hi, A_lo) of one product on the rows `rows`"""
    _, half, _, acols, (ar, ai), K, _, _, _, ocols, (cr, ci), N = spec
    hi, lo = q2h_decode(raw16, rows, acols, **dec)
    o = out32.reshape(ne, ocols)[rows].astype(np.float64)
    if not half:
        return o[:, cr:cr + N], hi[:, ar:ar + K], lo[:, ar:ar + K]
    return (np.concatenate([o[:, cr:cr + N], o[:, ci:ci + N]], axis=1), (hi[:, ar:ar + K], hi[:, ai:ai + K]), (lo[:, ar:ar + K], lo[:, ai:ai + K]))


# ---- preconditions -----------------------------------------------------------------------------------------------------------------------
def element_facts(z, src, dst, p):
    """>= 3 elements; an element pair (a, b), a != b, that occurs as (Z_src, Z_dst) in both orders, with source and target embedding rows
    that differ for a and for b"""
    z = np.asarray(z)
    pairs = set(zip(z[src].tolist(), z[dst].tolist()))
    both = sorted((a, b) for a, b in pairs if a < b and (b, a) in pairs)
    assert len(set(z.tolist())) >= 3, sorted(set(z.tolist()))
    assert both, "no element pair in both orders"
    a, b = both[0]
    se, te = p["source_embedding.weight"], p["target_embedding.weight"]
    assert not torch.equal(se[a], te[a]) and not torch.equal(se[b], te[b]) and not torch.equal(se[a], se[b]) and not torch.equal(te[a], te[b])
    return dict(elements=sorted(set(z.tolist())), pair=(a, b))


EXPECT_NE = {"T1": 51, "S": 1142, "L": 44404}


# ---- one case ----------------------------------------------------------------------------------------------------------------------------
def radial_links(rep, muts, orc, tag, R, d, zs, zd, h1, h2, a_out, a_bound_extra=None):
    """A1, A2, A3 of one radial MLP on captured float64 copies; a_out = the operand, un-negated, float64.  muts: collects the mutation ratios
    (worst = smallest over the MLPs) and the centre gains"""
    x = gauss_exponent(d, None, orc.cutoff)
    k_exp = measure_k_exp(x)
    ref, bound = link_fc1(orc, R, d, zs, zd, k_exp)
    add(rep, f"{tag} A1 fc1 h1pre", 64 + k_exp, h1, ref, bound)
    low = lambda name, r: muts.__setitem__(name, min(muts.get(name, np.inf), r))     # noqa: E731
    low("ts / tt swapped", ratio(h1, link_fc1(orc, R, d, zd, zs, k_exp)[0], bound)[0])
    low("fc1 bias omitted", ratio(h1, link_fc1(orc, R, d, zs, zd, k_exp, bias=False)[0], bound)[0])
    # float32 centres move a gaussian by 2 coeff (d - mu) dmu <= 2.5e-6 relative where |x_k| is small -- inside gamma_64 = 3.8e-6, so the
    # per-element bound cannot see them.  The projection statistic can: over the edges with a centre within half a spacing (|x_k| small for
    # the leading gaussians: every edge) the gain of (reference with float32 centres - reference) in the output is 0 for double centres, 1 for
    # float32 ones.  Asserted |gain| <= 0.25 on the engine's output: that assertion is the protection.  The mutation figure below builds the
    # reference itself from float32 centres; against an engine with double centres it reads 1 / 0.25 = 4 by the algebra of the statistic and
    # shows no more than that the assertion above would then fire.
    mu32 = gauss_centres(orc.cutoff).to(torch.float32).to(T64)
    ref32 = link_fc1(orc, R, d, zs, zd, k_exp, mu=mu32)[0]
    g = projection_gain(h1, ref, ref32 - ref)
    if not abs(g) <= 0.25:
        rep.failures.append((f"{tag} A1", f"gain of float32 centres = {g:.4f}"))
    muts.setdefault("centre gains", []).append(g)
    low("float32 centres (gain, |.| > 0.25 rejects)", abs(projection_gain(h1, ref32, ref - ref32)) / 0.25)
    # A2
    kh1 = silu_k_host(ln_silu(h1, R.ln1w, R.ln1b, 0.0, 0.0)[2])
    ref, bound, _ = link_fc2(R, h1, kh1)
    add(rep, f"{tag} A2 fc2 h2pre", 128 + 2 * kh1, h2, ref, bound)
    low("fc2 bias last, wrong sign", ratio(h2, link_fc2(R, h1, kh1, bias_last_sign=-1.0)[0], bound)[0])
    # LN1's eps: fc1's rows have a variance of 10 ... 100, so eps / (2 var) ~ 1e-7 of the normalised row lies inside the bound of this link
    # (reported as info).  The projection statistic sees it: the gain of (reference without eps - reference) in h2pre is 0 for a head that
    # adds eps and 1 for one that does not.  Asserted |gain| <= 0.25 on the engine's output.
    ref0 = link_fc2(R, h1, kh1, eps=0.0)[0]
    low("info: LN1 eps omitted", ratio(h2, ref0, bound)[0])
    g = projection_gain(h2, ref, ref0 - ref)
    if not abs(g) <= 0.25:
        rep.failures.append((f"{tag} A2", f"gain of an LN1 without eps = {g:.4f}"))
    muts.setdefault("LN1 eps gains", []).append(g)
    muts["info: smallest var(h1pre)"] = min(muts.get("info: smallest var(h1pre)", np.inf), float(h1.var(-1, unbiased=False).min()))
    # A3
    kh2 = silu_k_host(ln_silu(h2, R.ln2w, R.ln2b, 0.0, 0.0)[2])
    ref, bound, _ = link_a2(R, h2, kh2)
    if a_bound_extra is not None:
        bound = bound + a_bound_extra(ref)
    add(rep, f"{tag} A3 operand", 1 + 2 * kh2, a_out, ref, bound)
    low("LN eps omitted", ratio(a_out, link_a2(R, h2, kh2, eps=0.0)[0], bound)[0])
    return k_exp, max(kh1, kh2), ref, bound


def capture_names(mode, size):
    tags = ["deg"] + [str(i) for i in LAYERS[size]]
    names = ["row_ptr", "src", "dst", "out_ptr", "out_edge", "evec", "frame"]
    per = ["h1pre", "h2pre", MODES[mode]] + (["rad", "xn", "hg", "msg", "y1h", "hidh"] if mode == "split" else [])
    return names + [f"{n}.{t}" for n in per for t in tags]


def replay_case(mode, size, get, z, orc, w):
    """every link of one evaluation; returns (Report, asserted mutation ratios, gains of A_hi . B_lo2 outside 1 +- 0.25)"""
    tag0 = f"{mode} {size}"
    rep, muts, lo2 = Report(tag0), {}, []
    nn = SIZES[size][0]
    G = Graph(get, nn)
    ne, ne4 = G.ne, (G.ne + 3) // 4 * 4
    assert ne == EXPECT_NE[size] and int(G.row_ptr[-1]) == ne, ne
    if size == "T1":
        assert ne % 2 == 1 and ne < 64 and ne % 4 != 0
    if size == "S":
        assert ne % 64 == 54
    if size == "L":
        assert (ne + 63) // 64 > 512
    facts = element_facts(z, G.src.numpy(), G.dst.numpy(), orc.p)
    print(f"  [{tag0}] ne {ne}, {(ne + 63) // 64} tiles of 64, elements {facts['elements']}, pair in both orders {facts['pair']}")
    zt = torch.as_tensor(np.asarray(z), dtype=torch.long)
    zs, zd = zt[G.src], zt[G.dst]
    d = _t(G.evec[:, 3])
    sign = np.where(np.arange(ne) % 2 == 1, -1.0, 1.0)[:, None]
    all_rows = np.arange(ne)
    kexp = khmax = 0.0
    a2raw = {}
    for t in ["deg"] + [str(i) for i in LAYERS[size]]:
        R = Radial(orc.p, rad_prefix(t))
        h1, h2 = _t(get(f"h1pre.{t}").reshape(ne, RH)), _t(get(f"h2pre.{t}").reshape(ne, RH))
        extra = None
        if mode == "bf16x3":
            raw = _unblock(get(f"a2q.{t}"), RH)
            assert raw.shape[0] == ne4
            a_out, a_nosign = _t(raw[:ne].astype(np.float64) * sign), _t(raw[:ne])
        elif mode == "fp32":
            a_out = a_nosign = _t(get(f"a2.{t}").reshape(ne, RH))
        else:
            raw16 = a2raw[t] = get(f"a2h.{t}", np.uint16)
            assert raw16.size == ne4 * RH * 2
            hi, lo = q2h_decode(raw16, all_rows, RH)
            a_out = _t((hi + lo) / 16.0)
            a_nosign = _t(a_out.numpy() * sign)
            extra = lambda ref: 2.0 ** -22 * ref.abs() + 2.0 ** -29          # noqa: E731  (the plane term of Part B)
        ke, kh, ref, bound = radial_links(rep, muts, orc, t, R, d, zs, zd, h1, h2, a_out, extra)
        kexp, khmax = max(kexp, ke), max(khmax, kh)
        if mode != "fp32":
            muts["row sign not applied"] = min(muts.get("row sign not applied", np.inf), ratio(a_nosign, ref, bound)[0])
        if mode == "split":
            law = split_law(hi, lo)
            if any(law):
                rep.failures.append((f"a2h.{t}", f"split law {law}"))
            s_hi, s_lo = q2h_decode(raw16, all_rows, RH, swap=True)
            muts["hi and lo planes swapped (split law violations)"] = min(muts.get("hi and lo planes swapped (split law violations)", np.inf), float(sum(split_law(s_hi, s_lo))))
            o_hi, o_lo = q2h_decode(raw16, all_rows, RH, plane_bytes=16)
            muts["plane offset q 32 read as q 16"] = min(muts.get("plane offset q 32 read as q 16", np.inf), ratio(_t((o_hi + o_lo) / 16.0), ref, bound)[0])
    print(f"  [{tag0}] k_exp {kexp:.2f} u of the gaussian, k_host of SiLU on the LayerNorm outputs {khmax:.2f} u; centre gains "
          + " ".join(f"{g:+.4f}" for g in muts.pop("centre gains")) + "; gains of an LN1 without eps " + " ".join(f"{g:+.4f}" for g in muts.pop("LN1 eps gains")))
    gains = []
    if mode == "split":
        # ---- Part B: y1h and hidh against the float64 replays of the fmt-3 links
        for i in LAYERS[size]:
            xn = _t(get(f"xn.{i}")).reshape(nn, 9, C)
            rad32, hg32 = get(f"rad.{i}").reshape(ne, RAD), get(f"hg.{i}").reshape(ne, HG)
            y1raw, hidraw = get(f"y1h.{i}", np.uint16), get(f"hidh.{i}", np.uint16)
            assert y1raw.size == ne4 * XROT * 2 and hidraw.size == ne4 * ROW * 2
            kh = host_ulps(hg32)
            for sl in G.slices():
                rows = np.arange(sl.start, sl.stop)
                xcat = torch.cat([xn[G.src[sl]], xn[G.dst[sl]]], dim=2)
                ref, bound = EL.link_rotmod(G.wig(sl), xcat, _t(rad32[sl]))
                hi, lo = q2h_decode(y1raw, rows, XROT)
                q2h_check(rep, f"L{i} B y1h", 7, hi, lo, ref.reshape(-1, XROT), bound.reshape(-1, XROT))
                ref, bound, k0, k1 = EL.link_gate_fwd(_t(hg32[sl]), kh)
                hi, lo = q2h_decode(hidraw, rows, ROW)
                q2h_check(rep, f"L{i} B hidh", max(k0, k1), hi, lo, ref.reshape(-1, ROW), bound.reshape(-1, ROW))
            # ---- Part C
            rows = tile_rows(ne)
            assert rows[0] == 0 and rows[-1] == ne - 1 and (len(rows) == ne or len(rows) >= 10 * TILE)
            raws, outs = {"a2h": a2raw[str(i)], "y1h": y1raw, "hidh": hidraw}, {"rad": rad32, "hg": hg32, "msg": get(f"msg.{i}")}
            for spec in products(i):
                name, half, acap, _, _, K, wn, bn, ocap, _, _, _ = spec
                out, Ahi, Alo = product_operands(spec, raws[acap], outs[ocap], rows, ne)
                w32, bias = np.asarray(w[wn], np.float32), (None if bn is None else np.asarray(w[bn], np.float32))
                r, g2, glh = gemm_check(rep, lo2, f"L{i} C {name}", out, Ahi, Alo, w32, bias, K, half)
                gains.append((f"L{i} {name}", r, g2, glh))
                if i == LAYERS[size][0]:
                    ref, sab, t_h2, t_lh = gemm_ref(Ahi, Alo, w32, bias, half)
                    bnd = torch.from_numpy(gemm_bound(ref, sab, K, bool(half)))
                    o = torch.from_numpy(out)
                    low = lambda nm, v: muts.__setitem__(nm, min(muts.get(nm, np.inf), v))     # noqa: E731
                    low("cscale off by 2", ratio(o, torch.from_numpy(gemm_ref(Ahi, Alo, w32, bias, half, cscale_mul=2.0)[0]), bnd)[0])
                    low("A_lo.B_hi dropped from the GEMM reference", ratio(o, torch.from_numpy(ref - t_lh), bnd)[0])
                    if acap == "y1h" and not half:
                        s_out, s_hi, s_lo = product_operands(spec, raws[acap], outs[ocap], rows, ne, swap=True)
                        low("hi and lo planes swapped (GEMM)", ratio(o, torch.from_numpy(gemm_ref(s_hi, s_lo, w32, bias, half)[0]), bnd)[0])
        rows = tile_rows(ne)
        out, Ahi, Alo = product_operands(DEG_PRODUCT, a2raw["deg"], get("rad.deg"), rows, ne)
        r, g2, glh = gemm_check(rep, lo2, "deg C radial fc3", out, Ahi, Alo, np.asarray(w[DEG_PRODUCT[6]], np.float32), np.asarray(w[DEG_PRODUCT[7]], np.float32), RH)
        gains.append(("deg radial fc3", r, g2, glh))
        for name, r, g2, glh in gains:
            print(f"  [{tag0}] C {name:22s} max |err| / bound {r:.3e}  gain A_hi.B_lo2 {g2:.4f}  gain A_lo.B_hi {glh:.6f}")
    rep.close()
    for name, r in muts.items():
        print(f"  [{tag0}] mutation {name}: {r:.3g}" + ("" if name.startswith("info:") else " x the bound"))
    return rep, asserted(muts), lo2


_CASES = {}


def _case(mode, size, monkeypatch):
    """one evaluation and its replay, shared by the tests below"""
    if (mode, size) in _CASES:
        return _CASES[(mode, size)]
    from pdb2reaction_amd import synth, weights as Wt
    from pdb2reaction_amd.engine import Engine

    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    n_atoms, max_neigh = SIZES[size]
    w = Wt.make_synthetic_weights(0)
    z, pos = synth.make_cluster(n_atoms)
    orc = O.Oracle(w)
    monkeypatch.setenv("UMX_DEBUG_ONLY", ",".join(capture_names(mode, size)))
    eng = Engine(0, precision=mode)
    try:
        eng.load_weights(w)
        eng.set_system(z, max_neigh=max_neigh)
        eng.debug_keep(True)
        e, _ = eng.energy_forces(pos.astype(np.float32), forces=False)
        assert np.all(np.isfinite(e))
        assert GL.keys(eng, fwd=True) == GL.KEYS_FORWARD_LINKS[(mode, size)], sorted(GL.keys(eng))      # the table rows this case holds (the ledger)
        print()
        _CASES[(mode, size)] = replay_case(mode, size, lambda name, dtype=np.float32: eng.debug_fetch(name, dtype), z, orc, w)
    finally:
        eng.close()
    return _CASES[(mode, size)]


@pytest.mark.parametrize("size", ["T1", "S", "L"])
@pytest.mark.parametrize("mode", ["bf16x3", "fp32", "split"])
def test_forward_links_against_float64(mode, size, monkeypatch):
    """Every link of Parts A, B and C, the gain of A_lo . B_hi and the mutations.  Measured on the MI355X (profiles/forward_links.txt; largest
    |err| / bound over T1, S, L and their radial MLPs / layers; the nine cases take 60 s):
    * k_exp (numpy float32 exp against float64 on the rounded exponents) <= 3.3 u; k_host of SiLU on the LayerNorm outputs <= 3.7 u
    * A1 h1pre 0.45 (k = 64 + k_exp), A2 h2pre 0.047 (k = 128 + ...: the worst case of a 128-term chain is far off), A3 operand 0.37 in all
      three modes; the gain of float32 gaussian centres in h1pre: |g| <= 0.018 at 51 edges, <= 0.004 at 1142, <= 0.0007 at 44404
    * B y1h 0.9995, hidh 0.9988: elements below 2^-18 sit on the half-subnormal grid, where the 2^-29 term IS the error; split law: no violation
    * C per element: radial fc3 0.046, conv-1 m0 / m1 / m2 0.019 / 0.006 / 0.010, conv-2 m0 / m1 / m2 0.016 / 0.006 / 0.012;
      gain of A_lo . B_hi 1 +- 2e-5 everywhere
    * mutations (smallest over the sizes, in units of the bound): ts / tt 5.7e6, fc1 bias 4.4e5, float32 centres 3.97 (gain / 0.25: 4 by the
      algebra of the statistic, see radial_links), fc2 bias 1.5e4, LN eps (LN2, A3) 9.3, row sign 2.7e6, planes swapped 1.3e4 law violations
      and 4.2 (GEMM), q 16 offset 6.6e6, cscale 8.4e3, A_lo . B_hi dropped 2.2.  LN1's eps moves h2pre by 0.35 ... 0.44 of the A2 bound
      (eps / 2 var on rows of variance >= 0.49): it is asserted through its projection gain, |g| <= 0.0013 measured against the 0.25 allowed."""
    rep, muts, _ = _case(mode, size, monkeypatch)
    assert not rep.failures, rep.failures
    want = 5 if mode == "fp32" else 6          # Part A (+ the row sign where rows are negated); split: + the decoder and GEMM mutations
    if mode == "split":
        want += 5
    assert len(muts) == want and all(r > 1.0 for r in muts.values()), muts


@pytest.mark.parametrize("size", ["T1", "S", "L"])
def test_fp16_gemm_carries_a_hi_b_lo2(size, monkeypatch):
    """|gain of A_hi . B_lo2 - 1| <= 0.25 for every product of the fp16 forward GEMM.

    Measured on the MI355X (profiles/forward_links.txt): 0.91 ... 1.04 over every product, layer and size (radial fc3 0.98 ... 1.01, conv-1 m0
    0.91 ... 1.02, m1 0.93 ... 1.03, m2 1.00 ... 1.04, conv-2 m0 / m1 / m2 0.98 ... 1.04).  A kernel without the product reads 0.

    This test found a fault that the per-element bound cannot see (the term is 2^-24 of the leading product, the bound held with a margin of
    16 ... 200).  With all four products added into the running accumulator the gain read 0.43 ... 0.81 at every size: v_mfma_f32_32x32x16_f16
    aligns its 16 products to the largest addend -- the accumulator, which carries all earlier k-tiles and the bias -- and cuts them towards
    zero a few bits below its ulp (csrc/mfma_bias.hip, profiles/r04_mfma_adder_rounding.txt, f16 rows), so most of each such product was
    lost.  The product alone in a zero accumulator, added once per k-step, read 0.45 ... 0.80: smaller than half an ulp of a value on the
    float32 grid, it rounds away.  The kernel (umx_gemm_q.h) now sums the three small products of a k-step apart and folds them in with one
    float32 add; the 2^-11-order products beside it make that rounding unbiased for the sub-ulp term."""
    _, _, lo2 = _case("split", size, monkeypatch)
    assert not lo2, lo2
