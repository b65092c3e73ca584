"""The checker of tests/test_gpu_forward_links.py, exercised without a GPU: numpy-float32 and rounded-once restatements of the three radial
links pass it and its mutations are rejected; the Q2H decoder round-trips an encoder written with numpy.float16 (subnormal and near-overflow
values included); the B-plane rebuild is exact; the gain statistic reads 1 and 0; the checker's formulas are the oracle's."""
import os
import sys

import numpy as np
import torch

from oracle import escn_md_oracle as O
from oracle import tables as OT
from pdb2reaction_amd import weights as Wt

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
import test_gpu_forward_links as FL  # noqa: E402
from test_gpu_edge_links import T64, U, Report, _t, ratio  # noqa: E402

RH, NG = FL.RH, FL.NG
F32 = np.float32


def _setup(ne=203, seed=5):
    w = Wt.make_synthetic_weights(0)
    orc = O.Oracle(w)
    rng = np.random.default_rng(seed)
    d32 = rng.uniform(0.7, 5.99, ne).astype(F32)
    zs, zd = (torch.from_numpy(rng.choice([1, 6, 8], ne)) for _ in range(2))
    return w, orc, d32, zs, zd


def _fma_chain(a32, w32, start32):
    """acc = fma(a_k, w_k, acc) over k, float32: the product of two float32 is exact in double, the sum is rounded to double and then to
    float32 (a double rounding differs from a true fma in ~2^-29 of the cases, by one ulp: inside every bound here)"""
    acc = np.broadcast_to(start32, (a32.shape[0], w32.shape[0])).astype(F32)
    for k in range(a32.shape[1]):
        acc = (acc.astype(np.float64) + a32[:, k:k + 1].astype(np.float64) * w32[None, :, k].astype(np.float64)).astype(F32)
    return acc


def _ln_silu32(hi, lo, w, b):
    mu = F32((hi.sum(1, dtype=F32) + lo.sum(1, dtype=F32)) * F32(1 / 128))[:, None]
    v = ((hi.astype(np.float64) - mu) + lo).astype(F32)
    var = (v * v).sum(1, dtype=F32)[:, None] * F32(1 / 128)
    y = v * (F32(1) / np.sqrt(var + F32(OT.LN_EPS))) * w + b
    return (y * (F32(1) / (F32(1) + np.exp(-y)))).astype(F32)


def _float32_head(w, orc, prefix, d32, zs, zd):
    """the radial head restated in numpy float32 from the oracle's formulas: (h1pre, h2pre, a2)"""
    g = lambda n: np.asarray(w[f"{prefix}.{n}"], F32)     # noqa: E731
    W1 = g("fc1.weight")
    x32 = FL.gauss_exponent(_t(d32)).numpy().astype(F32)
    s = _fma_chain(np.exp(x32), W1[:, :NG], F32(0))
    se, te = np.asarray(w["source_embedding.weight"], np.float64), np.asarray(w["target_embedding.weight"], np.float64)
    tab = se[zs.numpy()] @ W1[:, NG:NG + 128].astype(np.float64).T + te[zd.numpy()] @ W1[:, NG + 128:].astype(np.float64).T + g("fc1.bias")
    h1_64 = s.astype(np.float64) + tab
    h1 = h1_64.astype(F32)
    a1 = _ln_silu32(h1, h1_64 - h1, g("ln1.weight"), g("ln1.bias"))
    h2 = _fma_chain(a1, g("fc2.weight"), g("fc2.bias")[None, :])
    return h1, h2, _ln_silu32(h2, np.zeros_like(h2, np.float64), g("ln2.weight"), g("ln2.bias"))


def test_radial_links_pass_on_float32_restatements_and_reject_mutations():
    w, orc, d32, zs, zd = _setup()
    d = _t(d32)
    for tag in ("deg", "0", "3"):
        R = FL.Radial(orc.p, FL.rad_prefix(tag))
        h1, h2, a2 = _float32_head(w, orc, FL.rad_prefix(tag), d32, zs, zd)
        for what in ("float32", "rounded once"):
            o1, o2, o3 = _t(h1), _t(h2), _t(a2)
            rep, muts = Report(f"cpu {what} {tag}"), {}
            if what == "rounded once":          # every link's float64 reference from the float32 restatement's input, rounded to float32 once
                k = FL.measure_k_exp(FL.gauss_exponent(d))
                o1 = FL.link_fc1(orc, R, d, zs, zd, k)[0].to(torch.float32).to(T64)
                o2 = FL.link_fc2(R, o1, 0.0)[0].to(torch.float32).to(T64)
                o3 = FL.link_a2(R, o2, 0.0)[0].to(torch.float32).to(T64)
            k_exp, kh, ref, bound = FL.radial_links(rep, muts, orc, tag, R, d, zs, zd, o1, o2, o3)
            gains = muts.pop("centre gains") + muts.pop("LN1 eps gains")
            rep.close()
            assert not rep.failures, rep.failures
            assert all(r < 1.0 for r, _, _ in rep.rows.values()), rep.rows
            assert 0.4 < k_exp < 4.0 and kh < 8.0, (k_exp, kh)
            muts = FL.asserted(muts)
            assert len(muts) == 5 and all(r > 1.0 for r in muts.values()), muts
            assert all(abs(g) < 0.25 for g in gains), gains
            if what == "rounded once":          # a head whose first LayerNorm adds no eps: the gain the checker asserts reads 1, not 0
                r_eps, r_0 = FL.link_fc2(R, o1, 0.0)[0], FL.link_fc2(R, o1, 0.0, eps=0.0)[0]
                assert abs(FL.projection_gain(r_0.to(torch.float32).to(T64), r_eps, r_0 - r_eps) - 1.0) < 0.25
            # the row sign: an operand whose odd rows stay negated is rejected
            sg = _t(np.where(np.arange(len(d32)) % 2 == 1, -1.0, 1.0)[:, None])
            assert ratio(o3 * sg, ref, bound)[0] > 1.0


def test_checker_formulas_are_the_oracles():
    w, orc, d32, zs, zd = _setup(64)
    d = _t(d32)
    xe = orc.edge_scalars(d, zs, zd)
    assert torch.equal(torch.exp(FL.gauss_exponent(d)), xe[:, :NG])
    assert torch.equal(FL.gauss_centres(), torch.linspace(0.0, OT.CUTOFF, OT.NUM_DISTANCE_BASIS, dtype=torch.float64))
    for tag in ("deg", "1"):
        pre = FL.rad_prefix(tag)
        R = FL.Radial(orc.p, pre)
        h1 = FL.link_fc1(orc, R, d, zs, zd, 1.0)[0]
        assert torch.equal(h1, xe @ orc.p[f"{pre}.fc1.weight"].T + orc.p[f"{pre}.fc1.bias"])
        _, _, xh = FL.ln_parts(h1)
        assert torch.allclose(xh * R.ln1w + R.ln1b, O.layer_norm(h1, R.ln1w, R.ln1b), rtol=0, atol=1e-14)
        a, _, y = FL.ln_silu(h1, R.ln1w, R.ln1b, 0.0, 1.0)
        assert torch.equal(a, O.silu(y))
        h2 = FL.link_fc2(R, h1, 1.0)[0]
        a2 = FL.link_a2(R, h2, 1.0)[0]
        # the three links chained are the oracle's radial_mlp
        rad = a2 @ R.W3.T + R.b3
        assert torch.allclose(rad, O.radial_mlp(orc.p, pre, xe), rtol=0, atol=1e-12 * float(rad.abs().max()))
    # the Jacobian the propagation bounds term by term is layer_norm's: against autograd on one row
    h = torch.randn(1, RH, dtype=T64, generator=torch.Generator().manual_seed(1)) * 0.7 + 0.2
    J = torch.autograd.functional.jacobian(lambda t: O.layer_norm(t, torch.ones(RH, dtype=T64), torch.zeros(RH, dtype=T64)), h)[0, :, 0, :]
    _, rstd, xh = FL.ln_parts(h)
    mine = rstd[0] * (torch.eye(RH, dtype=T64) - 1.0 / RH - xh[0][:, None] * xh[0][None, :] / RH)
    assert torch.allclose(J, mine, rtol=0, atol=1e-13)


def test_q2h_round_trip_and_split_law():
    rng = np.random.default_rng(3)
    rows, cols = 51, 128
    x = (rng.standard_normal((rows, cols)) * np.exp(rng.uniform(-14, 3, (rows, cols)))).astype(F32)
    x[0, :8] = [0.0, 2.0 ** -29, -2.0 ** -28, 3 * 2.0 ** -29, 2.0 ** -18, 2.0 ** -18 * (1 + 2.0 ** -11), 4093.0, -4093.9]     # subnormal halves of 16 x ... just below 65520 / 16
    x[1, :4] = [2.0 ** -17 * (1 + 3 * 2.0 ** -10) + 2.0 ** -29 * 0.75, 2.0 ** -16, -2.0 ** -30, 4094.9]
    raw = FL.q2h_encode(x)
    assert raw.size == 52 * cols * 2
    hi, lo = FL.q2h_decode(raw, np.arange(rows), cols)
    sg = np.where(np.arange(rows) % 2 == 1, F32(-1), F32(1))[:, None]
    xs = F32(16) * x
    h16 = xs.astype(np.float16)
    l16 = ((xs * sg) - (xs * sg).astype(np.float16).astype(F32)).astype(np.float16)
    assert np.array_equal(hi, h16.astype(np.float64)) and np.array_equal(lo, l16.astype(np.float64) * sg)
    assert FL.split_law(hi, lo) == (0, 0, 0)
    err = np.abs((hi + lo) / 16.0 - x.astype(np.float64))
    assert np.all(err <= 2.0 ** -22 * np.abs(x) + 2.0 ** -29)
    # one element by the layout rule, by hand: row 6, column 37, plane 1 of a 128-wide matrix
    byte = ((6 // 4) * (128 // 16) + 37 // 16) * 256 + (6 % 4) * 64 + 1 * 32 + (37 % 16) * 2
    assert FL.q2h_index([6], 128, 1)[0, 37] * 2 == byte
    # out of range: |x| >= 65520 / 16 turns into inf: the law reports it
    big = x.copy()
    big[2, 5] = 4095.0
    assert FL.split_law(*FL.q2h_decode(FL.q2h_encode(big), np.arange(rows), cols))[0] >= 1
    # the decoder mutations are rejected
    s_hi, s_lo = FL.q2h_decode(raw, np.arange(rows), cols, swap=True)
    assert sum(FL.split_law(s_hi, s_lo)) > 0
    o_hi, o_lo = FL.q2h_decode(raw, np.arange(rows), cols, plane_bytes=16)
    ref = _t(x.astype(np.float64))
    assert ratio(_t((o_hi + o_lo) / 16.0), ref, 2.0 ** -22 * ref.abs() + 2.0 ** -29)[0] > 1.0
    u_hi, u_lo = FL.q2h_decode(raw, np.arange(rows), cols, signed=False)
    assert ratio(_t((u_hi + u_lo) / 16.0), ref, 2.0 ** -22 * ref.abs() + 2.0 ** -29)[0] > 1.0


def test_b_planes_are_exact_for_the_synthetic_weights():
    w = Wt.make_synthetic_weights(0)
    names = [FL.DEG_PRODUCT[6]] + [s[6] for i in range(OT.NUM_LAYERS) for s in FL.products(i)]
    assert len(names) == 1 + 7 * OT.NUM_LAYERS
    for n in names:
        w32 = np.asarray(w[n], F32)
        s, (b0, b1, b2) = FL.b_planes(w32)
        mx = float(np.abs(w32).max()) * s
        assert 2.0 ** 14 <= mx < 2.0 ** 15 and np.log2(s) == int(np.log2(s)), (n, mx)
        # exact wherever float32's last bit of s w is on the half-subnormal grid 2^-24 (|s w| >= 1/2, i.e. |w| >= 2^-16 max|w|: umx_weights.h
        # pack_f16); below, the third plane rounds to that grid: an absolute 2^-25
        sw = w32.astype(np.float64) * s
        res = np.abs(b0 + b1 + b2 - sw)
        big = np.abs(sw) >= 0.5
        assert big.mean() > 0.999 and not res[big].any() and np.all(res <= 2.0 ** -25), (n, big.mean(), res.max())
        assert np.all(np.isfinite(b0)) and np.all(np.abs(b1) <= 0.5 * np.spacing(np.abs(b0).astype(np.float16)).astype(np.float64))


def test_gemm_checker_gains_and_mutations_on_a_model_gemm():
    rng = np.random.default_rng(11)
    rows = 70
    for half, K, N in ((0, 128, 96), (64, 96, 64)):
        w32 = (rng.standard_normal((2 * half if half else N, K)) * 0.05).astype(F32)
        bias = None if half else rng.standard_normal(N).astype(F32)
        x = rng.standard_normal((rows, 2 * K)).astype(F32)
        hi, lo = FL.q2h_decode(FL.q2h_encode(x), np.arange(rows), 2 * K)
        A = ((hi[:, :K], hi[:, K:]), (lo[:, :K], lo[:, K:])) if half else (hi[:, :K], lo[:, :K])
        ref, sab, t_h2, t_lh = FL.gemm_ref(A[0], A[1], w32, bias, half)
        assert ref.shape == (rows, 2 * half if half else N)
        # the four-product sum is the product with the exact weight up to the dropped A_lo . (B_mid + B_lo2): 2^-22 relative
        s, planes = FL.b_planes(w32)
        xq = (hi + lo) / 16.0
        exact = (FL._cmul((xq[:, :K], xq[:, K:]), w32.astype(np.float64), half) if half else xq[:, :K] @ w32.astype(np.float64).T + bias)
        assert np.all(np.abs(ref - exact) <= 2.0 ** -21 * sab)
        assert abs(FL.projection_gain(ref, ref - t_h2, t_h2) - 1.0) < 1e-9 and abs(FL.projection_gain(ref - t_h2, ref - t_h2, t_h2)) < 1e-9
        assert abs(FL.projection_gain(ref, ref - t_lh, t_lh) - 1.0) < 1e-9 and abs(FL.projection_gain(ref - t_lh, ref - t_lh, t_lh)) < 1e-9
        # a float32 image of the reference passes the checker, its mutations do not
        rep = Report("cpu gemm")
        lo2 = []
        r, g2, glh = FL.gemm_check(rep, lo2, "model", ref.astype(F32).astype(np.float64), A[0], A[1], w32, bias, K, half)
        assert not rep.failures and r < 1.0 and abs(glh - 1.0) < 0.01 and abs(g2 - 1.0) < 0.25 and not lo2, (r, g2, glh, rep.failures)
        bnd = _t(FL.gemm_bound(ref, sab, K, bool(half)))
        assert ratio(_t(ref.astype(F32)), _t(FL.gemm_ref(A[0], A[1], w32, bias, half, cscale_mul=2.0)[0]), bnd)[0] > 1.0
        assert ratio(_t(ref.astype(F32)), _t(ref - t_lh), bnd)[0] > 1.0
        rep = Report("cpu gemm without A_lo.B_hi")
        FL.gemm_check(rep, [], "model", (ref - t_lh).astype(F32).astype(np.float64), A[0], A[1], w32, bias, K, half)
        assert rep.failures
        # a kernel without A_hi . B_lo2 stays inside the per-element bound (a 2^-22 term) -- only its gain shows it
        rep = Report("cpu gemm without A_hi.B_lo2")
        r, g2, _ = FL.gemm_check(rep, lo2, "model", ref - t_h2, A[0], A[1], w32, bias, K, half)
        assert r < 1.0 and abs(g2) < 1e-9 and not rep.failures and lo2


def test_tile_rows_keeps_first_and_last_tile():
    assert np.array_equal(FL.tile_rows(1142), np.arange(1142))
    r = FL.tile_rows(44404)
    assert r[0] == 0 and r[-1] == 44403 and len(r) == 11 * 256 + 44404 % 256 and len(np.unique(r)) == len(r)
    assert np.array_equal(r, FL.tile_rows(44404))
