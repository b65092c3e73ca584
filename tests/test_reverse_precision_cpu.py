"""CPU calibration of the precision statistic that tests/test_gpu_reverse_links.py holds the engine's reverse GEMMs to (no GPU).

The statistic of one GEMM C = A . B^T against its float64 value C64 is

    stat = RMS over the output elements of  (C - C64) / sqrt(sum_k (a_k b_k)^2)

-- the error in units of the root-sum-square of the products, which is what rounding each product (or each partial sum) to p bits makes of
order 2^-p whatever the signs or the cancellation of the sum.  `t24(K)` separates "every product carries >= 24 significant bits" (bf16x3:
six bf16 plane products; the fp32 mode) from "16-bit products" (split-bf16: three plane products).  With 24-bit products what is left is the
float32 rounding of the running sums, which grows like sqrt(K) in these units (measured 0.25 * 2^-24 * sqrt(K) for K = 128 ... 1536, the
float32 sequential sum 0.30); 16-bit products give 4.3e-6 - 4.6e-6 at every K.  So T24 = 0.6 * 2^-24 * sqrt(K): at the conv GEMMs' K (<= 640)
the three-product statistic is >= 4 T24, at fc3^T's K = 1536 it is 3.8 T24.  Set here, on the bit-exact model of the matrix core
(tools/mfma_emul.c), from random operands with each reverse GEMM's K, the odd-rows-negated storage of the engine and SiLU-derivative-like
columns; the GPU test imports it.

The gross-error bound `kappa(mode, K)` is a worst case per element, |C - C64| <= kappa * sum_k |a_k| |b_k|: the dropped plane products plus
one float32 rounding per accumulation step.  It is loose on purpose; it catches what is wrong by a lot (a wrong row, offset or conj sign).
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mfma_model as MM  # noqa: E402

U = 2.0 ** -24


def t24(K: int) -> float:
    """The 24-bit threshold of the precision statistic for a GEMM of depth K (module docstring)."""
    return 0.6 * U * np.sqrt(K)


# the three-product (two-plane) form of the engine's split-bf16 reverse GEMMs on the model: a0.b0, a0.b1, a1.b0 (umx_gemm_pl.h, P = 2)
TWO_PLANE = dict(prog=[(0, 1, 0), (1, 0, 0), (0, 0, 0)], fold_step=[], fold_end=[])
# K of the reverse GEMMs: conv-2^T m0 / m1 / m2, conv-1^T m0 / m1 / m2 (per complex half), radial fc3^T
REVERSE_K = (384, 256, 128, 640, 256, 128, 1536)


def kappa(mode: str, K: int) -> float:
    """Per-element worst-case bound in units of sum_k |a_k b_k| (see the module docstring)."""
    if mode == "fp32":                       # float32 FMAs, one rounding per k (any order) + the float32 operands' own rounding
        return (K + 8) * U
    if mode == "bf16x3":                     # 6 plane products per 16-k MFMA, each with a rounded pass sum; 3 dropped products < 3 * 2^-24
        return (6 * K / 8 + 8) * U
    if mode == "split-bf16":                 # two planes: a - a0 - a1 < 2^-17 |a|; a1.b1 dropped (2^-18); 3 products per 16-k MFMA
        return 2.0 ** -15 + (3 * K / 8 + 8) * U
    raise ValueError(mode)


def link_stats(c, c64, abs_sum, sq_sum):
    """(max over elements of |C - C64| / sum|a b|, RMS of (C - C64) / sqrt(sum (a b)^2)); elements with no nonzero product must be exactly 0."""
    d = np.abs(np.asarray(c, np.float64) - c64)
    live = abs_sum > 0
    assert not d[~live].any(), "nonzero output where every product is zero"
    gross = float((d[live] / abs_sum[live]).max()) if live.any() else 0.0
    stat = float(np.sqrt(np.mean((d[live] / np.sqrt(sq_sum[live])) ** 2))) if live.any() else 0.0
    return gross, stat


def silu_grad(x):
    s = 1.0 / (1.0 + np.exp(-x))
    return s * (1.0 + x * (1.0 - s))


def reverse_operands(rng, M, K, N):
    """A: a gradient times SiLU'-like column factors (one-signed in most columns), rows over 2^-4 .. 1; B: ~N(0, 1/K) weights over 2^-2 .. 1."""
    g = rng.standard_normal((M, K)) * np.exp2(rng.uniform(-4, 0, size=(M, 1)))
    s = silu_grad(rng.standard_normal(K) * 1.5 + 0.5)[None, :] * np.where(rng.random((M, K)) < 0.8, 1.0, rng.standard_normal((M, K)))
    A = (np.abs(g) * s * np.sign(rng.standard_normal((M, 1)))).astype(np.float32)
    B = (rng.standard_normal((N, K)) / np.sqrt(K) * np.exp2(rng.uniform(-2, 0, size=(N, 1)))).astype(np.float32)
    return A, B


def test_six_products_stay_below_t24_and_three_products_do_not():
    rng = np.random.default_rng(11)
    M, N = 384, 64
    for K in sorted(set(REVERSE_K)):
        A, B = reverse_operands(rng, M, K, N)
        a, b = A.astype(np.float64), B.astype(np.float64)
        c64, abs_sum, sq_sum = a @ b.T, np.abs(a) @ np.abs(b).T, (a * a) @ (b * b).T
        c6 = MM.gemm_bf16x3(A, B, None, "plain", alt_rows=True)
        c3 = MM.gemm_bf16x3(A, B, None, TWO_PLANE, alt_rows=True)
        g6, s6 = link_stats(c6, c64, abs_sum, sq_sum)
        g3, s3 = link_stats(c3, c64, abs_sum, sq_sum)
        print(f"K {K:4d}: six products stat {s6:.2e} gross {g6:.2e} (kappa {kappa('bf16x3', K):.1e});  "
              f"three products stat {s3:.2e} gross {g3:.2e} (kappa {kappa('split-bf16', K):.1e})")
        # measured (seed 11, 384 rows x 64 columns): six products 1.7e-7 (K 128) ... 6.0e-7 (K 1536) = 0.25 - 0.27 * 2^-24 sqrt(K);
        # three products 4.3e-6 - 4.6e-6; gross 2.0e-7 - 2.9e-7 (six) and 9.6e-7 - 3.5e-6 (three)
        assert s6 <= t24(K), (K, s6)
        assert s3 >= (4 if K <= 640 else 3) * t24(K), (K, s3)
        assert g6 <= kappa("bf16x3", K) and g3 <= kappa("split-bf16", K), (K, g6, g3)


def test_aligned_planes_keep_a_small_in_group_element_unbiased():
    """ADVICE r6's case: in one pass group (8 consecutive k of a row) an x element 2^-14 below the group's largest meets a weight 2^6 above
    the others.  Aligned planes round the leading plane to 2^(e_max - 12) of the group, so that element's leading plane is 0 or 2^(e_max - 12)
    and its remainder goes down planes 1 and 2: it keeps 16 - 23 of its bits, not 24 -- an error of at most ~2^-16 of its product, which is
    2^-8 of the group's largest here: 2^-24 of the group.  The error has random sign with the element: no bias, with or without alignment."""
    lib = MM.load_lib()
    rng = np.random.default_rng(5)
    M, K, N = 4096, 16, 8
    A = (rng.uniform(0.5, 1.0, size=(M, K)) * np.sign(rng.standard_normal((M, K)))).astype(np.float32)
    A[:, 3] = (rng.uniform(1.0, 2.0, size=M) * 2.0 ** -14 * np.sign(rng.standard_normal(M))).astype(np.float32)   # x ratio 2^-14 in group 0
    B = rng.uniform(0.5, 1.0, size=(N, K)).astype(np.float32) * 2.0 ** -6
    B[:, 3] = rng.uniform(0.5, 1.0, size=N).astype(np.float32)                                                    # w ratio 2^6 at that k
    a, b = A.astype(np.float64), B.astype(np.float64)
    exact, abs_sum = a @ b.T, np.abs(a) @ np.abs(b).T
    da, dw, dw2 = (C.c_int.in_dll(lib, n) for n in ("gemm_dem_a", "gemm_dem_w", "gemm_dem_w2"))
    try:
        res = {}
        for align in (0, 12):
            da.value = dw.value = dw2.value = align
            res[align] = MM.gemm_bf16x3(A, B, None, "plain", alt_rows=True).astype(np.float64) - exact
    finally:
        da.value = dw.value = dw2.value = 0
    for align, err in res.items():
        rel = err / abs_sum
        t = rel.mean(0) / (rel.std(0) / np.sqrt(M))
        print(f"align {align:2d}: max |error| / sum|ab| {np.abs(rel).max():.2e}, |mean| / standard error per column <= {np.abs(t).max():.1f}")
        assert np.abs(rel).max() <= 8 * U, (align, float(np.abs(rel).max()))     # a 16-k MFMA: two passes, a handful of 2^-24 roundings
        assert np.abs(t).max() < 5.0, (align, t)
