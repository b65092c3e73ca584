"""CPU calibration of what tests/test_gpu_forward_gemm_links.py holds the engine's FORWARD GEMMs to (no GPU).

The calibration of tests/test_reverse_precision_cpu.py (`kappa`, `t24`, `link_stats`), carried to the forward products on the bit-exact model
of the matrix core (tools/mfma_model.py): the radial fc3 (K 128), conv-1 m0 / m1 / m2 (K 768, 2 x 512, 2 x 256) and conv-2 m0 / m1 / m2
(K 384, 2 x 256, 2 x 128).  A plain product has one-signed SiLU-like A columns and a bias; a complex one has sign-symmetric A columns, no bias,
and its two halves joined by one float32 subtraction (y_re = x_re . Wa^T - x_im . Wb^T), so its depth is twice the half's.  Weights
~N(0, 1/K); odd rows negated as the engine stores them.  Every accumulation form of umx_gemm_q.h is run -- `plain` (one accumulator), `ls1`
(the 2^-16-order products chained from zero every 16-k step and folded in), `ls2` (a second accumulator for the whole k loop) -- with aligned
leading planes on (gemm_dem_* = 12) and off.

Per form and K:
  * the six-product statistic is below `t24(K)` -- every form fits it on the model, measured 0.11 ... 0.46 of it, so no form needs a
    threshold of its own;
  * with any ONE of the three 2^-16-order plane products taken out of the program it is above: the check sees a lost plane product;
  * the gross error per element is within `kappa_fwd`.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mfma_model as MM  # noqa: E402
from test_reverse_precision_cpu import U, kappa, link_stats, t24  # noqa: E402

# (link, complex, K of the link): a complex link's K counts both halves of the joined sum
FORWARD_LINKS = (("fc3", 0, 128), ("conv-1 m0", 0, 768), ("conv-1 m1", 1, 2 * 512), ("conv-1 m2", 1, 2 * 256),
                 ("conv-2 m0", 0, 384), ("conv-2 m1", 1, 2 * 256), ("conv-2 m2", 1, 2 * 128))
FORMS = ("plain", "ls1", "ls2")
LOW_ORDER = ((0, 2), (1, 1), (2, 0))          # the plane products of order 2^-16 (planes qa of A, qb of W)


def kappa_fwd(mode: str, K: int, form: str = "plain", staged: bool = False) -> float:
    """Per-element worst case of a forward product, in units of sum_k |a_k b_k| + |bias|: `kappa(mode, K)` -- the roundings of the running
    sums, the dropped plane products, and (its constant 8) the bias seed and the one float32 join of a complex product -- plus
      ls1    one float32 add per 16-k step folds the spare accumulator into the main one: K / 16 roundings, each of a partial sum that
             sum|ab| + |bias| bounds                                                                                        -> K / 16
      ls2    the second accumulator is added once, behind the k loop                                                          -> 1
      staged (fp32 conv-1: A = xrot * rad formed while A is staged) every a_k is one rounded float32 product, a relative
             error of u in every term of the sum, which the float64 reference (exact xrot * rad) does not have                -> 1"""
    folds = {"plain": 0.0, "ls1": K / 16.0, "ls2": 1.0}[form]
    return kappa(mode, K) + (folds + (1.0 if staged else 0.0)) * U


def silu(x):
    return x / (1.0 + np.exp(-x))


def forward_operands(rng, M, K, N, cplx):
    """plain: SiLU outputs, one-signed in most columns (a column's pre-activations share an offset), rows over 2^-3 .. 1, and a bias;
    complex (K = one half's depth): rotated l >= 1 components, sign-symmetric.  W ~ N(0, 1/K), rows over 2^-2 .. 1."""
    scale = np.exp2(rng.uniform(-3, 0, size=(M, 1)))
    if cplx:
        A = rng.standard_normal((M, K)) * scale
    else:
        A = silu(rng.standard_normal((M, K)) * 0.7 + rng.standard_normal(K)[None, :] * 1.5 + 0.5) * scale
    B = rng.standard_normal((N, K)) / np.sqrt(K) * np.exp2(rng.uniform(-2, 0, size=(N, 1)))
    bias = None if cplx else (rng.standard_normal(N) * 0.1).astype(np.float32)
    return A.astype(np.float32), B.astype(np.float32), bias


def scheme_without(form, drop=None):
    s = MM.SCHEMES[form]
    return dict(prog=[p for p in s["prog"] if (p[0], p[1]) != drop], fold_step=s["fold_step"], fold_end=s["fold_end"])


def run_link(ops, cplx, scheme):
    """(C, C64, sum|ab| + |bias|, sum (ab)^2 + bias^2) of one link on the model: plain, or the re part of a complex product"""
    g = lambda A, B, b: MM.gemm_bf16x3(A, B, b, scheme, alt_rows=True)   # noqa: E731
    f8 = lambda x: x.astype(np.float64)   # noqa: E731
    if not cplx:
        A, B, bias = ops
        a, b, c0 = f8(A), f8(B), f8(bias)[None, :]
        return g(A, B, bias), a @ b.T + c0, np.abs(a) @ np.abs(b).T + np.abs(c0), (a * a) @ (b * b).T + c0 * c0
    (Are, Wa, _), (Aim, Wb, _) = ops
    c = g(Are, Wa, None) - g(Aim, Wb, None)                              # one float32 subtraction, as the epilogue's
    ar, ai, wa, wb = f8(Are), f8(Aim), f8(Wa), f8(Wb)
    return c, ar @ wa.T - ai @ wb.T, np.abs(ar) @ np.abs(wa).T + np.abs(ai) @ np.abs(wb).T, (ar * ar) @ (wa * wa).T + (ai * ai) @ (wb * wb).T


@pytest.mark.parametrize("align", [12, 0])
def test_forward_forms_stay_below_their_threshold_and_a_lost_plane_product_does_not(align):
    lib = MM.load_lib()
    dem = [C.c_int.in_dll(lib, n) for n in ("gemm_dem_a", "gemm_dem_w", "gemm_dem_w2")]
    rng = np.random.default_rng(23)
    M, N = 128, 32
    bad = []
    try:
        for d in dem:
            d.value = align
        for link, cplx, K in FORWARD_LINKS:
            ops = (forward_operands(rng, M, K // 2, N, 1), forward_operands(rng, M, K // 2, N, 1)) if cplx else forward_operands(rng, M, K, N, 0)
            for form in FORMS:
                c, c64, abs_sum, sq_sum = run_link(ops, cplx, MM.SCHEMES[form])
                g6, s6 = link_stats(c, c64, abs_sum, sq_sum)
                thr = t24(K)
                s5 = []
                for drop in LOW_ORDER:
                    c5 = run_link(ops, cplx, scheme_without(form, drop))[0]
                    s5.append(link_stats(c5, c64, abs_sum, sq_sum)[1])
                print(f"align {align:2d} {link:10s} K {K:4d} {form:5s}: six products stat {s6:.2e} (T24 {thr:.2e}), gross {g6:.2e} "
                      f"(kappa {kappa_fwd('bf16x3', K, form):.1e}); five products stat {min(s5):.2e} .. {max(s5):.2e}")
                if s6 > thr:
                    bad.append((link, form, "six products over the threshold", s6, thr))
                if min(s5) <= thr:
                    bad.append((link, form, "a lost plane product stays under the threshold", min(s5), thr))
                if g6 > kappa_fwd("bf16x3", K, form):
                    bad.append((link, form, "gross", g6))
    finally:
        for d in dem:
            d.value = 0
    assert not bad, bad


def test_fp32_sequential_sums_fit_the_same_thresholds():
    """The fp32 mode's forward links on the host: float32 operands, products summed in float32 (32-k partial sums, then across them -- any
    order is within kappa), the conv-1 operand the ROUNDED float32 product xrot * rad against the float64 reference of the exact product."""
    rng = np.random.default_rng(29)
    M, N = 128, 32
    for link, cplx, K in FORWARD_LINKS:
        A, B, bias = forward_operands(rng, M, K, N, 0 if not cplx else 1)
        staged = link.startswith("conv-1")
        a64 = A.astype(np.float64)
        if staged:
            R = silu(rng.standard_normal((M, K)) + 0.5).astype(np.float32)
            a64 = a64 * R.astype(np.float64)
            A = A * R                                                     # float32: rounded once
        b64 = B.astype(np.float64)
        c0 = 0.0 if bias is None else bias.astype(np.float64)[None, :]
        acc = np.zeros((M, N), np.float32) + (0 if bias is None else bias[None, :])
        for k0 in range(0, K, 32):
            part = np.zeros((M, N), np.float32)
            for k in range(k0, k0 + 32):
                part += A[:, k:k + 1] * B[None, :, k]
            acc += part
        gross, stat = link_stats(acc, a64 @ b64.T + c0, np.abs(a64) @ np.abs(b64).T + np.abs(c0), (a64 * a64) @ (b64 * b64).T + c0 * c0)
        print(f"fp32 {link:10s} K {K:4d}{' staged' if staged else ''}: stat {stat:.2e} (T24 {t24(K):.2e}), gross {gross:.2e} (kappa {kappa_fwd('fp32', K, 'plain', staged):.1e})")
        assert stat <= t24(K), (link, stat)
        assert gross <= kappa_fwd("fp32", K, "plain", staged), (link, gross)
