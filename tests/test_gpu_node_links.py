"""The node-level kernels (rows = atoms or atom x grid point), link by link, against float64 -- at the row counts where they change shape.

tests/test_gpu_reverse_links.py and tests/test_gpu_edge_links.py hold the edge side of the model link by link.  Here every kernel and GEMM
whose rows are atoms is replayed on the CPU in float64 from the engine's OWN captured input and compared with the engine's captured output
element by element.  No oracle forward pass is run.  The float64 formulas are built from the forward weight dict (oracle.Oracle(w).p: the
transposes of the reverse pass are the forward weights used from the other side, the engine's transposed copies are never read) and are
written plainly below (equal to oracle.rms_norm_sh and oracle/staged.py's norm_bwd, atomwise_fwd / atomwise_bwd and silu_grad: asserted in
tests/test_node_links_cpu.py); none is transcribed from a kernel.

    link                  captured input                                  -> captured output                   kernel / launcher
    norm 1                x0 | x.(i-1), sysemb                            -> xn.i                              k_norm_fwd (float64 row, sysemb)
    norm 2, final norm    xmid.i | x.(NL-1)                               -> xn2.i | xf                        k_norm_fwd (float64 row)
    scalar MLP            xn2.i (l = 0)                                   -> gspre.i                           gemm_node
    SO(3) linear 1        xn2.i                                           -> ffh.i                             so3_linear (z -> l map, bias on z = 0)
    gate                  ffh.i, gspre.i                                  -> ffhg.i                            k_gate_node_fwd
    SO(3) linear 2        ffhg.i, xmid.i                                  -> x.i                               so3_linear (residual)
    to grid               xn2.i                                           -> gridin.i                          k_grid_expand
    grid MLP              gridin.i -> ffg1.i -> ffg2.i                    -> gridout.i                         gemm_grid, two with A_SILU staging
    from grid             gridout.i, xmid.i                               -> x.i                               k_grid_contract (float64 sum + residual)
    readout               xf -> pre1 -> pre2                              -> e_node, E                         gemm_node x 2 (A_SILU), k_energy_node, k_energy
    readout^T             pre2 | g_pre2 | g_sil1, pre1 | g_pre1           -> g_pre2 | g_sil1 | g_pre1 | g_xf   k_silu_bwd (broadcast row), e2T, k_silu_bwd, e0T
    final norm^T          g_xf, x.(NL-1)                                  -> g_xfinal                          k_norm_bwd (no gres)
    SO(3) linear 2^T      g_xin.(i+1) | g_xfinal                          -> g_ffhg.i                          so3_linear (l2T)
    gate^T                g_ffhg.i, ffh.i, gspre.i                        -> g_ffh.i, g_gs.i                   k_gate_node_bwd
    SO(3) linear 1^T      g_ffh.i                                         -> g_xn2a.i                          so3_linear (l1T)
    scalar MLP^T          g_gs.i, g_xn2a.i                                -> g_xn2.i                           gemm_node in place (Cp == resid, l = 0 columns)
    from grid^T           g_xin.(i+1) | g_xfinal                          -> g_gridout.i                       k_grid_expand with from_grid
    grid MLP^T            g_gridout.i -> g_gsil2.i -> g_ffg2.i ->         -> g_gridin.i                        gemm_grid (g3T, g2T, g1T), k_silu_bwd x 2
                          g_gsil1.i -> g_ffg1.i; ffg2.i, ffg1.i
    to grid^T             g_gridin.i                                      -> g_xn2.i                           k_grid_contract with to_grid, no residual
    norm 2^T              g_xn2.i, xmid.i, g_xin.(i+1) | g_xfinal         -> g_xmid.i                          k_norm_bwd (gres)
    norm 1^T              g_xn.i, x0 | x.(i-1), g_xmid.i                  -> g_xin.i                           k_norm_bwd (gres)

Captures added for this test (umx_plan.h, each directly behind the launch that writes its buffer): forward ffhg.i, xf, gridin.i, gridout.i;
readout^T g_pre2, g_sil1 (dE / d silu(pre1)), g_pre1, g_xf (the whole row); spectral g_ffhg.i, g_ffh.i, g_gs.i, g_xn2a.i (before the scalar
MLP^T lands), g_xn2.i; grid g_gridout.i, g_gsil2.i, g_ffg2.i, g_gsil1.i, g_ffg1.i, g_gridin.i, g_xn2.i.  The node initialisation (element
embedding + system embedding, added in double) is part of x0 and is held by the edge-link test's "deg rotate back + sum x0" link: the
single-GPU plan has no launch of its own for it.

Cases: feed-forward {spectral, grid with biases} x accumulation {float64 (default), UMX_NODE_F64=0 + UMX_GRID_F64=0: the fp32-MFMA body}
x size, precision mode bf16x3; one fp32-mode case (the node links do not depend on the mode).
Sizes (preconditions asserted from the captured row_ptr and sizes): A = 3 atoms x 1 image (one partial block of the wave-per-node kernels,
one partial 64-row tile); B = 13 x 5 = 65 rows (one row past a 64-row tile, node % natoms at work, 5 blocks of k_energy); C = 43 x 3 = 129
rows (one row past the 128-row tile of the fp32 body; grid form 129 G rows ending in a partial tile); D = 257 x 1 (k_energy's strided loop
takes a second pass for one atom; five 64-row tiles + one row).

Bounds, per element, nothing relative to a tensor's maximum, no element excluded (u = 2^-24, gamma_k = k u / (1 - k u)):
  * float64-carried links (k_norm_fwd, k_grid_contract, k_energy_node, k_gemm_f64acc): u |ref64| + (terms + 2) 2^-53 sum|terms| -- "computed
    in double, rounded once"; the same link accumulated in float32 fails it (mutation 9, and the `f32 acc` ratio printed beside each);
  * k_energy: float64 throughout: natoms 2^-53 rmsd sum|e_node|, + 2^-53 |E| for the rounding of the float64 sum with the reference
    energies and natoms 2^-53 sum|element_refs| for the order in which the host adds those up;
  * float32 arithmetic links: gamma_k sum|terms| + u |ref64|, sum|terms| = the same formula on absolute values, k derived beside each link;
  * links through expf: (k_arith + 2 k_host) u |term|, k_host = the distance of the SAME formula in numpy float32 from float64 on the captured
    values, in u of the term (measured at run time against float64, printed; tests/test_gpu_edge_links.py's convention);
  * fp32-MFMA GEMMs: kappa("fp32", K) sum|terms| per element and the t24(K) statistic of tests/test_reverse_precision_cpu.py.
Structure, bitwise: the scalar MLP^T leaves every l > 0 column of g_xn2a as it was; e0T leaves the columns beyond C zero; every capture is
finite; image 0 of a batch (B) has the bits of the same image evaluated alone at every node capture.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import escn_md_oracle as O
from oracle import tables as OT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_edge_links import Report, _t, gamma, host_ulps, ratio  # noqa: E402
from test_reverse_precision_cpu import kappa, t24  # noqa: E402

pytestmark = pytest.mark.gpu

C, H, NL = OT.SPHERE_CHANNELS, OT.HIDDEN_CHANNELS, OT.NUM_LAYERS
ROW = 9 * C
U, E53 = 2.0 ** -24, 2.0 ** -53
T64, F32 = torch.float64, torch.float32
L_LP = torch.tensor(OT.L_OF_LP)
BAL = 1.0 / ((2.0 * L_LP.to(T64) + 1.0) * (OT.LMAX + 1))            # 1/3, 1/9 x 3, 1/15 x 5
SIZES = {"A": (3, 1), "B": (13, 5), "C": (43, 3), "D": (257, 1)}    # atoms, images
FF = {"spectral": {}, "grid": dict(ff_type="grid", grid_bias=True)}


class Link:
    """one replayed link: ref64, the per-element bound, and for a GEMM K, sum (a b)^2 and the float32-accumulated restatement"""

    def __init__(self, ref, bound, k=0.0, K=0, sq=None, f32=None):
        self.ref, self.bound, self.k, self.K, self.sq, self.f32 = ref, bound, k, K, sq, f32


def sig(x):
    return torch.sigmoid(x)


def silu(x):
    return x * sig(x)


def dsilu(x):
    s = sig(x)
    return s * (1.0 + x * (1.0 - s))


def dsilu_abs(x):
    """SiLU' on absolute values: the term of its bound"""
    s = sig(x)
    return s * (1.0 + x.abs() * (1.0 - s))


# ---- norms ---------------------------------------------------------------------------------------------------------------------------------
def _feat(x, center=True):
    mean0 = x[:, 0:1].mean(2, keepdim=True)
    feat = torch.cat([x[:, 0:1] - (mean0 if center else 0.0), x[:, 1:]], dim=1)
    fabs = torch.cat([x[:, 0:1].abs() + x[:, 0:1].abs().mean(2, keepdim=True), x[:, 1:].abs()], dim=1)
    return feat, fabs


def _rstd(feat):
    return ((feat ** 2 * BAL[None, :, None]).sum(dim=(1, 2), keepdim=True) / C + OT.NORM_EPS) ** -0.5


def link_norm_fwd(x, aw, ab, sysemb=None, sys_floor=None, center=True):
    """y = feat s aw[l] (+ ab + sysemb on l = 0), feat = x with the channel mean of l = 0 removed, s = (mean_c sum_r bal_r feat^2 + eps)^-1/2.
    Carried in double, rounded once.  Terms of the floor: the channel mean (C) and the sum of squares (9 C; all positive, so its relative
    error is s's): 10 C; sum|terms| = (|x| + mean|x| on l = 0) s |aw| + |ab| + |sysemb|.  sys_floor: the double arithmetic behind sysemb."""
    feat, fabs = _feat(x, center)
    s = _rstd(feat)
    ref = feat * s * aw[L_LP][None]
    terms = fabs * s * aw[L_LP][None].abs()
    add = ab if sysemb is None else ab + sysemb
    ref = torch.cat([ref[:, 0:1] + add[None, None], ref[:, 1:]], dim=1)
    terms = torch.cat([terms[:, 0:1] + (ab.abs() if sysemb is None else ab.abs() + sysemb.abs())[None, None], terms[:, 1:]], dim=1)
    bound = U * ref.abs() + (10 * C + 2) * E53 * terms
    if sys_floor is not None:
        bound = torch.cat([bound[:, 0:1] + sys_floor[None, None], bound[:, 1:]], dim=1)
    return Link(ref, bound, 1)


# float32 roundings on the longest path of k_norm_bwd.  The channel mean: 1 sum per lane, log2(64) + 1 = 7 for the wave sum, the product with
# 1 / C: 9, the subtraction: feat 10.  q: feat^2 doubles that (20) + 1, 18 products summed per lane (18), three divisions and two sums (5), the
# wave sum (7), 1 / C (1): 52 -- s = (q + eps)^-1/2 halves it (26) + the sum, the square root, the division: 29.  g aw: 1.  dot: g aw (1), feat
# (10), the product (1), 18 sums, the wave sum (7): 37.  k = s^3 dot / C: 3 x 29 + 2 + 37 + 2 = 128.  k bal feat: 128 + 2 + 10 = 140, the
# subtraction from g aw s (31): 141.  The l = 0 mean of the result (9) and its subtraction (1): 151; the residual: 152.
K_NORM_BWD = 152


def link_norm_bwd(gy, x, aw, gres=None, bal=BAL):
    """gx = gres + d(norm)/dx^T gy (float32): g_feat = gw s - s^3 (sum gw feat) bal feat / C, gw = gy aw[l]; the l = 0 row minus its channel
    mean.  `bal` is the balance of the gradient term alone (the mutation swaps it; s is the forward's)."""
    feat, fabs = _feat(x)
    s = _rstd(feat)
    gw = gy * aw[L_LP][None]
    dot = (gw * feat).sum(dim=(1, 2), keepdim=True)
    dabs = (gw.abs() * fabs).sum(dim=(1, 2), keepdim=True)
    gf = gw * s - s ** 3 * dot * bal[None, :, None] * feat / C
    ga = gw.abs() * s + s ** 3 * dabs * bal[None, :, None] * fabs / C
    ref = torch.cat([gf[:, 0:1] - gf[:, 0:1].mean(2, keepdim=True), gf[:, 1:]], dim=1)
    terms = torch.cat([ga[:, 0:1] + ga[:, 0:1].mean(2, keepdim=True), ga[:, 1:]], dim=1)
    if gres is not None:
        ref, terms = ref + gres, terms + gres.abs()
    return Link(ref, gamma(K_NORM_BWD) * terms + U * ref.abs(), K_NORM_BWD)


# ---- GEMMs ---------------------------------------------------------------------------------------------------------------------------------
def _gemm_link(prod, pabs, sq, K, extra, acc, k_silu, f32):
    """prod = sum_k a b, pabs = sum |a b|, sq = sum (a b)^2; extra: the bias / residual tensors added behind the sum.
    float64 body: rounded once: u |ref| + (K + extras + 2) 2^-53 sum|terms|.  fp32-MFMA body: kappa("fp32", K) sum|terms| (its 8 u beyond
    the K products hold the float32 bias and residual sums and the stored value).  A_SILU staging: SiLU in float32 before the products:
    + 2 k_host u sum|a b| (k_arith = 0: the operand is the expf formula and nothing else)."""
    ref, terms = prod, pabs
    for e in extra:
        ref, terms, sq = ref + e, terms + e.abs(), sq + e * e
    if acc == "f64":
        bound = U * ref.abs() + (K + len(extra) + 2) * E53 * terms
    else:
        bound = kappa("fp32", K) * terms
    if k_silu is not None:
        bound = bound + 2.0 * k_silu * U * pabs
    k = (1 if acc == "f64" else K + 8) + (2.0 * k_silu if k_silu is not None else 0.0)
    return Link(ref, bound, k, K, sq, f32)


def link_gemm(A, Wm, bias=None, resid=None, acc="f64", k_silu=None):
    """C = act(A) Wm^T + bias + resid; A [m, K], Wm [N, K] (a transposed link passes the forward weight's .T)"""
    a = silu(A) if k_silu is not None else A
    extra = [e.expand(A.shape[0], Wm.shape[0]) for e in (bias, resid) if e is not None]
    a32, w32 = a.to(F32), Wm.to(F32)
    f32 = a32 @ w32.T
    for e in extra:
        f32 = f32 + e.to(F32)
    # (an A_SILU link is not float64-carried: its staging term admits a float32 sum, so no float32-accumulated ratio is reported for it)
    return _gemm_link(a @ Wm.T, a.abs() @ Wm.abs().T, (a * a) @ (Wm * Wm).T, A.shape[1], extra, acc, k_silu, f32.to(T64) if k_silu is None else None)


def link_so3(A, Wl, bias=None, resid=None, acc="f64", transpose=False, lmap=L_LP, bias_rows=(0,)):
    """SO(3) linear on l-primary rows: out[n, z] = A[n, z] W[l(z)]^T (+ bias on z = 0) (+ resid); transpose: the same weights from the other
    side (the reverse pass).  lmap / bias_rows: the z -> l map and the rows that take the bias (the mutations move them)."""
    Wz = Wl[lmap]
    eq = "nmo,moi->nmi" if transpose else "nmi,moi->nmo"
    prod, pabs, sq = torch.einsum(eq, A, Wz), torch.einsum(eq, A.abs(), Wz.abs()), torch.einsum(eq, A * A, Wz * Wz)
    extra = []
    if bias is not None:
        b = torch.zeros_like(prod)
        b[:, list(bias_rows)] = bias
        extra.append(b)
    if resid is not None:
        extra.append(resid)
    f32 = torch.einsum(eq, A.to(F32), Wz.to(F32))
    for e in extra:
        f32 = f32 + e.to(F32)
    return _gemm_link(prod, pabs, sq, A.shape[2], extra, acc, None, f32.to(T64))


# ---- gates, SiLU', grid projections, energy ------------------------------------------------------------------------------------------------
def _gate_scalars(gspre, kh):
    """s' = sigmoid(silu(p)) per degree and its error bound ds: the inner SiLU errs by 2 k_silu u |p| sigmoid(p), which the outer sigmoid
    scales by s' (1 - s'); the outer sigmoid adds 2 k_sigmoid u s'.  kh: k_host of SiLU on p and of the sigmoid on float32 SiLU(p)."""
    sp = sig(silu(gspre))
    ds = U * (2.0 * kh["gs_sigmoid"] * sp + sp * (1.0 - sp) * 2.0 * kh["gs_silu"] * gspre.abs() * sig(gspre))
    n = gspre.shape[0]
    ex = lambda t: t.reshape(n, OT.LMAX, H)[:, L_LP[1:] - 1]      # noqa: E731
    return sp, ds, ex


def link_gate_fwd(h, gspre, kh):
    """hg row 0 = SiLU(h) (k_arith 0); rows l > 0 = h s'_l: one product: |h| (ds + u s')"""
    sp, ds, ex = _gate_scalars(gspre, kh)
    ref = torch.cat([silu(h[:, 0:1]), h[:, 1:] * ex(sp)], dim=1)
    bound = torch.cat([2.0 * kh["h0_silu"] * U * h[:, 0:1].abs() * sig(h[:, 0:1]), h[:, 1:].abs() * (ex(ds) + U * ex(sp))], dim=1)
    return Link(ref, bound, 1 + 2 * kh["gs_sigmoid"] + 2 * kh["gs_silu"])


def link_gate_bwd(g, h, gspre, kh, row0=dsilu):
    """g_h row 0 = g SiLU'(h) (one product: k_arith 1); rows l > 0 = g s'_l (as forward).  g_gs_l = a s' (1 - s') SiLU'(p), a = the sum over
    the rows of degree l of g h (<= 5 products and 4 sums: gamma_6 |a|): fl(1 - s') errs by ds + u (1 - s'), SiLU'(p) by 2 k u of its term,
    three products -> sum|g h| [ (6 + 3 + 1) u s' (1 - s') G + ds (1 - s') G + s' ds G + 2 k u s' (1 - s') Gabs ]."""
    sp, ds, ex = _gate_scalars(gspre, kh)
    n = g.shape[0]
    gh = torch.cat([g[:, 0:1] * row0(h[:, 0:1]), g[:, 1:] * ex(sp)], dim=1)
    b_gh = torch.cat([(1 + 2.0 * kh["h0_silu_grad"]) * U * g[:, 0:1].abs() * dsilu_abs(h[:, 0:1]), g[:, 1:].abs() * (ex(ds) + U * ex(sp))], dim=1)
    pr = g[:, 1:] * h[:, 1:]
    a = torch.stack([pr[:, 0:3].sum(1), pr[:, 3:8].sum(1)], dim=1).reshape(n, OT.LMAX * H)
    aabs = torch.stack([pr[:, 0:3].abs().sum(1), pr[:, 3:8].abs().sum(1)], dim=1).reshape(n, OT.LMAX * H)
    G, Gabs = dsilu(gspre), dsilu_abs(gspre)
    ggs = a * sp * (1.0 - sp) * G
    b_ggs = aabs * (10.0 * U * sp * (1.0 - sp) * G.abs() + ds * (1.0 - sp) * G.abs() + sp * ds * G.abs() + 2.0 * kh["gs_silu_grad"] * U * sp * (1.0 - sp) * Gabs)
    return Link(gh, b_gh, 1 + 2 * kh["h0_silu_grad"]), Link(ggs, b_ggs, 10 + 2 * kh["gs_silu_grad"])


def link_silu_bwd(g, pre, k_host, f=dsilu):
    """out = g SiLU'(pre): one product: (1 + 2 k_host) u |g| SiLU'_abs(pre)"""
    return Link(g * f(pre), (1 + 2.0 * k_host) * U * g.abs() * dsilu_abs(pre), 1 + 2 * k_host)


def link_grid_expand(x, M):
    """out[n, g] = sum_i M[g, i] x[n, i] in float32: a chain of 9 fused multiply-adds: gamma_9"""
    ref = torch.einsum("gi,nic->ngc", M, x)
    return Link(ref, gamma(9) * torch.einsum("gi,nic->ngc", M.abs(), x.abs()) + U * ref.abs(), 9)


def link_grid_contract(y, M, resid=None):
    """out[n, i] = resid[n, i] + sum_g M[g, i] y[n, g], carried in double, rounded once: G (+ 1) terms"""
    ref, terms = torch.einsum("gi,ngc->nic", M, y), torch.einsum("gi,ngc->nic", M.abs(), y.abs())
    f32 = torch.zeros_like(ref, dtype=F32)
    for g in range(M.shape[0]):                      # the float32-accumulated restatement: one float32 product and sum per grid point
        f32 = f32 + M[g].to(F32)[None, :, None] * y[:, g].to(F32)[:, None, :]
    if resid is not None:
        ref, terms, f32 = ref + resid, terms + resid.abs(), f32 + resid.to(F32)
    n_terms = M.shape[0] + (1 if resid is not None else 0)
    return Link(ref, U * ref.abs() + (n_terms + 2) * E53 * terms, 1, f32=f32.to(T64))


def link_energy_node(pre2, w4, b4):
    """e_node = SiLU(pre2) . w + b in double (the exponential too: 6 more roundings), rounded once"""
    ref = silu(pre2) @ w4.reshape(-1) + b4.reshape(())
    terms = silu(pre2).abs() @ w4.reshape(-1).abs() + b4.abs().reshape(())
    f32 = (silu(pre2).to(F32) * w4.reshape(-1).to(F32)[None]).sum(1) + b4.reshape(()).to(F32)
    return Link(ref, U * ref.abs() + (H + 1 + 6 + 2) * E53 * terms, 1, f32=f32.to(T64))


def link_energy(e_node, natoms, rmsd, refsum, refs_abs):
    """E[img] = rmsd sum e_node + refsum, float64 throughout: natoms 2^-53 rmsd sum|e_node| for the sum; the float64 result is rounded once
    more (2^-53 |E|), and refsum is itself a float64 sum of natoms reference energies in the host's order (natoms 2^-53 sum|refs|)"""
    e = e_node.reshape(-1, natoms)
    ref = rmsd * e.sum(1) + refsum
    return Link(ref, natoms * E53 * rmsd * e.abs().sum(1) + E53 * ref.abs() + natoms * E53 * refs_abs, 0)


# ---- one evaluation ------------------------------------------------------------------------------------------------------------------------
def capture_names(ff, layers=range(NL)):
    """every node capture the replay reads"""
    names = ["xf", "pre1", "pre2", "e_node", "g_pre2", "g_sil1", "g_pre1", "g_xf", "g_xfinal", "x0"]
    per = ["xn", "xmid", "xn2", "x", "g_xn2", "g_xmid", "g_xn", "g_xin"]
    per += ["gridin", "ffg1", "ffg2", "gridout", "g_gridout", "g_gsil2", "g_ffg2", "g_gsil1", "g_ffg1", "g_gridin"] if ff == "grid" else \
        ["gspre", "ffh", "ffhg", "g_ffhg", "g_ffh", "g_gs", "g_xn2a"]
    return names + [f"{n}.{i}" for i in layers for n in per]


def measure_k_host(get, ff, layers):
    """k_host of every expf formula on the captured float32 arguments (numpy float32 against float64, in u of the term)"""
    kh = {}
    cat = lambda names: np.concatenate([get(n).reshape(-1) for n in names])      # noqa: E731
    r = host_ulps(cat(["pre1", "pre2"]))
    kh["ro_silu"], kh["ro_silu_grad"] = r["silu"], r["silu_grad"]
    if ff == "grid":
        r = host_ulps(cat([f"{n}.{i}" for i in layers for n in ("ffg1", "ffg2")]))
        kh["grid_silu"], kh["grid_silu_grad"] = r["silu"], r["silu_grad"]
    else:
        p = cat([f"gspre.{i}" for i in layers])
        r = host_ulps(p)
        kh["gs_silu"], kh["gs_silu_grad"] = r["silu"], r["silu_grad"]
        with np.errstate(over="ignore"):
            s32 = (p / (np.float32(1.0) + np.exp(-p))).astype(np.float32)
        kh["gs_sigmoid"] = host_ulps(s32)["sigmoid"]
        r = host_ulps(np.concatenate([get(f"ffh.{i}").reshape(-1, 9, H)[:, 0].reshape(-1) for i in layers]))
        kh["h0_silu"], kh["h0_silu_grad"] = r["silu"], r["silu_grad"]
    return kh


class NodeReport(Report):
    """Report + the fp32-MFMA statistic and the ratio the float32-accumulated restatement of a float64-carried link would have had"""

    def __init__(self, tag):
        super().__init__(tag)
        self.stats, self.alt = {}, {}

    def link(self, name, out, L, acc=None):
        assert bool(torch.isfinite(out).all()), name
        r = self.add(name, L.k, out, L.ref, L.bound)
        if L.f32 is not None and acc == "f64":
            self.alt[name] = max(self.alt.get(name, 0.0), ratio(L.f32, L.ref, L.bound)[0])
        if L.sq is not None and acc == "f32":
            live = L.sq > 0
            st = float(torch.sqrt((((out - L.ref)[live] / torch.sqrt(L.sq[live])) ** 2).mean())) if bool(live.any()) else 0.0
            s0, K0 = self.stats.get(name, (0.0, L.K))
            self.stats[name] = (max(s0, st), L.K)
        return r

    def close(self, extra=None):
        notes = dict(extra or {})
        for name, a in self.alt.items():
            notes[name] = notes.get(name, "") + f"  (f32 acc: {a:.3g})"
        for name, (st, K) in self.stats.items():
            notes[name] = notes.get(name, "") + f"  (stat {st / t24(K):.3f} t24)"
            if st > t24(K):
                self.failures.append((name, f"statistic {st:.3e} over t24({K}) = {t24(K):.3e}"))
        super().close(notes)


def replay_case(get, p, ff, acc, natoms, nimg, tag, sysemb, sys_floor, rmsd, refsum, refs_abs, energies, layers=tuple(range(NL)), keep=False):
    """Replay every node link of one evaluation.  get(name, dtype=np.float32): the captures; p: the float64 forward weights
    (oracle.Oracle(w).p); energies: what the evaluation returned.  Returns (NodeReport, kept, k_host): kept = what the mutations need."""
    nn = natoms * nimg
    rep = NodeReport(tag)
    kept = {}
    kh = measure_k_host(get, ff, layers)
    print(f"  [{tag}] k_host (u of the term): " + ", ".join(f"{k} {v:.2f}" for k, v in kh.items()))
    rows = lambda name, *shape: _t(get(name)).reshape(*shape)      # noqa: E731
    node = lambda name: rows(name, nn, 9, C)                       # noqa: E731
    last = NL - 1
    # ---- readout and its reverse head
    x_last, xf = node(f"x.{last}"), node("xf")
    pre1, pre2, e_node = rows("pre1", nn, H), rows("pre2", nn, H), rows("e_node", nn)
    rep.link("final norm xf", xf, link_norm_fwd(x_last, p["norm.affine_weight"], p["norm.affine_bias"]))
    e0, e2, e4 = p["energy_block.0.weight"], p["energy_block.2.weight"], p["energy_block.4.weight"]
    rep.link("readout pre1", pre1, link_gemm(xf[:, 0], e0, p["energy_block.0.bias"], acc=acc), acc)
    rep.link("readout pre2 (A_SILU)", pre2, link_gemm(pre1, e2, p["energy_block.2.bias"], acc=acc, k_silu=kh["ro_silu"]), acc)
    rep.link("readout e_node", e_node, link_energy_node(pre2, e4, p["energy_block.4.bias"]), "f64")
    rep.link("readout E", _t(energies), link_energy(e_node, natoms, rmsd, refsum, refs_abs))
    g_pre2, g_sil1, g_pre1, g_xf = rows("g_pre2", nn, H), rows("g_sil1", nn, H), rows("g_pre1", nn, H), node("g_xf")
    L_gpre2 = link_silu_bwd(e4.expand(nn, H), pre2, kh["ro_silu_grad"])
    rep.link("readout^T g_pre2 (broadcast row)", g_pre2, L_gpre2)
    rep.link("readout^T g_sil1 (e2T)", g_sil1, link_gemm(g_pre2, e2.T, acc=acc), acc)
    rep.link("readout^T g_pre1", g_pre1, link_silu_bwd(g_sil1, pre1, kh["ro_silu_grad"]))
    rep.link("readout^T g_xf (e0T)", g_xf[:, 0], link_gemm(g_pre1, e0.T, acc=acc), acc)
    assert not g_xf[:, 1:].any(), "e0T wrote beyond the l = 0 columns of the zeroed row"
    g_xfinal = node("g_xfinal")
    L_nb = link_norm_bwd(g_xf, x_last, p["norm.affine_weight"])
    rep.link("final norm^T g_xfinal", g_xfinal, L_nb)
    if keep:
        kept.update(g_pre2=(g_pre2, L_gpre2, e4.expand(nn, H), pre2, kh["ro_silu_grad"]), norm_bwd=(g_xfinal, L_nb, g_xf, x_last, p["norm.affine_weight"]))
    for i in layers:
        b, pa = f"blocks.{i}", f"blocks.{i}.atom_wise"
        x_in, xmid, xn2, x_out = node(f"x.{i - 1}" if i else "x0"), node(f"xmid.{i}"), node(f"xn2.{i}"), node(f"x.{i}")
        g_out = node(f"g_xin.{i + 1}") if i < last else g_xfinal
        L_n1 = link_norm_fwd(x_in, p[f"{b}.norm_1.affine_weight"], p[f"{b}.norm_1.affine_bias"], sysemb, sys_floor)
        rep.link(f"L{i} norm 1 xn (sysemb)", node(f"xn.{i}"), L_n1)
        rep.link(f"L{i} norm 2 xn2", xn2, link_norm_fwd(xmid, p[f"{b}.norm_2.affine_weight"], p[f"{b}.norm_2.affine_bias"]))
        if keep and i == layers[0]:
            kept["norm_fwd"] = (node(f"xn.{i}"), L_n1, x_in, p[f"{b}.norm_1.affine_weight"], p[f"{b}.norm_1.affine_bias"], sysemb, sys_floor)
        if ff == "grid":
            tg, fg = p["so3_grid.to_grid_mat"], p["so3_grid.from_grid_mat"]
            G = tg.shape[0]
            ng = nn * G
            w1, w2, w3 = (p[f"{pa}.grid_mlp.{li}.weight"] for li in (0, 2, 4))
            b1, b2, b3 = (p.get(f"{pa}.grid_mlp.{li}.bias") for li in (0, 2, 4))
            gridin, ffg1, ffg2, gridout = rows(f"gridin.{i}", nn, G, C), rows(f"ffg1.{i}", ng, H), rows(f"ffg2.{i}", ng, H), rows(f"gridout.{i}", nn, G, C)
            rep.link(f"L{i} to grid gridin", gridin, link_grid_expand(xn2, tg))
            rep.link(f"L{i} grid MLP ffg1", ffg1, link_gemm(gridin.reshape(ng, C), w1, b1, acc=acc), acc)
            rep.link(f"L{i} grid MLP ffg2 (A_SILU)", ffg2, link_gemm(ffg1, w2, b2, acc=acc, k_silu=kh["grid_silu"]), acc)
            rep.link(f"L{i} grid MLP gridout (A_SILU)", gridout.reshape(ng, C), link_gemm(ffg2, w3, b3, acc=acc, k_silu=kh["grid_silu"]), acc)
            L_x = link_grid_contract(gridout, fg, xmid)
            rep.link(f"L{i} from grid + residual x", x_out, L_x, "f64")
            g_go, g_s2, g_f2 = rows(f"g_gridout.{i}", nn, G, C), rows(f"g_gsil2.{i}", ng, H), rows(f"g_ffg2.{i}", ng, H)
            g_s1, g_f1, g_gi = rows(f"g_gsil1.{i}", ng, H), rows(f"g_ffg1.{i}", ng, H), rows(f"g_gridin.{i}", nn, G, C)
            L_go = link_grid_expand(g_out, fg)
            rep.link(f"L{i} from grid^T g_gridout", g_go, L_go)
            rep.link(f"L{i} grid MLP^T g_gsil2 (g3T)", g_s2, link_gemm(g_go.reshape(ng, C), w3.T, acc=acc), acc)
            rep.link(f"L{i} grid MLP^T g_ffg2", g_f2, link_silu_bwd(g_s2, ffg2, kh["grid_silu_grad"]))
            rep.link(f"L{i} grid MLP^T g_gsil1 (g2T)", g_s1, link_gemm(g_f2, w2.T, acc=acc), acc)
            rep.link(f"L{i} grid MLP^T g_ffg1", g_f1, link_silu_bwd(g_s1, ffg1, kh["grid_silu_grad"]))
            rep.link(f"L{i} grid MLP^T g_gridin (g1T)", g_gi.reshape(ng, C), link_gemm(g_f1, w1.T, acc=acc), acc)
            g_xn2 = node(f"g_xn2.{i}")
            L_gx = link_grid_contract(g_gi, tg)
            rep.link(f"L{i} to grid^T g_xn2", g_xn2, L_gx, "f64")
            if keep and i == layers[0]:
                kept.update(x=(x_out, L_x, xmid), g_gridout=(g_go, L_go, g_out, tg), g_xn2_grid=(g_xn2, L_gx, g_gi, fg), G=G)
        else:
            smlp, l1w, l2w = p[f"{pa}.scalar_mlp.weight"], p[f"{pa}.so3_linear_1.weight"], p[f"{pa}.so3_linear_2.weight"]
            gspre, ffh, ffhg = rows(f"gspre.{i}", nn, 2 * H), rows(f"ffh.{i}", nn, 9, H), rows(f"ffhg.{i}", nn, 9, H)
            rep.link(f"L{i} scalar MLP gspre", gspre, link_gemm(xn2[:, 0], smlp, p[f"{pa}.scalar_mlp.bias"], acc=acc), acc)
            L_h = link_so3(xn2, l1w, p[f"{pa}.so3_linear_1.bias"], acc=acc)
            rep.link(f"L{i} SO(3) linear 1 ffh", ffh, L_h, acc)
            rep.link(f"L{i} gate ffhg", ffhg, link_gate_fwd(ffh, gspre, kh))
            L_x = link_so3(ffhg, l2w, p[f"{pa}.so3_linear_2.bias"], xmid, acc=acc)
            rep.link(f"L{i} SO(3) linear 2 + residual x", x_out, L_x, acc)
            g_ffhg, g_ffh, g_gs = node(f"g_ffhg.{i}"), node(f"g_ffh.{i}"), rows(f"g_gs.{i}", nn, 2 * H)
            g_xn2a, g_xn2 = node(f"g_xn2a.{i}"), node(f"g_xn2.{i}")
            rep.link(f"L{i} SO(3) linear 2^T g_ffhg", g_ffhg, link_so3(g_out, l2w, acc=acc, transpose=True), acc)
            L_gh, L_gs = link_gate_bwd(g_ffhg, ffh, gspre, kh)
            rep.link(f"L{i} gate^T g_ffh", g_ffh, L_gh)
            rep.link(f"L{i} gate^T g_gs", g_gs, L_gs)
            rep.link(f"L{i} SO(3) linear 1^T g_xn2a", g_xn2a, link_so3(g_ffh, l1w, acc=acc, transpose=True), acc)
            rep.link(f"L{i} scalar MLP^T g_xn2 (in place)", g_xn2[:, 0], link_gemm(g_gs, smlp.T, resid=g_xn2a[:, 0], acc=acc), acc)
            assert np.array_equal(get(f"g_xn2.{i}").reshape(nn, 9, C)[:, 1:].view(np.uint32), get(f"g_xn2a.{i}").reshape(nn, 9, C)[:, 1:].view(np.uint32)), \
                "the scalar MLP^T touched a column of l > 0"
            if keep and i == layers[0]:
                kept.update(ffh=(ffh, L_h, xn2, l1w, p[f"{pa}.so3_linear_1.bias"]), x=(x_out, L_x, xmid))
        rep.link(f"L{i} norm 2^T g_xmid (gres)", node(f"g_xmid.{i}"), link_norm_bwd(g_xn2, xmid, p[f"{b}.norm_2.affine_weight"], g_out))
        rep.link(f"L{i} norm 1^T g_xin (gres)", node(f"g_xin.{i}"), link_norm_bwd(node(f"g_xn.{i}"), x_in, p[f"{b}.norm_1.affine_weight"], node(f"g_xmid.{i}")))
    rep.close()
    return rep, kept, kh


# ---- the checker must be able to fail: host-side mutations ---------------------------------------------------------------------------------
def mutation_checks(kept, ff, acc, nn):
    """Each mutation is applied to a captured output (shifted by what the mutated formula changes, or rows moved) and must be rejected:
    largest |err| / bound > 1.  Returns {name: ratio}."""
    out = {}
    rej = lambda o, L: ratio(o, L.ref, L.bound)[0]     # noqa: E731
    shift = lambda o, L, Lm: rej(o + (Lm.ref - L.ref), L)      # noqa: E731
    if ff == "spectral":
        ffh, L, xn2, l1w, l1b = kept["ffh"]
        out["1 so3_linear bias on an l = 1 row"] = shift(ffh, L, link_so3(xn2, l1w, l1b, acc=acc, bias_rows=(0, 1)))
        lm = L_LP.clone()
        lm[4] = 1
        out["2a degree-1 weights for z = 4"] = shift(ffh, L, link_so3(xn2, l1w, l1b, acc=acc, lmap=lm))
        lm = L_LP.clone()
        lm[3] = 2
        out["2b degree-2 weights for z = 3"] = shift(ffh, L, link_so3(xn2, l1w, l1b, acc=acc, lmap=lm))
        if acc == "f64":
            out["9a so3_linear accumulated in float32"] = rej(L.f32, L)
    x, L, xmid = kept["x"]
    m = x.clone()
    m[nn - 1] -= xmid[nn - 1]
    out["3 residual dropped from the last row"] = rej(m, L)
    m = x.clone()
    m[nn - 1] = x[nn - 2]
    out["4 row nn - 1 = row nn - 2"] = rej(m, L)
    xn, L, x_in, aw, ab, sysemb, sys_floor = kept["norm_fwd"]
    out["5 k_norm_fwd without the l = 0 mean removal"] = shift(xn, L, link_norm_fwd(x_in, aw, ab, sysemb, sys_floor, center=False))
    gx, L, gy, xx, aw = kept["norm_bwd"]
    swapped = torch.where(L_LP == 1, torch.tensor(1.0 / 15.0, dtype=T64), torch.where(L_LP == 2, torch.tensor(1.0 / 9.0, dtype=T64), BAL))
    # (the final norm's incoming gradient lives in l = 0 only; the swapped balance shows in the rows of l > 0, through the dot-product term)
    out["6 1/9 and 1/15 swapped in k_norm_bwd"] = shift(gx, L, link_norm_bwd(gy, xx, aw, bal=swapped))
    if ff == "grid":
        g_go, L, g_out, tg = kept["g_gridout"]
        out["7a to_grid in place of from_grid (reverse expand)"] = shift(g_go, L, link_grid_expand(g_out, tg))
        g_xn2, L, g_gi, fg = kept["g_xn2_grid"]
        out["7b from_grid in place of to_grid (reverse contract)"] = shift(g_xn2, L, link_grid_contract(g_gi, fg))
        if acc == "f64":
            x, L, xmid = kept["x"]
            out["9b k_grid_contract accumulated in float32"] = rej(L.f32, L)
    g_pre2, L, g, pre, k = kept["g_pre2"]
    out["8 silu in place of silu' in k_silu_bwd"] = shift(g_pre2, L, link_silu_bwd(g, pre, k, f=silu))
    return out


N_MUTATIONS = {("spectral", "f64"): 9, ("spectral", "f32"): 8, ("grid", "f64"): 8, ("grid", "f32"): 7}


# ---- coverage preconditions ----------------------------------------------------------------------------------------------------------------
def size_facts(natoms, nimg, G=0):
    nn = natoms * nimg
    f = dict(nn=nn, wave_blocks=(nn + 3) // 4, wave_tail=nn % 4, tiles64=(nn + 63) // 64, tail64=nn % 64, tiles128=(nn + 127) // 128, tail128=nn % 128,
             energy_blocks=nimg, energy_passes=(natoms + 255) // 256, energy_tail=natoms % 256)
    if G:
        f.update(ng=nn * G, g_tail64=nn * G % 64, g_tail128=nn * G % 128)
    return f


def check_size(size, f):
    """the shape changes the issue names, per size"""
    if size == "A":
        assert f["nn"] == 3 and f["wave_blocks"] == 1 and f["wave_tail"] == 3 and f["tiles64"] == 1 and f["tail64"] == 3, f
    if size == "B":
        assert f["nn"] == 65 and f["tiles64"] == 2 and f["tail64"] == 1 and f["energy_blocks"] == 5, f
    if size == "C":
        assert f["nn"] == 129 and f["tiles128"] == 2 and f["tail128"] == 1 and f["tiles128"] % 8 != 0, f
        if "ng" in f:
            assert f["g_tail64"] != 0 and f["g_tail128"] != 0, f
    if size == "D":
        assert f["nn"] == 257 and f["energy_passes"] == 2 and f["energy_tail"] == 1 and f["tiles64"] == 5 and f["tail64"] == 1, f


def system_terms(orc, w, z, charge=0, spin=1, task="omol"):
    """(sysemb, the floor of its own double arithmetic, refsum, sum|refs|): sysemb = SiLU(mix_csd [charge | spin | dataset] + bias) in
    double on both sides, in different orders: (terms + 2) 2^-53 sum|terms|, SiLU' <= 1.1"""
    p = orc.p
    parts = [orc.charge_spin_embedding("charge", charge), orc.charge_spin_embedding("spin", spin)]
    if "dataset_embedding.weight" in p:
        parts.append(p["dataset_embedding.weight"][orc.dataset_list.index(task)])
    v = torch.cat(parts)
    floor = 1.1 * (len(v) + 3) * E53 * (p["mix_csd.weight"].abs() @ v.abs() + p["mix_csd.bias"].abs())
    refs = np.asarray(w["element_refs"], np.float64)[np.asarray(z)]
    return orc.system_embedding(charge, spin, task), floor, float(refs.sum()), float(np.abs(refs).sum())


def _run(eng, pos32, names):
    e, _ = eng.energy_forces(pos32, forces=True)
    return e, {n: eng.debug_fetch(n) for n in names}


CASES = [(ff, acc, size, "bf16x3") for ff in ("spectral", "grid") for acc in ("f64", "f32") for size in ("A", "B", "C", "D")] + [("spectral", "f64", "B", "fp32")]


@pytest.mark.parametrize("ff,acc,size,mode", CASES, ids=["-".join(c) for c in CASES])
def test_node_links_against_float64(ff, acc, size, mode, monkeypatch):
    """Measured on the MI355X (profiles/node_links.txt has every link and case; the 17 cases take 0.2 - 2.1 s each):
    * k_host on the captured arguments: SiLU <= 4.1 u, sigmoid <= 2.7 u, SiLU' <= 11.3 u of the term
    * float64-carried links (norms, A_PLAIN GEMMs and SO(3) linears of the default body, k_grid_contract, k_energy_node): 0.54 ... 0.9999 of
      u |ref64| + floor -- one rounding; the float32-accumulated restatement of the same link: 7 ... 1e6 of the same bound (e_node of 3 atoms: 1.5)
    * fp32-MFMA bodies: <= 0.08 of kappa("fp32", K) sum|terms|, statistic <= 0.57 t24(K)
    * k_norm_bwd <= 0.03 (k 152), gates 0.2 ... 0.5, k_silu_bwd and k_grid_expand <= 0.73; E: the float64 replay's bits
    * mutations, smallest over B and C in units of the bound: bias on l = 1 6.0e4, z = 4 / z = 3 9.3e4 / 9.1e4, lost residual 7.1e4, repeated row
      4.4e5, no centring 1.0e10, swapped balances 1.6e4, to_grid <-> from_grid 1.6e8 / 2.9e9, SiLU for SiLU' 2.6e6, float32 accumulation 1.1e5
      (so3_linear) / 4.6e4 (k_grid_contract)"""
    from pdb2reaction_amd import synth, weights as Wt
    from pdb2reaction_amd.engine import Engine

    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    natoms, nimg = SIZES[size]
    w = Wt.make_synthetic_weights(0, **FF[ff])
    z, imgs, _ = synth.make_images(natoms, nimg, seed=7)
    pos32 = imgs.astype(np.float32)
    orc = O.Oracle(w)
    sysemb, sys_floor, refsum, refs_abs = system_terms(orc, w, z)
    if acc == "f32":
        monkeypatch.setenv("UMX_NODE_F64", "0")
        monkeypatch.setenv("UMX_GRID_F64", "0")
    names = capture_names(ff)
    eng = Engine(0, precision=mode)
    try:
        eng.load_weights(w)
        eng.set_system(z)
        eng.debug_keep(True)
        e, cap = _run(eng, pos32, names)
        row_ptr = eng.debug_fetch("row_ptr", np.int32)
        single = _run(eng, pos32[0], names)[1] if nimg > 1 else None
    finally:
        eng.close()
    nn = natoms * nimg
    assert len(row_ptr) == nn + 1 and cap["xf"].size == nn * ROW, "the batch did not run as one chunk"
    G = int(np.asarray(w["so3_grid.to_grid_mat"]).shape[0]) if ff == "grid" else 0
    facts = size_facts(natoms, nimg, G)
    check_size(size, facts)
    if G:
        assert cap["gridin.0"].size == nn * G * C
    tag = f"{ff} {acc} {size} {mode}"
    print(f"\n  [{tag}] {facts}")
    if single is not None:      # image 0 of the batch has the bits of the same image evaluated alone, at every node capture
        for n in names:
            k = single[n].size
            assert np.array_equal(cap[n][:k].view(np.uint32), single[n].view(np.uint32)), f"{n}: image 0 of the batch differs from the image alone"
    layers = tuple(range(NL))
    rep, kept, _ = replay_case(lambda n, dt=np.float32: cap[n], orc.p, ff, acc, natoms, nimg, tag, sysemb, sys_floor, float(np.float32(w["normalizer.rmsd"][0])),
                               refsum, refs_abs, e, layers, keep=size in ("B", "C"))
    assert not rep.failures, rep.failures
    if kept:
        res = mutation_checks(kept, ff, acc, nn)
        for name, r in res.items():
            print(f"  [{tag}] mutation {name}: {r:.3g} x the bound")
        assert len(res) == N_MUTATIONS[(ff, acc)] and all(r > 1.0 for r in res.values()), res
