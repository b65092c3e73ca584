"""The HBM-bound edge kernels between the GEMMs, link by link, against float64 -- at the edge counts and degrees where they change shape.

tests/test_gpu_mfma_model.py and tests/test_gpu_reverse_links.py pin the GEMMs but take their operands (y1q, hidq, gmsgq / gmsgpl, ghgq /
ghgpl, gradq / gradpl) from the engine's captures as given.  Here every kernel that WRITES such an operand (and the node sums, the torque /
dE/dd accumulators and the force assembly) is replayed on the CPU in float64 from the engine's OWN captured inputs and compared with the
engine's captured output element by element.  No oracle forward pass is run.  The float64 formulas are the oracle's (edge_rotation,
wigner_m_primary, envelope, gate_m_primary, staged.torque, silu_grad; the radial row of each m-primary row and the [src | dst] halves as
oracle/staged.py spells them) or are written plainly below; none is transcribed from a kernel.

    frame                 evec                                            -> frame (R, D2, env, denv)          k_edge_geom
    rotate + modulate     xn.i, src, dst, frame, rad.i                    -> y1q.i  | xrot.i (fp32)            k_gather_rotate_mod_q3<3> | k_gather_rotate
    gate                  hg.i                                            -> hidq.i | hid.i                    k_gate_edge_fwd_q3<3> | k_gate_edge_fwd
    rotate back + sum     msg.i | rad.deg, frame, row_ptr, x.(i-1) | x0   -> xmid.i, x0                        k_rotate_back_reduce<9>, <3>
    rotate back^T         g_xmid.i, msg.i, frame, dst                     -> gmsgq.i | gmsgpl.i | g_msg.i      k_rotate_back_bwd_q3<3> | _pl<2> | <9>
    rotate back^T (deg)   g_xin.0, rad.deg, frame, dst                    -> gradpl.deg (3 | 2 planes)         k_rotate_back_bwd<3,3> | <3,2>
    gate^T                g_hid.i, hg.i                                   -> ghgq.i | ghgpl.i | g_hg.i         k_gate_edge_bwd_q3<3> | _pl<2> | k_gate_edge_bwd
    modulate^T, rotate^T  g_y1.i, xn.i, frame, rad.i, row_ptr, out_ptr,   -> gradq.i | gradpl.i | g_rad.i,     k_modrot_bwd_pl<0> | <2> | k_modulate_bwd +
                          out_edge                                           g_xn.i (g_xrot.i in fp32)         k_gather_rotate_bwd
    accumulators          every rotate back^T and modulate^T link of ALL  -> tau (tau + tau2), dedd - dedd_rad k_add4, the += of the kernels above
                          four layers + the edge-degree link
    force assembly        dedd, tau, frame, evec; gvec, CSR lists         -> gvec; forces                      k_force_edge, k_force_node

Modes: bf16x3 (float32 quad-row operands, the fused k_modrot_bwd_pl<0> that production runs in every mode), split-bf16 (the same forward
kernels: its reverse links only, two PL planes), fp32 (the plain row kernels; with captures on its reverse pass is the unfused one).  The
fast mode's fp16 forward operands (k_*_q3<1>) are held by tests/test_gpu_forward_links.py, with the links of this file.

Sizes (preconditions asserted from the captured row_ptr / out_ptr / ne): S = 40 atoms, 1142 edges; L = 700 atoms, 44404 edges, layers 0 and
3 only; T1 = 17 atoms with max_neigh 3 (51 edges, two nodes without out-edges) and T2 = 13 atoms with max_neigh 5 (65 edges): truncated
graphs, the only way to an odd ne and to in- and out-lists of different lengths.  The accumulators are replayed as TOTALS at every size, L
included: UMX_DEBUG_ONLY is read at every capture, so the evaluation is repeated once per layer with that layer's names only (the engine is
deterministic) and the contributions are reduced layer by layer; the engine holds ~2.7 GB of captures during a full-layer pass at L.

Bounds, per element, nothing relative to a tensor's maximum, no element excluded (u = 2^-24, gamma_k = k u / (1 - k u)):
  * arithmetic links: |out - ref64| <= gamma_k * sum|terms| + u |ref64|, sum|terms| = the same formula on absolute values, k = the float32
    roundings on the longest path, derived beside each link below;
  * frame: u |ref64| + a floor of a few 2^-52 of the formula's magnitude (the kernel works in double and rounds once);
  * links through expf: (k_arith + 2 k_host) u |term|, k_host = the distance of the SAME formula in numpy float32, operation by operation,
    from float64 on the captured hg values, in u of the term (measured at run time, printed);
  * bf16 plane outputs: + 2^(-8 P) |ref64|.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import escn_md_oracle as O
from oracle import tables as OT
from oracle.staged import silu_grad, torque

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_reverse_links import _planes, _sign, _unblock  # noqa: E402

pytestmark = pytest.mark.gpu

C, H, NL = OT.SPHERE_CHANNELS, OT.HIDDEN_CHANNELS, OT.NUM_LAYERS
ROW, HG, XROT, RAD, FRAME = 9 * C, 2 * H + 9 * H, 9 * 2 * C, 6 * 2 * C, 36
U = 2.0 ** -24
T64 = torch.float64
SIZES = {"T1": (17, 3), "T2": (13, 5), "S": (40, None), "L": (700, None)}          # atoms, max_neigh
LINK_LAYERS = {"T1": (0, 1, 2, 3), "T2": (0, 1, 2, 3), "S": (0, 1, 2, 3), "L": (0, 3)}
CHUNK = 4096                                                                       # edges per float64 replay slice
L_MP = torch.tensor(OT.L_OF_MP)


def gamma(k):
    return k * U / (1.0 - k * U)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(T64)


# ---- the torque generators as matrices, read off oracle.staged.torque by probing it with unit vectors: tau_k = sum_rc L_k[r, c] <g_r, a_c>
def _generators():
    L = torch.zeros(3, 9, 9, dtype=T64)
    for r in range(9):
        for c in range(9):
            g, a = torch.zeros(1, 9, 1, dtype=T64), torch.zeros(1, 9, 1, dtype=T64)
            g[0, r, 0] = a[0, c, 0] = 1.0
            L[:, r, c] = torque(g, a)[0]
    return L


GEN = _generators()


def tq(L, g, a):
    return torch.einsum("krc,erh,ech->ek", L, g, a)


def radx(rad):
    """(E, 1536) radial weights -> the factor of each m-primary row (E, 9, 2C): m0 rows one block each, the +m / -m rows share theirs
    (oracle so2_conv / staged.backward)"""
    c2 = 2 * C
    m1, m2 = rad[:, 3 * c2: 5 * c2].reshape(-1, 2, c2), rad[:, 5 * c2:].reshape(-1, 1, c2)
    return torch.cat([rad[:, : 3 * c2].reshape(-1, 3, c2), m1, m1, m2, m2], dim=1)


def rad_fold(gx):
    e = gx.shape[0]
    return torch.cat([gx[:, 0:3].reshape(e, -1), (gx[:, 3:5] + gx[:, 5:7]).reshape(e, -1), (gx[:, 7:8] + gx[:, 8:9]).reshape(e, -1)], dim=1)


class Graph:
    """the captured graph, frames and edge vectors; W_e (m-primary rows x l-primary columns) is assembled from the captured R and D2 with
    the oracle's row order TO_M"""

    def __init__(self, get, nn):
        self.nn = nn
        self.src = torch.from_numpy(get("src", np.int32).astype(np.int64))
        self.dst = torch.from_numpy(get("dst", np.int32).astype(np.int64))
        self.ne = len(self.src)
        self.row_ptr = get("row_ptr", np.int32).astype(np.int64)
        self.out_ptr = get("out_ptr", np.int32).astype(np.int64)
        self.out_edge = get("out_edge", np.int32).astype(np.int64)
        self.frame = get("frame").reshape(self.ne, FRAME)
        self.evec = get("evec").reshape(self.ne, 4)
        self.indeg, self.outdeg = np.diff(self.row_ptr), np.diff(self.out_ptr)
        # the two CSR lists say what src / dst say
        assert self.row_ptr[0] == 0 and self.row_ptr[-1] == self.ne and self.out_ptr[0] == 0 and self.out_ptr[-1] == self.ne
        assert np.array_equal(np.repeat(np.arange(nn), self.indeg), self.dst.numpy())
        assert np.array_equal(self.src.numpy()[self.out_edge], np.repeat(np.arange(nn), self.outdeg))
        assert np.array_equal(np.sort(self.out_edge), np.arange(self.ne))

    def slices(self):
        return [slice(a, min(a + CHUNK, self.ne)) for a in range(0, self.ne, CHUNK)]

    def wig(self, sl):
        f = _t(self.frame[sl])
        e = f.shape[0]
        lp = torch.zeros(e, 9, 9, dtype=T64)
        lp[:, 0, 0] = 1.0
        lp[:, 1:4, 1:4] = f[:, 0:9].reshape(e, 3, 3)
        lp[:, 4:9, 4:9] = f[:, 9:34].reshape(e, 5, 5)
        return lp[:, list(OT.TO_M), :]

    def env(self, sl):
        return _t(self.frame[sl, 34])[:, None, None]

    def denv(self, sl):
        return _t(self.frame[sl, 35])


# ---- the links: each returns (ref64, bound) for a slice of edges (or for all nodes) -------------------------------------------------------
def link_frame(evec, cutoff=OT.CUTOFF):
    """k_edge_geom: double arithmetic on the float32 unit vector, ONE rounding per entry -> u |ref| + a floor for the double arithmetic:
    16 (R, env, denv) / 64 (D2: 9 x 9 products of R entries) x 2^-52 x the largest intermediate (|1 - k nx^2| <= 3 with k = 1 / (1 + ny) <=
    10 behind the flip, so D2 terms <= 9 x 3 = 27 ... 30; the envelope's coefficients sum to 72, denv's to 420 / cutoff)"""
    v = _t(evec)
    rm = O.edge_rotation(v[:, :3])
    _, d2 = O.wigner_blocks(rm)
    u = v[:, 3] / cutoff
    env = O.envelope(u)
    denv = torch.where(u < 1.0, (-105.0 * u ** 4 + 210.0 * u ** 5 - 105.0 * u ** 6) / cutoff, torch.zeros_like(u))
    e = v.shape[0]
    ref = torch.cat([rm.reshape(e, 9), d2.reshape(e, 25), env[:, None], denv[:, None]], dim=1)
    eps = 2.0 ** -52
    floor = torch.cat([torch.full((e, 9), 16 * eps * 3.0), torch.full((e, 25), 64 * eps * 30.0), torch.full((e, 1), 16 * eps * 72.0),
                       torch.full((e, 1), 16 * eps * 420.0 / cutoff)], dim=1).to(T64)
    return ref, U * ref.abs() + floor


K_ROT = 5          # one row of W x: at most a 5-term dot product (the D2 block): 5 products, 4 sums, gamma_5


def link_rotate(Wg, xcat):
    """xrot = W [xn[src] | xn[dst]]: k = 5 (the D2 dot product)"""
    ref = torch.bmm(Wg, xcat)
    return ref, gamma(K_ROT) * torch.bmm(Wg.abs(), xcat.abs()) + U * ref.abs()


def link_rotmod(Wg, xcat, rad):
    """y1 = (W [xn[src] | xn[dst]]) .* radx, stored with the row's sign: k = 5 (dot) + 1 (radial factor) + 1 (sign) = 7"""
    rx = radx(rad)
    ref = torch.bmm(Wg, xcat) * rx
    return ref, gamma(7) * torch.bmm(Wg.abs(), xcat.abs()) * rx.abs() + U * ref.abs()


def host_ulps(x32):
    """k_host of the three expf formulas on these float32 arguments: max |f32 - f64| / (u * term), the float32 form evaluated operation by
    operation in numpy; term = the formula on absolute values: sigmoid s; SiLU |x| s; SiLU' s (1 + |x| (1 - s))"""
    x32 = np.ascontiguousarray(x32, np.float32).reshape(-1)
    one = np.float32(1.0)
    with np.errstate(over="ignore"):
        den = one + np.exp(-x32)
        s32, silu32 = one / den, x32 / den
        g32 = s32 * (one + x32 * (one - s32))
        x = x32.astype(np.float64)
        s = 1.0 / (1.0 + np.exp(-x))
    ax = np.abs(x)
    out = {}
    for name, f32, f64, term in (("sigmoid", s32, s, s), ("silu", silu32, x * s, ax * s), ("silu_grad", g32, s * (1.0 + x * (1.0 - s)), s * (1.0 + ax * (1.0 - s)))):
        live = term > 0
        out[name] = float((np.abs(f32.astype(np.float64) - f64)[live] / (U * term[live])).max()) if live.any() else 0.0
    return out


def link_gate_fwd(hg, kh):
    """hid = gate_m_primary(gate, hpre) with the row's sign.  Row 0: SiLU (k_host) and the sign: k_arith = 1; rows of l > 0: one product with
    the sigmoid (k_host) and the sign: k_arith = 2.  Returns (ref, bound, k of row 0, k of the other rows)."""
    e = hg.shape[0]
    gate, hpre = hg[:, : 2 * H], hg[:, 2 * H:].reshape(e, 9, H)
    ref = O.gate_m_primary(gate, hpre)
    s0 = torch.sigmoid(hpre[:, 0:1])
    sg = torch.sigmoid(gate).reshape(e, OT.LMAX, H)[:, L_MP[1:] - 1]
    k0, k1 = 1 + 2 * kh["silu"], 2 + 2 * kh["sigmoid"]
    bound = torch.cat([k0 * U * hpre[:, 0:1].abs() * s0, k1 * U * hpre[:, 1:].abs() * sg], dim=1)
    return ref, bound, k0, k1


def link_gate_bwd(g_hid, hg, kh):
    """g_hg = [g_gate l1 | g_gate l2 | g_hpre 9 x H] (oracle/staged.py backward), with the row's sign.
    g_hpre row 0 = g SiLU'(hpre): product + sign, k_arith = 2; rows l > 0 = g sigmoid(gate_l): k_arith = 2.
    g_gate_l = a s (1 - s), a = the sum over the rows of degree l of g hpre (<= 5 products: gamma_5 + 1), s = sigmoid to K = 2 k_host u:
    fl(1 - s) - (1 - s64) = -s64 ds + (1 - s) d, so |error| <= sum|g hpre| [ (5 + 1 + 3 + 1) u s (1 - s) + K u s (1 - s) + K u s^2 ]
    = sum|g hpre| s [ 10 u (1 - s) + K u ]   (two products, the subtraction, the sign: 3 + 1)."""
    e = hg.shape[0]
    gate, hpre = hg[:, : 2 * H], hg[:, 2 * H:].reshape(e, 9, H)
    g = g_hid.reshape(e, 9, H)
    sgt = torch.sigmoid(gate)
    sgm = sgt.reshape(e, OT.LMAX, H)[:, L_MP[1:] - 1]
    g_hpre = torch.cat([g[:, 0:1] * silu_grad(hpre[:, 0:1]), g[:, 1:] * sgm], dim=1)
    pr = g[:, 1:] * hpre[:, 1:]
    l1 = L_MP[1:] == 1
    a = torch.stack([pr[:, l1].sum(1), pr[:, ~l1].sum(1)], dim=1).reshape(e, 2 * H)
    a_abs = torch.stack([pr[:, l1].abs().sum(1), pr[:, ~l1].abs().sum(1)], dim=1).reshape(e, 2 * H)
    ref = torch.cat([a * sgt * (1 - sgt), g_hpre.reshape(e, -1)], dim=1)
    s0 = torch.sigmoid(hpre[:, 0:1])
    K = 2 * kh["sigmoid"]
    b_gate = a_abs * sgt * (10 * U * (1 - sgt) + K * U)
    b_row0 = (2 + 2 * kh["silu_grad"]) * U * g[:, 0:1].abs() * s0 * (1.0 + hpre[:, 0:1].abs() * (1.0 - s0))
    b_rows = (2 + 2 * kh["sigmoid"]) * U * g[:, 1:].abs() * sgm
    return ref, torch.cat([b_gate, torch.cat([b_row0, b_rows], dim=1).reshape(e, -1)], dim=1)


def link_rotate_back_bwd(Wg, env, g_dst, div=1.0, planes=0):
    """g_msg = (env / div) W g[dst], with the row's sign: k = 5 (dot) + 1 (env) + 1 (sign) = 7, + 1 for the division of the edge-degree
    link; P bf16 planes add 2^(-8 P) |ref|.  Returns (ref, bound, W g, |W| |g|): the last two feed the accumulators."""
    gl = torch.bmm(Wg, g_dst)
    gl_abs = torch.bmm(Wg.abs(), g_dst.abs())
    ref = gl * env / div
    k = 7 if div == 1.0 else 8
    return ref, gamma(k) * gl_abs * env.abs() / div + (U + (2.0 ** (-8 * planes) if planes else 0.0)) * ref.abs(), gl, gl_abs


def link_force_edge(dedd, tau, frame, evec):
    """gvec = dE/dd nhat + R^T (tau_z, 0, -tau_x) / d, the torque dropped where nhat_y is 1 to the oracle's isclose -- replayed as the SAME
    float32 comparison on the captured evec, so no edge is ambiguous.  k = 1 (1 / d) + 2 (two products, one sum) + 1 (x 1/d) + 1 (g n) + 1
    (sum) = 6.  Returns (ref, bound, the pole mask, the torque term alone)."""
    ny = np.ascontiguousarray(evec[:, 1], np.float32)
    pole = torch.from_numpy(np.abs(ny - np.float32(1.0)) <= np.float32(np.float32(1e-8) + np.float32(1e-5)))
    v, f = _t(evec), _t(frame)
    rm = f[:, 0:9].reshape(-1, 3, 3)
    tloc = torch.stack([tau[:, 2], torch.zeros_like(tau[:, 0]), -tau[:, 0]], dim=1)
    tterm = torch.bmm(rm.transpose(1, 2), tloc[:, :, None])[:, :, 0] / v[:, 3:4]
    tabs = torch.bmm(rm.abs().transpose(1, 2), tloc.abs()[:, :, None])[:, :, 0] / v[:, 3:4]
    keep = (~pole)[:, None].to(T64)
    ref = dedd[:, None] * v[:, :3] + tterm * keep
    return ref, gamma(6) * ((dedd[:, None] * v[:, :3]).abs() + tabs * keep) + U * ref.abs(), pole, tterm


def link_force_node(gvec, G, rmsd):
    """F[n] = -rmsd (sum over out-edges of gvec - sum over in-edges): a lane adds every 64th entry of each list (ceil(d_in / 64) + ceil(d_out
    / 64) sums), a 6-level wave sum, the product with float32 rmsd: k = trips + 6 + 2 per node"""
    z = torch.zeros(G.nn, 3, dtype=T64)
    ref = -rmsd * (z.index_add(0, G.src, gvec) - z.index_add(0, G.dst, gvec))
    terms = rmsd * (z.index_add(0, G.src, gvec.abs()) + z.index_add(0, G.dst, gvec.abs()))
    k = torch.from_numpy((G.indeg + 63) // 64 + (G.outdeg + 63) // 64 + 8).to(T64)[:, None]
    return ref, k * U / (1.0 - k * U) * terms + U * ref.abs(), int(k.max())


# accumulators.  One contribution to dE/dd: the dot product (5), the product with msg (1), 18 sums per lane (9 rows x 2 channels), a 6-level
# wave sum, the envelope derivative and the division (2): 32; over the 5 links 5 float32 += and the final sum with dedd_rad: K_DEDD = 38.
# One contribution to tau: g_msg or g_xrot (6 or 1), the rotated operand (5), their product (1), the generator's expression (<= 8 terms, the
# float32 sqrt(3) and its product: 10), two channels (2), a 6-level wave sum: <= 30; 9 += over the links and k_add4: K_TAU = 40.
K_DEDD, K_TAU = 38, 40


def ratio(out, ref, bound):
    """(largest |out - ref| / bound, number of elements over their bound); where the bound is 0 the output must equal the reference"""
    err = (out - ref).abs()
    live = bound > 0
    bad = int((err[live] > bound[live]).sum()) + int((err[~live] != 0).sum())
    r = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
    return (np.inf if int((err[~live] != 0).sum()) else r), bad


class Report:
    def __init__(self, tag):
        self.tag, self.rows, self.failures = tag, {}, []

    def add(self, name, k, out, ref, bound):
        r, bad = ratio(out, ref, bound)
        r0, k0, b0 = self.rows.get(name, (0.0, k, 0))
        self.rows[name] = (max(r0, r), max(k0, k), b0 + bad)
        return r

    def close(self, extra=None):
        for name, (r, k, bad) in self.rows.items():
            note = (extra or {}).get(name, "")
            print(f"  [{self.tag}] {name:28s} k {k:6.1f}: max |err| / bound {r:.3e}{note}")
            if bad:
                self.failures.append((name, f"{bad} elements over the bound, worst {r:.3e}"))


def _rows(get, mode, i, ne, q, pl, plain, cols, P=2):
    """one captured operand as float64 rows [ne, cols], un-negated with the engine's rule"""
    if mode == "bf16x3":
        return _t(_unblock(get(f"{q}.{i}"), cols)[:ne].astype(np.float64) * _sign(ne))
    if mode == "split-bf16":
        return _t(_planes(get(f"{pl}.{i}").view(np.uint16), ne, cols, P) * _sign(ne))
    return _t(get(f"{plain}.{i}").reshape(ne, cols))


def pass_names(i, full):
    base = ["row_ptr", "src", "dst", "out_ptr", "out_edge", "evec", "frame", "tau", "dedd", "gvec", "x0", "rad.deg", "gradpl.deg", "g_xin.0"]
    per = ["g_xmid", "msg", "g_y1", "xn", "rad"]
    if full:
        per += ["hg", "xmid", "g_hid", "g_xn", "y1q", "hidq", "gmsgq", "gmsgpl", "ghgq", "ghgpl", "gradq", "gradpl", "xrot", "hid", "g_msg", "g_hg",
                "g_xrot", "g_rad"]
        base += [f"x.{i - 1}"] if i > 0 else []
    return base + [f"{n}.{i}" for n in per]


def replay_case(mode, tag, passes, nn, link_layers, base0, rmsd, forces, keep_for_mutations=False):
    """Replay every link of one evaluation.  passes(i, full) -> get(name, dtype=np.float32): the captures of an evaluation that kept
    pass_names(i, full).  base0 [nn, C] float64: the l = 0 row of the node initialisation (element embedding + system embedding).
    forces() -> the forces of that evaluation.  Returns (Report, Graph, kept): kept = what the mutation checks need (small systems only)."""
    rep = Report(tag)
    fwd = mode != "split-bf16"
    pl, q = mode != "fp32", mode == "bf16x3"
    P = {"bf16x3": 3, "split-bf16": 2, "fp32": 0}[mode]
    G, kept, khs = None, {}, {}
    tau_ref = tau_abs = tau2_ref = dedd_ref = dedd_abs = None
    for i in range(NL):
        full = i in link_layers
        get = passes(i, full)
        if G is None:
            G = Graph(get, nn)
            ne = G.ne
            tau_ref, tau_abs, tau2_ref = (torch.zeros(ne, 3, dtype=T64) for _ in range(3))
            dedd_ref, dedd_abs = torch.zeros(ne, dtype=T64), torch.zeros(ne, dtype=T64)
            ref, bound = link_frame(G.evec)
            rep.add("frame", 1, _t(G.frame), ref, bound)
            if keep_for_mutations:
                kept["frame"] = (_t(G.frame), ref, bound)
        xn, g_xmid = _t(get(f"xn.{i}")).reshape(nn, 9, C), _t(get(f"g_xmid.{i}")).reshape(nn, 9, C)
        msg32, gy32, rad32 = get(f"msg.{i}").reshape(ne, 9, C), get(f"g_y1.{i}").reshape(ne, 9, 2 * C), get(f"rad.{i}").reshape(ne, RAD)
        if full:
            hg32 = get(f"hg.{i}").reshape(ne, HG)
            kh = host_ulps(hg32)
            khs[i] = kh
            g_hid32 = get(f"g_hid.{i}").reshape(ne, ROW)
            if fwd:
                y1 = _rows(get, mode, i, ne, "y1q", None, "xrot", XROT).reshape(ne, 9, 2 * C)
                hid = _rows(get, mode, i, ne, "hidq", None, "hid", ROW).reshape(ne, 9, H)
            g_msg = _rows(get, mode, i, ne, "gmsgq", "gmsgpl", "g_msg", ROW).reshape(ne, 9, C)
            g_hg = _rows(get, mode, i, ne, "ghgq", "ghgpl", "g_hg", HG)
            if mode == "bf16x3":
                g_rad = _t(get(f"gradq.{i}").reshape(ne, RAD).astype(np.float64) * _sign(ne))
            else:
                g_rad = _rows(get, mode, i, ne, None, "gradpl", "g_rad", RAD)
            g_xrot = _t(get(f"g_xrot.{i}")).reshape(ne, 9, 2 * C) if mode == "fp32" else None
            xsum, xabs = torch.zeros(nn, 9, C, dtype=T64), torch.zeros(nn, 9, C, dtype=T64)
            gxn, gxn_abs = torch.zeros(nn, 9, C, dtype=T64), torch.zeros(nn, 9, C, dtype=T64)
        for sl in G.slices():
            Wg, env, denv = G.wig(sl), G.env(sl), G.denv(sl)
            src, dst = G.src[sl], G.dst[sl]
            msg, gy, rad = _t(msg32[sl]), _t(gy32[sl]), _t(rad32[sl])
            xcat = torch.cat([xn[src], xn[dst]], dim=2)
            # ---- rotate back^T: g_msg and its contributions to dE/dd and the torque
            ref, bound, gl, gl_abs = link_rotate_back_bwd(Wg, env, g_xmid[dst], 1.0, 0 if mode != "split-bf16" else 2)
            dedd_ref[sl] += denv * (gl * msg).sum(dim=(1, 2))
            dedd_abs[sl] += denv.abs() * (gl_abs * msg.abs()).sum(dim=(1, 2))
            tau_ref[sl] -= tq(GEN, gl * env, msg)
            tau_abs[sl] += tq(GEN.abs(), gl_abs * env.abs(), msg.abs())
            # ---- modulate^T + rotate^T: contributions to the torque (target half -> tau, source half -> tau2)
            xr, xr_abs, rx = torch.bmm(Wg, xcat), torch.bmm(Wg.abs(), xcat.abs()), radx(rad)
            gxr = gy * rx
            t_all, t_dst = tq(GEN, gxr, xr), tq(GEN, gxr[:, :, C:], xr[:, :, C:])
            tau_ref[sl] += t_all
            tau2_ref[sl] += t_all - t_dst
            tau_abs[sl] += tq(GEN.abs(), gxr.abs(), xr_abs)
            if not full:
                continue
            rep.add(f"L{i} rotate back^T g_msg", 7, g_msg[sl], ref, bound)
            if keep_for_mutations and i == link_layers[0]:
                kept["g_msg"] = (g_msg[sl], ref, bound)
            # ---- forward links
            if fwd:
                if mode == "fp32":
                    ref, bound = link_rotate(Wg, xcat)
                    rep.add(f"L{i} rotate xrot", K_ROT, y1[sl], ref, bound)
                else:
                    ref, bound = link_rotmod(Wg, xcat, rad)
                    rep.add(f"L{i} rotate+modulate y1q", 7, y1[sl], ref, bound)
                    if keep_for_mutations and i == link_layers[0]:
                        kept["y1q"] = (y1[sl], ref, bound)
                ref, bound, k0, k1 = link_gate_fwd(_t(hg32[sl]), kh)
                rep.add(f"L{i} gate hid row 0", k0, hid[sl][:, 0:1], ref[:, 0:1], bound[:, 0:1])
                rep.add(f"L{i} gate hid rows l>0", k1, hid[sl][:, 1:], ref[:, 1:], bound[:, 1:])
                if keep_for_mutations and i == link_layers[0]:
                    kept["hid"] = (hid[sl], ref, bound)
                # rotate back + sum: the float32 part is W^T msg (k = 5); the scale and the sum over the edges are carried in double
                t = torch.bmm(Wg.transpose(1, 2), msg) * env
                xsum.index_add_(0, dst, t)
                xabs.index_add_(0, dst, torch.bmm(Wg.abs().transpose(1, 2), msg.abs()) * env.abs())
            # ---- gate^T
            ref, bound = link_gate_bwd(_t(g_hid32[sl]), _t(hg32[sl]), kh)
            if mode == "split-bf16":
                bound = bound + 2.0 ** -16 * ref.abs()
            rep.add(f"L{i} gate^T g_gate", 10 + 2 * kh["sigmoid"], g_hg[sl][:, : 2 * H], ref[:, : 2 * H], bound[:, : 2 * H])
            rep.add(f"L{i} gate^T g_hpre row 0", 2 + 2 * kh["silu_grad"], g_hg[sl][:, 2 * H: 3 * H], ref[:, 2 * H: 3 * H], bound[:, 2 * H: 3 * H])
            rep.add(f"L{i} gate^T g_hpre rows l>0", 2 + 2 * kh["sigmoid"], g_hg[sl][:, 3 * H:], ref[:, 3 * H:], bound[:, 3 * H:])
            # ---- modulate^T: g_rad[k] = the sum over the (<= 2) rows of radial block k of g_y1 (W x): k = 5 + 1 + 2 + 1 (sign) = 9
            ref = rad_fold(gy * xr)
            bound = gamma(9) * rad_fold(gy.abs() * xr_abs) + (U + (2.0 ** -16 if mode == "split-bf16" else 0.0)) * ref.abs()
            rep.add(f"L{i} modulate^T g_rad", 9, g_rad[sl], ref, bound)
            if g_xrot is not None:        # fp32 with captures on: the unfused kernels expose g_xrot = g_y1 .* radx (k = 1)
                rep.add(f"L{i} modulate^T g_xrot", 1, g_xrot[sl], gxr, gamma(1) * gxr.abs())
            # ---- rotate^T: g_xn[n] = the sum over in(n) of W^T g_xrot[:, target half] + over out(n) of W^T g_xrot[:, source half]
            gb, gb_abs = torch.bmm(Wg.transpose(1, 2), gxr), torch.bmm(Wg.abs().transpose(1, 2), gxr.abs())
            gxn.index_add_(0, src, gb[:, :, :C]).index_add_(0, dst, gb[:, :, C:])
            gxn_abs.index_add_(0, src, gb_abs[:, :, :C]).index_add_(0, dst, gb_abs[:, :, C:])
        if not full:
            continue
        # g_xn: the modulation (1), the scale (1), the dot product (5): 7; one float32 sum per edge of the two lists (d); the three sums that
        # join the four waves' partials: k = 7 + d + 3 per node
        kn = torch.from_numpy(G.indeg + G.outdeg + 10).to(T64)[:, None, None]
        bound = kn * U / (1.0 - kn * U) * gxn_abs + U * gxn.abs()
        g_xn_out = _t(get(f"g_xn.{i}")).reshape(nn, 9, C)
        rep.add(f"L{i} rotate^T g_xn", float(kn.max()), g_xn_out, gxn, bound)
        if keep_for_mutations and i == link_layers[0]:
            kept["g_xn"] = (g_xn_out, gxn, bound, _t(gy32), _t(rad32))
        if fwd:
            # xmid = x_in + the sum: gamma_5 on the float32 part, the final rounding, 2^-50 for the double arithmetic
            xin = _t(get(f"x.{i - 1}" if i else "x0")).reshape(nn, 9, C)
            ref = xin + xsum
            bound = gamma(K_ROT) * xabs + U * ref.abs() + 2.0 ** -50 * (xabs + xin.abs())
            rep.add(f"L{i} rotate back + sum xmid", K_ROT + 1, _t(get(f"xmid.{i}")).reshape(nn, 9, C), ref, bound)
        if i == 0:
            rad_deg = _t(get("rad.deg")).reshape(ne, 3, C)
            g_x0 = _t(get("g_xin.0")).reshape(nn, 9, C)
            emb = torch.cat([rad_deg, torch.zeros(ne, 6, C, dtype=T64)], dim=1)
            x0sum, x0abs = torch.zeros(nn, 9, C, dtype=T64), torch.zeros(nn, 9, C, dtype=T64)
            if pl:
                g_deg = _t(_planes(get("gradpl.deg").view(np.uint16)[: ne * 3 * C * P], ne, 3 * C, P) * _sign(ne)).reshape(ne, 3, C)
            for sl in G.slices():
                Wg, env, denv, dst = G.wig(sl), G.env(sl), G.denv(sl), G.dst[sl]
                ref, bound, gl, gl_abs = link_rotate_back_bwd(Wg, env, g_x0[dst], OT.DEG_RESCALE, P)
                if pl:
                    rep.add("deg rotate back^T g_rad.deg", 8, g_deg[sl], ref[:, 0:3], bound[:, 0:3])
                dedd_ref[sl] += denv * (gl * emb[sl]).sum(dim=(1, 2)) / OT.DEG_RESCALE
                dedd_abs[sl] += denv.abs() * (gl_abs * emb[sl].abs()).sum(dim=(1, 2)) / OT.DEG_RESCALE
                tau_ref[sl] -= tq(GEN, ref, emb[sl])
                tau_abs[sl] += tq(GEN.abs(), gl_abs * env.abs() / OT.DEG_RESCALE, emb[sl].abs())
                x0sum.index_add_(0, dst, torch.bmm(Wg.transpose(1, 2), emb[sl]) * env / OT.DEG_RESCALE)
                x0abs.index_add_(0, dst, torch.bmm(Wg.abs().transpose(1, 2), emb[sl].abs()) * env.abs() / OT.DEG_RESCALE)
            if fwd:
                base = torch.zeros(nn, 9, C, dtype=T64)
                base[:, 0] = base0
                ref = base + x0sum
                rep.add("deg rotate back + sum x0", K_ROT + 1, _t(get("x0")).reshape(nn, 9, C), ref,
                        gamma(K_ROT) * x0abs + U * ref.abs() + 2.0 ** -50 * (x0abs + base.abs()))
            # the totals and the force assembly come from this pass too (every pass captures the same final values)
            tau_out, dedd_out = _t(get("tau")).reshape(ne, 4)[:, :3], _t(get("dedd"))
            dedd_rad, gvec_out = _t(get("dedd_rad.deg")), _t(get("gvec")).reshape(ne, 4)
    # ---- accumulators: totals over all four layers and the edge-degree link
    b_tau = gamma(K_TAU) * tau_abs + U * tau_ref.abs()
    rep.add("total tau (tau + tau2)", K_TAU, tau_out, tau_ref, b_tau)
    b_dedd = gamma(K_DEDD) * dedd_abs + U * dedd_ref.abs() + U * dedd_out.abs()        # dedd_out = fl(dedd + dedd_rad): one more rounding
    rep.add("total dedd - dedd_rad", K_DEDD, dedd_out - dedd_rad, dedd_ref, b_dedd)
    ref, bound, pole, tterm = link_force_edge(dedd_out, tau_out, G.frame, G.evec)
    rep.add("force edge gvec", 6, gvec_out[:, :3], ref, bound)
    assert not gvec_out[:, 3].any()
    fref, fbound, kf = link_force_node(gvec_out[:, :3], G, rmsd)
    rep.add("force node F", kf, _t(forces()).reshape(nn, 3), fref, fbound)
    if keep_for_mutations:
        kept["tau"] = (tau_out, tau_ref, b_tau, tau2_ref)
        kept["gvec"] = (gvec_out[:, :3], ref, bound, pole, tterm)
    notes = {}
    if khs:
        ks = {n: max(k[n] for k in khs.values()) for n in ("sigmoid", "silu", "silu_grad")}
        print(f"  [{tag}] k_host on the captured hg: sigmoid {ks['sigmoid']:.2f} u, SiLU {ks['silu']:.2f} u, SiLU' {ks['silu_grad']:.2f} u")
        for name, (r, k, bad) in rep.rows.items():
            if "gate" in name:
                notes[name] = f"  (device: {r * k:.2f} u of the term)"
    rep.close(notes)
    return rep, G, kept


# ---- the checker must be able to fail: host-side mutations of captured outputs ------------------------------------------------------------
def mutation_checks(G, kept, mode="bf16x3"):
    """Each mutation of a captured output must be rejected (largest |err| / bound > 1).  Returns the ratios."""
    out = {}
    ne = G.ne
    rej = lambda o, ref, bound: ratio(o, ref, bound)[0]     # noqa: E731
    # (1) y1q: the src and dst column halves of one m-primary row of one edge swapped
    y1, ref, bound = kept["y1q"]
    m = y1.clone()
    m[ne // 2, 4] = torch.cat([y1[ne // 2, 4, C:], y1[ne // 2, 4, :C]])
    out["1 src / dst halves swapped"] = rej(m, ref, bound)
    # (2) the last valid row of the last row group replaced by the row of edge e0 of that group (a wrong `valid` handling)
    e0 = (ne - 1) // 4 * 4
    if e0 != ne - 1:
        m = y1.clone()
        m[ne - 1] = y1[e0] * (1.0 if (ne - 1 - e0) % 2 == 0 else -1.0)      # stored with e0's sign, read back with the row's own
        out["2 tail row = row of e0"] = rej(m, ref, bound)
    else:                        # ne % 4 == 1: e0 IS the last valid row; the row before the group then stands in for it
        m = y1.clone()
        m[ne - 1] = -y1[ne - 2]
        out["2 tail row = row of e0"] = rej(m, ref, bound)
    # (3) g_xn without the last incoming edge of a node with in-degree % 4 == 1 (the one the 1st wave takes alone)
    cand = np.nonzero(G.indeg % 4 == 1)[0]
    if len(cand):                # (T1 has in-degree 3 everywhere: the callers require this mutation at the other sizes)
        g_xn, ref, bound, gy, rad = kept["g_xn"]
        n = int(cand[0])
        e = int(G.row_ptr[n + 1] - 1)
        drop = torch.bmm(G.wig(slice(e, e + 1)).transpose(1, 2), (gy[e:e + 1] * radx(rad[e:e + 1]))[:, :, C:])[0]
        m = g_xn.clone()
        m[n] -= drop
        out["3 last in-edge of a 4k+1 node dropped"] = rej(m, ref, bound)
    # (4) one odd row of hidq multiplied by -1
    hid, ref, bound = kept["hid"]
    m = hid.clone()
    m[1] = -m[1]
    out["4 odd row of hidq negated"] = rej(m, ref, bound)
    # (5) tau without the tau2 half (the source halves of every modulate^T link)
    tau, ref, bound, tau2_part = kept["tau"]
    out["5 tau without tau2"] = rej(tau - tau2_part, ref, bound)
    # (6) gvec of one pole-masked edge shifted by its unmasked torque term; without such an edge, the mask applied where it must not be
    gvec, ref, bound, pole, tterm = kept["gvec"]
    m = gvec.clone()
    if bool(pole.any()):
        cands = torch.nonzero(pole)[:, 0]
        e = int(cands[tterm[cands].abs().sum(1).argmax()])
        m[e] += tterm[e]
    else:
        e = int(tterm.abs().sum(1).argmax())
        m[e] -= tterm[e]
    out["6 pole mask on the wrong side"] = rej(m, ref, bound)
    # (7) one element that is small against its tensor (< 1e-4 of the largest) scaled by 1 + 2^-16: a max-norm check passes it
    for name in ("y1q", "g_msg"):
        o, ref, bound = kept[name]
        big = float(ref.abs().max())
        small = (ref.abs() < 1e-4 * big) & (ref.abs() > 1e-7 * big)
        assert bool(small.any()), name
        # the element whose bound is tightest against its value: the one a per-element check is most sure about
        score = torch.where(small, ref.abs() / bound, torch.zeros_like(ref))
        idx = np.unravel_index(int(score.argmax()), tuple(ref.shape))
        m = o.clone()
        m[idx] = m[idx] * (1.0 + 2.0 ** -16)
        old = float((m - ref).abs().max()) / big                 # what the stage test's max-norm check looks at
        out[f"7 small element of {name} x (1 + 2^-16)"] = rej(m, ref, bound)
        assert old <= 2e-5, (name, old)
    return out


# ---- coverage preconditions ---------------------------------------------------------------------------------------------------------------
def graph_facts(ne, indeg, outdeg, ny):
    return dict(ne=int(ne), ne4=int(ne % 4), ne8=int(ne % 8), groups8=int((ne + 3) // 4 % 8), deg_4k1=int((indeg % 4 == 1).sum()),
                deg_lt4=int(((indeg < 4) | (outdeg < 4)).sum()), empty_out=int((outdeg == 0).sum()), in_ne_out=int((indeg != outdeg).sum()),
                in_gt64=int((indeg > 64).sum()), in_lt64=int((indeg < 64).sum()), flipped=int((ny < np.float32(-0.9)).sum()))


def check_preconditions(facts):
    """facts: {size: graph_facts}.  Every shape change of the table in DESIGN.md section 3 is met by some size."""
    assert {f["ne4"] for f in facts.values()} == {0, 1, 2, 3}, facts
    assert any(1 <= f["ne8"] <= 4 for f in facts.values()) and any(5 <= f["ne8"] <= 7 for f in facts.values()), facts
    assert any(f["deg_4k1"] for f in facts.values()) and any(f["deg_lt4"] for f in facts.values()), facts
    assert any(f["empty_out"] for f in facts.values()) and any(f["in_ne_out"] for f in facts.values()), facts
    assert any(f["flipped"] for f in facts.values()), facts
    if "L" in facts:
        assert facts["L"]["in_gt64"] and facts["L"]["in_lt64"], facts["L"]
        assert facts["L"]["groups8"] != 0, facts["L"]                  # the XCD map has empty virtual blocks


_FACTS = {}


def _engine_passes(eng, pos32, monkeypatch, state):
    def passes(i, full):
        monkeypatch.setenv("UMX_DEBUG_ONLY", ",".join(pass_names(i, full)))
        _, f = eng.energy_forces(pos32, forces=True)
        if "forces" in state:
            assert np.array_equal(state["forces"], f), "the evaluation is not deterministic"
        state["forces"] = f
        return lambda name, dtype=np.float32: eng.debug_fetch(name, dtype)
    return passes


@pytest.mark.parametrize("size", ["T1", "T2", "S", "L"])
@pytest.mark.parametrize("mode", ["bf16x3", "fp32", "split-bf16"])
def test_edge_links_against_float64(mode, size, monkeypatch):
    """Measured on the MI355X (largest |err| / bound over T1, T2, S and L and the replayed layers; the 12 cases take 165 s):
    * k_host on the captured hg (numpy float32 against float64): sigmoid <= 3.6 u, SiLU <= 3.8 u, SiLU' <= 4.3 u of the term; the device, in
      u of the term: gate rows 2.6 (SiLU) / 3.1 (sigmoid), gate^T g_hpre 4.5 (row 0) / 3.1, g_gate 5.6 (8.1 with two planes) -- against
      bounds of k = 9 ... 17 u: the device's expf formulas lie as close to float64 as the host's
    * bf16x3: frame 1.00 (one rounding, the bound is exact); y1q 0.56 (k 7), hidq 0.35 / 0.39, x0 0.85 and xmid 0.75 (k 6), gmsgq 0.60 (k 7),
      gradpl.deg 0.44 (k 8), ghgq 0.33 / 0.42 / 0.37, gradq 0.44 (k 9), g_xn 0.21 (k = 10 + d, up to 200), gvec 0.46 (k 6), F 0.15 (k <= 12);
      total tau 2.5e-3 ... 6.7e-3 (k 40), total dedd - dedd_rad 7.4e-3 ... 4.7e-2 (k 38): the two accumulators sit lowest, their sum|terms|
      runs over 9 x 256 channels of nine links -- mutation 5 (tau without tau2) still lands 9.9e3 x above the bound
    * fp32 (row kernels, unfused reverse): xrot 0.70 (k 5), g_xrot 1.00 (k 1: exact), g_msg 0.58, g_rad 0.45, g_xn 0.23, the rest as bf16x3
    * split-bf16 (two planes, + 2^-16 |ref|): gmsgpl 0.50, ghgpl 0.48 / 0.49 / 0.49, gradpl 0.49, gradpl.deg 0.49, g_xn 0.20
    * mutations (bf16x3; smallest over T1, T2, S, in units of the bound): halves swapped 1.5e8, tail row 2.2e8, dropped edge 2.3e4, negated
      row 4.2e6, tau without tau2 9.9e3, pole mask 1.1e6, small element x (1 + 2^-16) 32 (y1q) and 8.7 (g_msg)
    * graph facts: T1 51 edges (in-degree 3, two empty out-lists, 4 flipped frames), T2 65 (in-degree 5), S 1142 (9 nodes of degree 4k + 1,
      60 flipped), L 44404 (319 nodes above and 371 below in-degree 64, 11101 row groups = 5 mod 8, 2070 flipped)"""
    from pdb2reaction_amd import synth, weights as Wt
    from pdb2reaction_amd.engine import Engine

    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    n_atoms, max_neigh = SIZES[size]
    w = Wt.make_synthetic_weights(0)
    z, pos = synth.make_cluster(n_atoms)
    orc = O.Oracle(w)
    base0 = orc.p["sphere_embedding.weight"][torch.as_tensor(np.asarray(z), dtype=torch.long)] + orc.system_embedding(0, 1, "omol")[None]
    eng = Engine(0, precision=mode)
    state = {}
    try:
        eng.load_weights(w)
        eng.set_system(z, max_neigh=max_neigh)
        eng.debug_keep(True)
        passes = _engine_passes(eng, pos.astype(np.float32), monkeypatch, state)
        tag = f"{mode} {size}"
        print()
        rep, G, kept = replay_case(mode, tag, passes, n_atoms, LINK_LAYERS[size], base0, float(np.float32(w["normalizer.rmsd"][0])),
                                   lambda: state["forces"], keep_for_mutations=(mode == "bf16x3" and size != "L"))
    finally:
        eng.close()
    facts = graph_facts(G.ne, G.indeg, G.outdeg, G.evec[:, 1])
    print(f"  [{tag}] {facts}")
    _FACTS[size] = facts
    expect = {"T1": (51, 3, 3), "T2": (65, 1, 1), "S": (1142, 2, 6), "L": (44404, 0, 4)}[size]
    assert (facts["ne"], facts["ne4"], facts["ne8"]) == expect, facts
    if size == "T1":
        assert facts["empty_out"] >= 1 and facts["in_ne_out"] and facts["deg_lt4"]
    if size == "T2":
        assert facts["deg_4k1"] and facts["in_ne_out"]
    if size == "S":
        assert facts["deg_4k1"] and facts["flipped"]
    if size == "L":
        assert facts["in_gt64"] and facts["in_lt64"] and facts["groups8"] != 0 and facts["flipped"]
    if len(_FACTS) == 4:
        check_preconditions(_FACTS)
    assert not rep.failures, rep.failures
    if kept:
        res = mutation_checks(G, kept)
        for name, r in res.items():
            print(f"  [{tag}] mutation {name}: {r:.3g} x the bound")
        assert all(r > 1.0 for r in res.values()) and len(res) == (7 if size == "T1" else 8), res

