"""The checker of tests/test_gpu_node_links.py on the CPU (no GPU): numpy / torch restatements of every node link -- float32 where the kernel
works in float32, float64 rounded once where it carries the row in double -- on random inputs at the four sizes pass its bounds, all nine
host-side mutations are rejected, the plain formulas of the checker are the oracle's, and the size preconditions hold."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import escn_md_oracle as O
from oracle import staged as ST
from pdb2reaction_amd import synth, weights as Wt

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_node_links as NLK  # noqa: E402

C, H, NL = NLK.C, NLK.H, NLK.NL
F32, T64 = torch.float32, torch.float64
L_LP = NLK.L_LP
ONE = np.float32(1.0)


def _sig32(x):
    with np.errstate(over="ignore"):
        return torch.from_numpy(ONE / (ONE + np.exp(-x.numpy())))


def _silu32(x):
    with np.errstate(over="ignore"):
        return torch.from_numpy(x.numpy() / (ONE + np.exp(-x.numpy())))


def _dsilu32(x):
    s = _sig32(x)
    return s * (1.0 + x * (1.0 - s))


def _once(t):
    return t.to(F32)


def _gemm(a, wm, bias, resid, acc):
    """float64 rounded once | float32 throughout"""
    dt = T64 if acc == "f64" else F32
    out = a.to(dt) @ wm.to(dt).T
    for e in (bias, resid):
        if e is not None:
            out = out + e.to(dt)
    return out.to(F32)


def _so3(a, wl, bias, resid, acc, transpose=False):
    dt = T64 if acc == "f64" else F32
    out = torch.einsum("nmo,moi->nmi" if transpose else "nmi,moi->nmo", a.to(dt), wl[L_LP].to(dt))
    if bias is not None:
        out[:, 0] += bias.to(dt)
    if resid is not None:
        out = out + resid.to(dt)
    return out.to(F32)


def _norm_fwd(x, aw, ab, sysemb=None):
    y = O.rms_norm_sh(x.to(T64), aw, ab)
    if sysemb is not None:
        y = torch.cat([y[:, 0:1] + sysemb[None, None], y[:, 1:]], dim=1)
    return _once(y)


def _norm_bwd32(gy, x, aw, gres):
    """the float32 restatement: oracle/staged.py's norm_bwd on float32 tensors"""
    out = ST.norm_bwd(gy, x, aw.to(F32))
    return out if gres is None else out + gres


def restate(w, ff, acc, natoms, nimg, seed):
    """What the engine's node captures of one evaluation would hold if every node kernel were a plain restatement of its link.  The tensors
    that come from the edge side (x0, xmid.i, g_xn.i) and the gradient that enters each layer from above are random."""
    rng = np.random.default_rng(seed)
    orc = O.Oracle(w)
    p = orc.p
    nn = natoms * nimg
    r32 = lambda *s, scale=1.0: torch.from_numpy((rng.standard_normal(s) * scale * np.exp2(rng.uniform(-6, 0, size=s))).astype(np.float32))     # noqa: E731
    z = rng.integers(1, 9, size=natoms)
    sysemb, sys_floor, refsum, refs_abs = NLK.system_terms(orc, w, z)
    cap = {}
    x_in = r32(nn, 9, C)
    cap["x0"] = x_in
    tg, fg = (p["so3_grid.to_grid_mat"], p["so3_grid.from_grid_mat"]) if ff == "grid" else (None, None)
    for i in range(NL):
        b, pa = f"blocks.{i}", f"blocks.{i}.atom_wise"
        cap[f"xn.{i}"] = _norm_fwd(x_in, p[f"{b}.norm_1.affine_weight"], p[f"{b}.norm_1.affine_bias"], sysemb)
        xmid = r32(nn, 9, C)
        xn2 = _norm_fwd(xmid, p[f"{b}.norm_2.affine_weight"], p[f"{b}.norm_2.affine_bias"])
        cap[f"xmid.{i}"], cap[f"xn2.{i}"] = xmid, xn2
        if ff == "grid":
            G = tg.shape[0]
            ng = nn * G
            w1, w2, w3 = (p[f"{pa}.grid_mlp.{li}.weight"] for li in (0, 2, 4))
            b1, b2, b3 = (p.get(f"{pa}.grid_mlp.{li}.bias") for li in (0, 2, 4))
            gridin = torch.einsum("gi,nic->ngc", tg.to(F32), xn2)
            ffg1 = _gemm(gridin.reshape(ng, C), w1, b1, None, acc)
            ffg2 = _gemm(_silu32(ffg1), w2, b2, None, acc)
            gridout = _gemm(_silu32(ffg2), w3, b3, None, acc).reshape(nn, G, C)
            x = _once(xmid.to(T64) + torch.einsum("gi,ngc->nic", fg, gridout.to(T64)))
            cap.update({f"gridin.{i}": gridin, f"ffg1.{i}": ffg1, f"ffg2.{i}": ffg2, f"gridout.{i}": gridout})
        else:
            smlp, l1w, l2w = p[f"{pa}.scalar_mlp.weight"], p[f"{pa}.so3_linear_1.weight"], p[f"{pa}.so3_linear_2.weight"]
            gspre = _gemm(xn2[:, 0], smlp, p[f"{pa}.scalar_mlp.bias"], None, acc)
            ffh = _so3(xn2, l1w, p[f"{pa}.so3_linear_1.bias"], None, acc)
            sp = _sig32(_silu32(gspre)).reshape(nn, 2, H)[:, L_LP[1:] - 1]
            ffhg = torch.cat([_silu32(ffh[:, 0:1]), ffh[:, 1:] * sp], dim=1)
            x = _so3(ffhg, l2w, p[f"{pa}.so3_linear_2.bias"], xmid, acc)
            cap.update({f"gspre.{i}": gspre, f"ffh.{i}": ffh, f"ffhg.{i}": ffhg})
        cap[f"x.{i}"] = x
        x_in = x
    # readout and its reverse head
    xf = _norm_fwd(x_in, p["norm.affine_weight"], p["norm.affine_bias"])
    e0, e2, e4 = p["energy_block.0.weight"], p["energy_block.2.weight"], p["energy_block.4.weight"]
    pre1 = _gemm(xf[:, 0], e0, p["energy_block.0.bias"], None, acc)
    pre2 = _gemm(_silu32(pre1), e2, p["energy_block.2.bias"], None, acc)
    e_node = _once(NLK.silu(pre2.to(T64)) @ e4.reshape(-1) + p["energy_block.4.bias"].reshape(()))
    rmsd = float(np.float32(w["normalizer.rmsd"][0]))
    energies = (rmsd * e_node.to(T64).reshape(nimg, natoms).sum(1) + refsum).numpy()
    g_pre2 = e4.to(F32).expand(nn, H) * _dsilu32(pre2)
    g_sil1 = _gemm(g_pre2, e2.T, None, None, acc)
    g_pre1 = g_sil1 * _dsilu32(pre1)
    g_xf = torch.zeros(nn, 9, C, dtype=F32)
    g_xf[:, 0] = _gemm(g_pre1, e0.T, None, None, acc)
    g_out = _norm_bwd32(g_xf, x_in, p["norm.affine_weight"], None)
    cap.update(xf=xf, pre1=pre1, pre2=pre2, e_node=e_node, g_pre2=g_pre2, g_sil1=g_sil1, g_pre1=g_pre1, g_xf=g_xf, g_xfinal=g_out)
    for i in reversed(range(NL)):
        b, pa = f"blocks.{i}", f"blocks.{i}.atom_wise"
        xmid, x_prev = cap[f"xmid.{i}"], cap[f"x.{i - 1}" if i else "x0"]
        if ff == "grid":
            G = tg.shape[0]
            ng = nn * G
            w1, w2, w3 = (p[f"{pa}.grid_mlp.{li}.weight"] for li in (0, 2, 4))
            g_go = torch.einsum("gi,nic->ngc", fg.to(F32), g_out)
            g_s2 = _gemm(g_go.reshape(ng, C), w3.T, None, None, acc)
            g_f2 = g_s2 * _dsilu32(cap[f"ffg2.{i}"])
            g_s1 = _gemm(g_f2, w2.T, None, None, acc)
            g_f1 = g_s1 * _dsilu32(cap[f"ffg1.{i}"])
            g_gi = _gemm(g_f1, w1.T, None, None, acc).reshape(nn, G, C)
            g_xn2 = _once(torch.einsum("gi,ngc->nic", tg, g_gi.to(T64)))
            cap.update({f"g_gridout.{i}": g_go, f"g_gsil2.{i}": g_s2, f"g_ffg2.{i}": g_f2, f"g_gsil1.{i}": g_s1, f"g_ffg1.{i}": g_f1, f"g_gridin.{i}": g_gi})
        else:
            smlp, l1w, l2w = p[f"{pa}.scalar_mlp.weight"], p[f"{pa}.so3_linear_1.weight"], p[f"{pa}.so3_linear_2.weight"]
            ffh, gspre = cap[f"ffh.{i}"], cap[f"gspre.{i}"]
            g_ffhg = _so3(g_out, l2w, None, None, acc, transpose=True)
            s = _sig32(_silu32(gspre))
            sp = s.reshape(nn, 2, H)[:, L_LP[1:] - 1]
            g_ffh = torch.cat([g_ffhg[:, 0:1] * _dsilu32(ffh[:, 0:1]), g_ffhg[:, 1:] * sp], dim=1)
            pr = g_ffhg[:, 1:] * ffh[:, 1:]
            a = torch.stack([pr[:, 0:3].sum(1), pr[:, 3:8].sum(1)], dim=1).reshape(nn, 2 * H)
            g_gs = a * s * (1.0 - s) * _dsilu32(gspre)
            g_xn2a = _so3(g_ffh, l1w, None, None, acc, transpose=True)
            g_xn2 = g_xn2a.clone()
            g_xn2[:, 0] = _gemm(g_gs, smlp.T, None, g_xn2a[:, 0], acc)
            cap.update({f"g_ffhg.{i}": g_ffhg, f"g_ffh.{i}": g_ffh, f"g_gs.{i}": g_gs, f"g_xn2a.{i}": g_xn2a})
        g_xmid = _norm_bwd32(g_xn2, xmid, p[f"{b}.norm_2.affine_weight"], g_out)
        g_xn = r32(nn, 9, C)
        g_xin = _norm_bwd32(g_xn, x_prev, p[f"{b}.norm_1.affine_weight"], g_xmid)
        cap.update({f"g_xn2.{i}": g_xn2, f"g_xmid.{i}": g_xmid, f"g_xn.{i}": g_xn, f"g_xin.{i}": g_xin})
        g_out = g_xin
    cap = {k: np.ascontiguousarray(v.numpy(), np.float32).reshape(-1) for k, v in cap.items()}
    return cap, p, energies, (sysemb, sys_floor, rmsd, refsum, refs_abs)


_W = {}


def _weights(ff):
    if ff not in _W:
        _W[ff] = Wt.make_synthetic_weights(0, **NLK.FF[ff])
    return _W[ff]


@pytest.mark.parametrize("acc", ["f64", "f32"])
@pytest.mark.parametrize("ff", ["spectral", "grid"])
def test_restatements_pass_and_mutations_are_rejected(ff, acc):
    torch.manual_seed(0)
    w = _weights(ff)
    for size, (natoms, nimg) in NLK.SIZES.items():
        cap, p, energies, (sysemb, sys_floor, rmsd, refsum, refs_abs) = restate(w, ff, acc, natoms, nimg, seed=natoms)
        assert set(NLK.capture_names(ff)) <= set(cap)
        tag = f"cpu {ff} {acc} {size}"
        print()
        rep, kept, _ = NLK.replay_case(lambda n, dt=np.float32: cap[n], p, ff, acc, natoms, nimg, tag, sysemb, sys_floor, rmsd, refsum, refs_abs, energies,
                                       keep=size in ("B", "C"))
        assert not rep.failures, rep.failures
        assert all(r <= 1.0 for r, _, _ in rep.rows.values())
        if acc == "f64":       # "rounded once" is no empty phrase: the float32-accumulated restatement of every such link misses its bound
            assert rep.alt and all(a > 1.0 for a in rep.alt.values()), {k: a for k, a in rep.alt.items() if a <= 1.0}
        if kept:
            res = NLK.mutation_checks(kept, ff, acc, natoms * nimg)
            print(res)
            assert len(res) == NLK.N_MUTATIONS[(ff, acc)] and all(r > 1.0 for r in res.values()), res


def test_plain_formulas_are_the_oracle_s():
    """the checker's own float64 formulas against oracle.rms_norm_sh and oracle/staged.py (norm_bwd, atomwise_fwd / atomwise_bwd, silu_grad)"""
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=T64)      # noqa: E731
    n = 5
    x, gy, gres = rnd(n, 9, C), rnd(n, 9, C), rnd(n, 9, C)
    for ff in ("spectral", "grid"):
        p = O.Oracle(_weights(ff)).p
        aw, ab = p["blocks.1.norm_2.affine_weight"], p["blocks.1.norm_2.affine_bias"]
        assert torch.allclose(NLK.link_norm_fwd(x, aw, ab).ref, O.rms_norm_sh(x, aw, ab), rtol=1e-13, atol=1e-15)
        assert torch.allclose(NLK.link_norm_bwd(gy, x, aw, gres).ref, ST.norm_bwd(gy, x, aw) + gres, rtol=1e-12, atol=1e-14)
        assert torch.allclose(NLK.dsilu(x), ST.silu_grad(x), rtol=1e-14, atol=0)
        pa = "blocks.1.atom_wise"
        xn2 = O.rms_norm_sh(x, aw, ab)
        o2, saved = ST.atomwise_fwd(p, pa, xn2)
        g_ref = ST.atomwise_bwd(p, pa, gy, saved)
        kh = dict(gs_silu=1.0, gs_sigmoid=1.0, gs_silu_grad=1.0, h0_silu=1.0, h0_silu_grad=1.0)
        if ff == "grid":
            tg, fg = p["so3_grid.to_grid_mat"], p["so3_grid.from_grid_mat"]
            G = tg.shape[0]
            w1, w2, w3 = (p[f"{pa}.grid_mlp.{li}.weight"] for li in (0, 2, 4))
            b1, b2, b3 = (p.get(f"{pa}.grid_mlp.{li}.bias") for li in (0, 2, 4))
            g1 = NLK.link_gemm(NLK.link_grid_expand(xn2, tg).ref.reshape(n * G, C), w1, b1).ref
            g2 = NLK.link_gemm(g1, w2, b2, k_silu=1.0).ref
            g3 = NLK.link_gemm(g2, w3, b3, k_silu=1.0).ref.reshape(n, G, C)
            assert torch.allclose(NLK.link_grid_contract(g3, fg).ref, o2, rtol=1e-12, atol=1e-14)
            assert torch.allclose(g1.reshape(n, G, H), saved["ffg1"], rtol=1e-12, atol=1e-14) and torch.allclose(g2.reshape(n, G, H), saved["ffg2"], rtol=1e-12, atol=1e-14)
            t = NLK.link_gemm(NLK.link_grid_expand(gy, fg).ref.reshape(n * G, C), w3.T).ref
            t = NLK.link_gemm(NLK.link_silu_bwd(t, g2, 1.0).ref, w2.T).ref
            t = NLK.link_gemm(NLK.link_silu_bwd(t, g1, 1.0).ref, w1.T).ref.reshape(n, G, C)
            assert torch.allclose(NLK.link_grid_contract(t, tg).ref, g_ref, rtol=1e-11, atol=1e-13)
        else:
            smlp, l1w, l2w = p[f"{pa}.scalar_mlp.weight"], p[f"{pa}.so3_linear_1.weight"], p[f"{pa}.so3_linear_2.weight"]
            gspre = NLK.link_gemm(xn2[:, 0], smlp, p[f"{pa}.scalar_mlp.bias"]).ref
            ffh = NLK.link_so3(xn2, l1w, p[f"{pa}.so3_linear_1.bias"]).ref
            ffhg = NLK.link_gate_fwd(ffh, gspre, kh).ref
            assert torch.allclose(gspre, saved["gspre"], rtol=1e-12, atol=1e-14) and torch.allclose(ffh, saved["ffh"], rtol=1e-12, atol=1e-14)
            assert torch.allclose(ffhg, saved["ffhg"], rtol=1e-12, atol=1e-14)
            assert torch.allclose(NLK.link_so3(ffhg, l2w, p[f"{pa}.so3_linear_2.bias"], x).ref, x + o2, rtol=1e-12, atol=1e-14)
            g_ffhg = NLK.link_so3(gy, l2w, transpose=True).ref
            L_gh, L_gs = NLK.link_gate_bwd(g_ffhg, ffh, gspre, kh)
            g_a = NLK.link_so3(L_gh.ref, l1w, transpose=True).ref
            g0 = NLK.link_gemm(L_gs.ref, smlp.T, resid=g_a[:, 0]).ref
            assert torch.allclose(torch.cat([g0[:, None], g_a[:, 1:]], dim=1), g_ref, rtol=1e-11, atol=1e-13)


def test_sizes_meet_their_preconditions():
    G = int(np.asarray(_weights("grid")["so3_grid.to_grid_mat"]).shape[0])
    for size, (natoms, nimg) in NLK.SIZES.items():
        z, imgs, _ = synth.make_images(natoms, nimg, seed=7)
        src, dst = O.radius_graph(torch.as_tensor(imgs[0].astype(np.float32).astype(np.float64)), NLK.OT.CUTOFF, None)
        assert imgs.shape == (nimg, natoms, 3) and len(src) > 0
        NLK.check_size(size, NLK.size_facts(natoms, nimg))
        NLK.check_size(size, NLK.size_facts(natoms, nimg, G))
