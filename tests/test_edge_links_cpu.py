"""The checker of tests/test_gpu_edge_links.py on the CPU (no GPU): float32 restatements of every link on random inputs pass its bounds, the
seven host-side mutations are rejected, and the two truncated systems meet their preconditions on the oracle's graph."""
import os
import sys

import numpy as np
import torch

from oracle import escn_md_oracle as O
from oracle import tables as OT
from pdb2reaction_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_edge_links as EL  # noqa: E402

C, H, NL = EL.C, EL.H, EL.NL
F32 = torch.float32


def _graph(n_atoms, max_neigh, pole_edge=False):
    z, pos = synth.make_cluster(n_atoms)
    p32 = pos.astype(np.float32)
    if pole_edge:                      # atom 1 straight above atom 0: one edge exactly along +y, its reverse along -y
        p32[1] = p32[0] + np.array([0.0, 1.5, 0.0], np.float32)
    p = torch.as_tensor(p32.astype(np.float64))
    src, dst = O.radius_graph(p, OT.CUTOFF, max_neigh)
    return z, p, src.numpy(), dst.numpy()


def _block(x, cols):
    rows = (x.shape[0] + 3) // 4 * 4
    pad = np.zeros((rows, cols), np.float32)
    pad[: x.shape[0]] = x
    return pad.reshape(rows // 4, 4, cols // 16, 16).transpose(0, 2, 1, 3).reshape(-1).copy()


def _to_planes(x, P):
    """float32 [ne, cols] -> P round-to-nearest-even bf16 planes in the PL layout (per row and 32 columns: P planes of 32)"""
    ne, cols = x.shape
    rest = x.astype(np.float32).copy()
    out = np.zeros((ne, cols // 32, P, 32), np.uint16)
    for q in range(P):
        bits = rest.view(np.uint32).astype(np.uint64)
        hi = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)
        out[:, :, q, :] = hi.reshape(ne, cols // 32, 32)
        rest = rest - (hi.astype(np.uint32) << 16).view(np.float32)
    return out.reshape(-1)


def synthetic_captures(n_atoms, max_neigh, seed=0, pole_edge=False):
    """What the engine's bf16x3 captures of one evaluation would hold if every edge kernel were a plain float32 restatement of its link
    (the GEMM outputs between them are random: the links are checked one by one from their own inputs)"""
    rng = np.random.default_rng(seed)
    z, p, src, dst = _graph(n_atoms, max_neigh, pole_edge)
    nn, ne = n_atoms, len(src)
    vec = (p[src] - p[dst]).numpy()
    d = np.linalg.norm(vec, axis=1)
    evec = np.concatenate([vec / d[:, None], d[:, None]], axis=1).astype(np.float32)
    frame = EL.link_frame(evec)[0].numpy().astype(np.float32)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=nn))]).astype(np.int32)
    out_edge = np.argsort(src, kind="stable").astype(np.int32)
    out_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=nn))]).astype(np.int32)
    cap = dict(src=src.astype(np.int32), dst=dst.astype(np.int32), row_ptr=row_ptr, out_ptr=out_ptr, out_edge=out_edge, evec=evec.reshape(-1),
               frame=frame.reshape(-1))
    G = EL.Graph(lambda n, dt=np.float32: cap[n], nn)
    Wg = G.wig(slice(0, ne)).to(F32)
    env, denv = G.env(slice(0, ne)).to(F32), G.denv(slice(0, ne)).to(F32)
    tsrc, tdst = torch.from_numpy(src), torch.from_numpy(dst)
    sign = torch.from_numpy(EL._sign(ne)).to(F32)
    gen = EL.GEN.to(F32)
    r32 = lambda *s, scale=1.0: torch.from_numpy((rng.standard_normal(s) * scale * np.exp2(rng.uniform(-6, 0, size=s))).astype(np.float32))     # noqa: E731
    tau, dedd = torch.zeros(ne, 3, dtype=F32), torch.zeros(ne, dtype=F32)
    # the node initialisation + the edge-degree embedding: x0, the input of layer 0
    rad_deg, base0 = r32(ne, 3, C), r32(nn, C)
    emb = torch.cat([rad_deg, torch.zeros(ne, 6, C, dtype=F32)], dim=1)
    t = torch.bmm(Wg.transpose(1, 2), emb).double() * env.double() / OT.DEG_RESCALE
    x0 = torch.zeros(nn, 9, C, dtype=torch.float64).index_add_(0, tdst, t)
    x0[:, 0] += base0.double()
    x_prev = x0.to(F32)
    cap["x0"], cap["rad.deg"] = x_prev, rad_deg
    for i in range(NL):
        xn, rad, hg, msg = r32(nn, 9, C), r32(ne, EL.RAD), r32(ne, EL.HG, scale=3.0), r32(ne, 9, C)
        g_xmid, g_hid, g_y1 = r32(nn, 9, C), r32(ne, 9, H), r32(ne, 9, 2 * C)
        xcat = torch.cat([xn[tsrc], xn[tdst]], dim=2)
        xr = torch.bmm(Wg, xcat)
        y1 = xr * EL.radx(rad)
        gate, hpre = hg[:, : 2 * H], hg[:, 2 * H:].reshape(ne, 9, H)
        hid = O.gate_m_primary(gate, hpre)
        xin = x_prev
        t = torch.bmm(Wg.transpose(1, 2), msg).double() * env.double()
        xmid = (xin.double() + torch.zeros(nn, 9, C, dtype=torch.float64).index_add_(0, tdst, t)).to(F32)
        gl = torch.bmm(Wg, g_xmid[tdst])
        g_msg = gl * env
        dedd += denv * (gl * msg).sum(dim=(1, 2))
        tau -= EL.tq(gen, g_msg, msg)
        sgt = torch.sigmoid(gate)
        sgm = sgt.reshape(ne, 2, H)[:, EL.L_MP[1:] - 1]
        s0 = torch.sigmoid(hpre[:, 0:1])
        g_hpre = torch.cat([g_hid[:, 0:1] * (s0 * (1.0 + hpre[:, 0:1] * (1.0 - s0))), g_hid[:, 1:] * sgm], dim=1)
        pr = g_hid[:, 1:] * hpre[:, 1:]
        l1 = EL.L_MP[1:] == 1
        a = torch.stack([pr[:, l1].sum(1), pr[:, ~l1].sum(1)], dim=1).reshape(ne, 2 * H)
        g_hg = torch.cat([a * sgt * (1.0 - sgt), g_hpre.reshape(ne, -1)], dim=1)
        g_rad = EL.rad_fold(g_y1 * xr)
        gxr = g_y1 * EL.radx(rad)
        tau += EL.tq(gen, gxr, xr)
        gb = torch.bmm(Wg.transpose(1, 2), gxr)
        g_xn = torch.zeros(nn, 9, C, dtype=F32).index_add_(0, tsrc, gb[:, :, :C]).index_add_(0, tdst, gb[:, :, C:])
        x_prev = r32(nn, 9, C)
        cap.update({f"xn.{i}": xn, f"rad.{i}": rad, f"hg.{i}": hg, f"msg.{i}": msg, f"g_xmid.{i}": g_xmid, f"g_hid.{i}": g_hid, f"g_y1.{i}": g_y1,
                    f"xmid.{i}": xmid, f"g_xn.{i}": g_xn, f"x.{i}": x_prev, f"gradq.{i}": g_rad * sign,
                    f"y1q.{i}": _block((y1.reshape(ne, -1) * sign).numpy(), EL.XROT), f"hidq.{i}": _block((hid.reshape(ne, -1) * sign).numpy(), EL.ROW),
                    f"gmsgq.{i}": _block((g_msg.reshape(ne, -1) * sign).numpy(), EL.ROW), f"ghgq.{i}": _block((g_hg * sign).numpy(), EL.HG)})
    # the edge-degree link of the reverse pass
    g_x0 = r32(nn, 9, C)
    gl = torch.bmm(Wg, g_x0[tdst])
    g_emb = gl * (env / np.float32(OT.DEG_RESCALE))
    dedd += denv / np.float32(OT.DEG_RESCALE) * (gl * emb).sum(dim=(1, 2))
    tau -= EL.tq(gen, g_emb, emb)
    cap["g_xin.0"] = g_x0
    cap["gradpl.deg"] = _to_planes((g_emb[:, 0:3].reshape(ne, -1) * sign).numpy(), 3)
    dedd_rad = r32(ne)
    g = dedd + dedd_rad
    pole = torch.from_numpy(np.abs(evec[:, 1] - np.float32(1.0)) <= np.float32(np.float32(1e-8) + np.float32(1e-5)))
    tloc = torch.stack([tau[:, 2], torch.zeros(ne), -tau[:, 0]], dim=1) * (~pole)[:, None]
    rm = torch.from_numpy(frame[:, :9]).reshape(ne, 3, 3)
    ev = torch.from_numpy(evec)
    gvec = g[:, None] * ev[:, :3] + torch.bmm(rm.transpose(1, 2), tloc[:, :, None])[:, :, 0] * (1.0 / ev[:, 3:4])
    rmsd = np.float32(1.5)
    zf = torch.zeros(nn, 3, dtype=F32)
    forces = -rmsd * (zf.index_add(0, tsrc, gvec) - zf.index_add(0, tdst, gvec))
    cap.update({"tau": torch.cat([tau, torch.zeros(ne, 1)], dim=1), "dedd": g, "dedd_rad.deg": dedd_rad,
                "gvec": torch.cat([gvec, torch.zeros(ne, 1)], dim=1)})
    cap = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in cap.items()}
    cap = {k: (np.ascontiguousarray(v).reshape(-1)) for k, v in cap.items()}
    return cap, base0.double(), float(rmsd), forces.numpy(), bool(pole.any())


def _replay(cap, nn, base0, rmsd, forces):
    get = lambda name, dtype=np.float32: cap[name]       # noqa: E731
    return EL.replay_case("bf16x3", "synthetic", lambda i, full: get, nn, (0, 1, 2, 3), base0, rmsd, lambda: forces, keep_for_mutations=True)


def test_float32_restatements_pass_and_mutations_are_rejected():
    torch.manual_seed(0)
    for n_atoms, max_neigh, pole_edge in ((17, 3, False), (13, 5, True)):
        cap, base0, rmsd, forces, has_pole = synthetic_captures(n_atoms, max_neigh, seed=n_atoms, pole_edge=pole_edge)
        assert has_pole == pole_edge
        rep, G, kept = _replay(cap, n_atoms, base0, rmsd, forces)
        assert not rep.failures, rep.failures
        assert all(r <= 1.0 for r, _, _ in rep.rows.values())
        res = EL.mutation_checks(G, kept)
        print(res)
        assert len(res) == (8 if (G.indeg % 4 == 1).any() else 7) and all(r > 1.0 for r in res.values()), res
        assert bool(kept["gvec"][3].any()) == pole_edge


def test_truncated_systems_meet_their_preconditions():
    facts = {}
    for size in ("T1", "T2", "S"):
        n_atoms, max_neigh = EL.SIZES[size]
        _, p, src, dst = _graph(n_atoms, max_neigh)
        vec = (p[src] - p[dst]).numpy()
        ny = (vec[:, 1] / np.linalg.norm(vec, axis=1)).astype(np.float32)
        facts[size] = EL.graph_facts(len(src), np.bincount(dst, minlength=n_atoms), np.bincount(src, minlength=n_atoms), ny)
    t1, t2 = facts["T1"], facts["T2"]
    assert (t1["ne"], t1["ne4"], t1["ne8"]) == (51, 3, 3) and t1["empty_out"] == 2 and t1["in_ne_out"] and t1["deg_lt4"] == 17, t1
    assert (t2["ne"], t2["ne4"], t2["ne8"]) == (65, 1, 1) and t2["deg_4k1"] == 13 and t2["in_ne_out"], t2
    assert (facts["S"]["ne"], facts["S"]["ne4"], facts["S"]["ne8"]) == (1142, 2, 6) and facts["S"]["flipped"], facts["S"]
    facts["L"] = dict(facts["S"], ne4=0, ne8=4, groups8=5, in_gt64=1, in_lt64=1)        # L's own facts are asserted on the GPU (44404 edges)
    EL.check_preconditions(facts)
