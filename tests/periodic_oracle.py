"""Float64 checker for periodic boundary conditions -- a helper, not a test.

``oracle/escn_md_oracle.Oracle.model_energy`` forms ``vec = pos[src] - pos[dst]`` inline, so the unchanged oracle cannot express a
lattice translation.  This module restates the PROJECT'S OWN oracle with one difference, ``vec = pos[src] + t - pos[dst]``, and adds
the periodic radius graph that supplies ``t``.  tests/test_periodic_cpu.py holds it to the parent oracle (zero translations: bit for
bit) and to the physical invariants of a periodic system.  What fairchem's periodic graph generation returns has not been compared
[3P-UNVERIFIED].
"""
from __future__ import annotations

import itertools
from typing import Optional

import numpy as np
import torch

from oracle import tables as W
from oracle.escn_md_oracle import (C, S, Oracle, atomwise, edge_rotation, envelope, gate_m_primary, radial_mlp, rms_norm_sh, silu,
                                   so2_conv, wigner_m_primary)


def lattice_translations(cell, pbc, cutoff: float):
    """(ints [T,3], plane distances h [3]): every integer combination of the periodic lattice vectors that can bring a source within
    the cutoff of a target when both lie inside the cell -- |n_k| <= floor(cutoff / h_k) + 1 along a periodic axis, 0 along an open
    one -- in lexicographic order of (n_a, n_b, n_c), c running fastest.  The index in this list is the translation index."""
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    pbc = np.broadcast_to(np.asarray(pbc, dtype=bool), (3,))
    h = np.full(3, np.inf)
    if pbc.any():
        dual = np.linalg.pinv(cell[pbc])                 # (3, p): column k is the dual vector of periodic axis k within the periodic span
        h[pbc] = 1.0 / np.linalg.norm(dual, axis=0)
    nmax = [int(np.floor(cutoff / h[k])) + 1 if pbc[k] else 0 for k in range(3)]
    ints = np.array(list(itertools.product(*[range(-n, n + 1) for n in nmax])), dtype=np.int64)
    return ints, h


def wrap_offsets(pos, cell, pbc):
    """Integer lattice offsets n (N,3) such that pos - n @ cell lies inside the cell along the periodic axes (0 along open ones)."""
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    pbc = np.broadcast_to(np.asarray(pbc, dtype=bool), (3,))
    n = np.zeros((len(pos), 3), dtype=np.int64)
    if pbc.any():
        frac = np.asarray(pos, dtype=np.float64) @ np.linalg.pinv(cell[pbc])
        n[:, pbc] = np.floor(frac).astype(np.int64)
    return n


def periodic_radius_graph(pos, cell, pbc, cutoff: float, max_neigh: Optional[int] = None):
    """All (source j, translation t) -> target i with 0 < |r_j + t - r_i| <= cutoff, sorted by (target, source, translation index).

    Returns (src [E], dst [E], t [E,3] float64, tidx [E]).  ``t`` is the translation to add to the positions AS GIVEN (an atom outside
    the cell is wrapped for the search and its lattice offset folded back into ``t``).  ``max_neigh`` keeps the nearest M candidates
    per target over all images; ties as ``oracle.radius_graph`` (a stable argsort of the squared distances), the candidates laid out
    as translation index * N + source.  Brute force over the translations.  No periodic axis: one zero translation, and exactly the
    graph of ``oracle.radius_graph``.
    """
    with torch.no_grad():
        p0 = torch.as_tensor(np.asarray(pos), dtype=torch.float64).detach()
        n = p0.shape[0]
        cell = np.asarray(cell if cell is not None else np.zeros((3, 3)), dtype=np.float64).reshape(3, 3)
        pbc = np.broadcast_to(np.asarray(pbc if pbc is not None else False, dtype=bool), (3,))
        ints, _ = lattice_translations(cell, pbc, cutoff)
        off = wrap_offsets(p0.numpy(), cell, pbc)
        tcell = torch.as_tensor(cell)
        p = p0 - torch.as_tensor(off, dtype=torch.float64) @ tcell if off.any() else p0
        tv = torch.as_tensor(ints, dtype=torch.float64) @ tcell if pbc.any() else torch.zeros(len(ints), 3, dtype=torch.float64)
        zero = int(np.nonzero((ints == 0).all(1))[0][0])
        # d2[i, t, j] = |p_j + t - p_i|^2
        d2 = (((p[None, None, :, :] + tv[None, :, None, :]) - p[:, None, None, :]) ** 2).sum(-1)
        mask = d2 <= cutoff * cutoff
        mask[:, zero, :] &= ~torch.eye(n, dtype=torch.bool)
        mask &= d2 > 0.0
        if max_neigh is not None:
            flat = torch.where(mask, d2, torch.full_like(d2, float("inf"))).reshape(n, -1)       # candidate index = tidx * n + j
            order = torch.argsort(flat, dim=1, stable=True)
            rank = torch.empty_like(order)
            rank.scatter_(1, order, torch.arange(flat.shape[1]).expand(n, flat.shape[1]))
            mask = mask & (rank.reshape(d2.shape) < max_neigh)
        dst, src, tidx = torch.nonzero(mask.permute(0, 2, 1), as_tuple=True)                     # (target, source, translation)
        shift = torch.as_tensor(ints[tidx.numpy()] + off[dst.numpy()] - off[src.numpy()], dtype=torch.float64).reshape(-1, 3) @ tcell \
            if pbc.any() else torch.zeros(len(src), 3, dtype=torch.float64)
    return src, dst, shift, tidx


class PeriodicOracle(Oracle):
    """``Oracle`` with a cell: ``model_energy`` is the parent's, line for line, except ``vec = pos[src] + t - pos[dst]``."""

    def __init__(self, weights, cell=None, pbc=None, **kw):
        super().__init__(weights, **kw)
        self.cell = None if cell is None else np.asarray(cell, dtype=np.float64).reshape(3, 3)
        self.pbc = np.broadcast_to(np.asarray(False if pbc is None else pbc, dtype=bool), (3,))

    def model_energy(self, z, pos, charge=0, spin=1, task="omol", roll=None, graph=None, keep=False):
        p = self.p
        n = pos.shape[0]
        dbg = self.debug if keep else None
        src, dst, shift, tidx = graph if graph is not None else periodic_radius_graph(pos, self.cell, self.pbc, self.cutoff, self.max_neigh)
        vec = pos[src] + shift.to(self.dtype) - pos[dst]
        dist = vec.norm(dim=1)
        nhat = vec / dist[:, None]
        rm = edge_rotation(nhat, roll)
        pole = torch.isclose(nhat[:, 1], torch.ones_like(nhat[:, 1]))
        if bool(pole.any()):
            rm = torch.where(pole[:, None, None], rm.detach(), rm)
        wig = wigner_m_primary(rm)
        wig_inv = wig.transpose(1, 2)
        env = envelope(dist / self.cutoff)
        x_edge = self.edge_scalars(dist, z[src], z[dst])
        sys_emb = self.system_embedding(charge, spin, task)

        x = torch.zeros(n, S, C, dtype=self.dtype)
        x[:, 0, :] = p["sphere_embedding.weight"][z] + sys_emb[None, :]

        rad0 = radial_mlp(p, "edge_degree_embedding.rad_func", x_edge).reshape(-1, 3, C)
        emb = torch.cat([rad0, torch.zeros(len(src), S - 3, C, dtype=self.dtype)], dim=1)
        emb = torch.bmm(wig_inv, emb) * env[:, None, None] / W.DEG_RESCALE
        x = x.index_add(0, dst, emb)
        if dbg is not None:
            dbg.update(src=src, dst=dst, vec=vec, dist=dist, wig=wig, env=env, x0=x, sys_emb=sys_emb, tidx=tidx)

        for i in range(W.NUM_LAYERS):
            b = f"blocks.{i}"
            xn = rms_norm_sh(x, p[f"{b}.norm_1.affine_weight"], p[f"{b}.norm_1.affine_bias"])
            xn = torch.cat([xn[:, 0:1, :] + sys_emb[None, None, :], xn[:, 1:, :]], dim=1)
            msg = torch.cat([xn[src], xn[dst]], dim=2)
            msg = torch.bmm(wig, msg)
            rad = radial_mlp(p, f"{b}.edge_wise.so2_conv_1.rad_func", x_edge)
            hpre, gate = so2_conv(p, f"{b}.edge_wise.so2_conv_1", msg, rad, 2 * C, W.HIDDEN_CHANNELS, W.LMAX * W.HIDDEN_CHANNELS)
            hid = gate_m_primary(gate, hpre)
            out, _ = so2_conv(p, f"{b}.edge_wise.so2_conv_2", hid, None, W.HIDDEN_CHANNELS, C, 0)
            out = torch.bmm(wig_inv, out * env[:, None, None])
            x = x + torch.zeros_like(x).index_add(0, dst, out)
            xn2 = rms_norm_sh(x, p[f"{b}.norm_2.affine_weight"], p[f"{b}.norm_2.affine_bias"])
            x = x + atomwise(p, f"{b}.atom_wise", xn2)

        xf = rms_norm_sh(x, p["norm.affine_weight"], p["norm.affine_bias"])
        h = silu(xf[:, 0, :] @ p["energy_block.0.weight"].T + p["energy_block.0.bias"])
        h = silu(h @ p["energy_block.2.weight"].T + p["energy_block.2.bias"])
        e_node = (h @ p["energy_block.4.weight"].T + p["energy_block.4.bias"]).reshape(-1)
        return e_node.sum()


def commensurate_atoms(cell, grid, seed: int, jitter: float = 0.25, faces=None):
    """Atoms on a jittered lattice commensurate with the cell: grid = (ga, gb, gc) points per lattice vector, each displaced by up to
    ``jitter`` of its grid spacing (fractional), elements from the synthetic distribution.  All positions lie inside the cell, so the
    wrap is the identity.  ``faces = (i, j)``: atom i is moved to the fractional coordinate 0.02 and atom j to 0.98 along a, next to
    opposite faces of the cell -- almost a whole cell apart, which is what brings a translation of two cells along a short axis within
    the cutoff.  Returns (z int32 [N], pos float64 [N,3])."""
    from pdb2reaction_amd import synth

    rng = np.random.default_rng(seed)
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    g = np.array(grid)
    idx = np.stack(np.meshgrid(*[np.arange(k) for k in g], indexing="ij"), axis=-1).reshape(-1, 3)
    frac = (idx + 0.5 + rng.uniform(-jitter, jitter, size=idx.shape)) / g
    z = rng.choice(np.array(synth.ELEMENT_Z, dtype=np.int32), size=len(idx), p=np.array(synth.ELEMENT_P))
    if faces is not None:
        frac[faces[0], 0], frac[faces[1], 0] = 0.02, 0.98
    return z.astype(np.int32), frac @ cell


def assert_clear_of_the_pole_band(vec: np.ndarray, thr: float = 1.001e-5):
    """A condition on INPUTS: no edge direction may have |1 - nhat_y| within a factor 2 of the pole threshold,
    where float32 and float64 could decide the detached-frame branch differently.  Directions exactly at the pole (lattice-aligned
    self-image edges, |1 - nhat_y| = 0) are treated alike by both sides."""
    ny = vec[:, 1] / np.linalg.norm(vec, axis=1)
    d = np.abs(1.0 - ny)
    band = (d >= thr / 2) & (d <= thr * 2)
    assert not band.any(), f"{int(band.sum())} edges inside the ambiguous pole band: choose another seed"
