"""Float64 checker for the strain derivative (virial) and the stress -- a helper, not a test.

The model sees a geometry only through its edge vectors ``vec_e = r_src + t_e - r_dst``.  Under the homogeneous strain
``r -> r (1 + eps)``, ``cell -> cell (1 + eps)`` every translation ``t_e`` (an integer combination of the lattice vectors) is strained
with the cell, so every ``vec_e`` is multiplied by ``(1 + eps)``.  ``strain_derivative`` builds the graph ONCE, on the unstrained
geometry, feeds ``tests/periodic_oracle.PeriodicOracle.model_energy`` the strained positions and translations, and differentiates with
autograd with respect to ``eps`` at 0:  ``W[a, b] = dE / d eps_ab`` in eV (times the normaliser's rmsd; the element references do not
depend on the strain).  tests/test_stress_cpu.py holds it to central differences of the energy, to ``W = -sum r (x) F`` for a cluster
and to the supercell rule.  fairchem's own stress has not been compared [3P-UNVERIFIED].
"""
from __future__ import annotations

import copy

import numpy as np
import torch

from periodic_oracle import PeriodicOracle, periodic_radius_graph


def in_dtype(orc: PeriodicOracle, dtype) -> PeriodicOracle:
    """The same checker evaluating in ``dtype`` (the weights are float32 values: the cast loses nothing)."""
    if orc.dtype == dtype:
        return orc
    o = copy.copy(orc)
    o.dtype = dtype
    o.p = {k: v.to(dtype) for k, v in orc.p.items()}
    o.debug = {}
    return o


def strain_derivative(orc: PeriodicOracle, z, pos, dtype=torch.float64, graph=None) -> np.ndarray:
    """W (3,3) float64 in eV: autograd of the checker's energy with respect to the strain tensor at zero, the graph of the unstrained
    geometry (built in float64, whatever ``dtype``) held fixed; the model itself runs in ``dtype``."""
    o = in_dtype(orc, dtype)
    p64 = np.asarray(pos, dtype=np.float64)
    src, dst, shift, tidx = graph if graph is not None else periodic_radius_graph(p64, o.cell, o.pbc, o.cutoff, o.max_neigh)
    zt = torch.as_tensor(np.asarray(z), dtype=torch.long)
    eps = torch.zeros(3, 3, dtype=dtype, requires_grad=True)
    defo = torch.eye(3, dtype=dtype) + eps
    p = torch.as_tensor(p64, dtype=dtype) @ defo
    t = shift.to(dtype) @ defo
    e = o.model_energy(zt, p, graph=(src, dst, t, tidx))
    (g,) = torch.autograd.grad(e, eps)
    return g.detach().to(torch.float64).numpy() * float(orc.p["normalizer.rmsd"][0])


def strained_energy(orc: PeriodicOracle, z, pos, eps) -> float:
    """Total energy in eV of the geometry AND the cell under the strain ``eps`` (3,3), the graph built anew on the strained geometry."""
    defo = np.eye(3) + np.asarray(eps, dtype=np.float64)
    o = copy.copy(orc)
    o.cell = None if orc.cell is None else orc.cell @ defo
    o.debug = {}
    return o.energy_forces(z, np.asarray(pos, dtype=np.float64) @ defo, forces=False)[0]


def voigt_stress(W, cell) -> np.ndarray:
    """(6,) eV/A^3 in Voigt order xx, yy, zz, yz, xz, xy: the symmetric part of W over |det cell| (ASE's convention, tensile positive)."""
    W = np.asarray(W, dtype=np.float64)
    s = 0.5 * (W + W.T) / abs(np.linalg.det(np.asarray(cell, dtype=np.float64).reshape(3, 3)))
    return np.array([s[0, 0], s[1, 1], s[2, 2], s[1, 2], s[0, 2], s[0, 1]])


# ---- the periodic cases of tests/test_gpu_periodic.py (same cells, grids and seeds), positions rounded to float32 ------------------
CUBIC = np.eye(3) * 14.0
TRICLINIC = np.array([[5.0, 0.0, 0.0], [1.1, 6.0, 0.0], [0.7, -0.9, 7.0]])
SLAB = np.array([[8.6, 0.0, 0.0], [1.3, 8.2, 0.0], [0.0, 0.0, 6.5]])
CASES = {
    # name: (cell, pbc, grid, seed, faces)
    "cubic": (CUBIC, (True, True, True), (5, 5, 5), 11, None),            # 125 atoms
    "triclinic": (TRICLINIC, (True, True, True), (2, 2, 3), 5, (10, 1)),  # 12 atoms: several images per pair, self images
    "slab": (SLAB, (True, True, False), (4, 4, 3), 7, None),              # 48 atoms, open along c
}


def make_case(name, k=1):
    """(z, images float32 [k,N,3], cell, pbc): image 0 is the jittered lattice, the others add N(0, 0.02 A) noise."""
    from periodic_oracle import commensurate_atoms

    cell, pbc, grid, seed, faces = CASES[name]
    z, pos = commensurate_atoms(cell, grid, seed, faces=faces)
    imgs = [pos] + [pos + 0.02 * np.random.default_rng(seed + 100 + i).standard_normal(pos.shape) for i in range(1, k)]
    return z, np.asarray(imgs, dtype=np.float32), cell, pbc
