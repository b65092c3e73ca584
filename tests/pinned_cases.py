"""Cases and float64 yardsticks of the pinned-graph tests (tests/test_gpu_pinned_graph.py, tests/test_pinned_graph_cpu.py).

The yardstick is ``PeriodicOracle.model_energy(graph=...)``: the checker's energy on a GIVEN edge list -- the graph of a reference
geometry held fixed while the positions (and the cell) move.  With ``graph=None`` the checker rebuilds the graph from the positions
it is given, which is what the engine does when nothing is pinned.

The rank swap: ``max_neigh`` keeps the nearest M candidates of every target.  Take a target whose M-th and (M+1)-th candidates have
different sources, and move the (M+1)-th's source along its line towards the target until it is 0.01 A closer than the M-th: the two
swap ranks, one edge of full weight leaves the rebuilt graph and another enters, while the pinned graph keeps the first."""
import numpy as np
import torch

from periodic_oracle import PeriodicOracle, periodic_radius_graph
from pdb2reaction_amd import synth

MAX_NEIGH = 4
INSIDE = 0.01          # A: how far inside the M-th neighbour the moved atom ends up
FD_H = 1e-3            # A: the step of the differences across the swap (and of the strain differences, as a strain)


def checker(weights, cell=None, pbc=None, max_neigh=MAX_NEIGH):
    return PeriodicOracle(weights, cell=cell, pbc=pbc, max_neigh=max_neigh)


def graph_of(orc, pos):
    """The checker's graph of ``pos`` (float64): (src, dst, shift, tidx)."""
    return periodic_radius_graph(np.asarray(pos, dtype=np.float64), orc.cell, orc.pbc, orc.cutoff, orc.max_neigh)


def graph_in_cell(orc, graph, cell):
    """``graph`` (built in ``orc.cell``) with its translations formed in another cell: the same integer triples times ``cell``."""
    src, dst, shift, tidx = graph
    ints = np.rint(shift.numpy() @ np.linalg.inv(orc.cell))
    assert np.abs(ints @ orc.cell - shift.numpy()).max() < 1e-9
    return src, dst, torch.as_tensor(ints @ np.asarray(cell, dtype=np.float64)), tidx


def same_graph(a, b):
    return len(a[0]) == len(b[0]) and bool((a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] - b[2]).abs().max() < 1e-9)


def energy_forces_on(orc, z, pos, graph=None):
    """(E eV float, F (N,3) eV/A float64) of the checker on ``graph`` (None: rebuilt from ``pos``)."""
    zt = torch.as_tensor(np.asarray(z), dtype=torch.long)
    p = torch.as_tensor(np.asarray(pos, dtype=np.float64), dtype=orc.dtype).clone().requires_grad_(True)
    e = orc.model_energy(zt, p, graph=graph)
    (g,) = torch.autograd.grad(e, p)
    rmsd = float(orc.p["normalizer.rmsd"][0])
    return float(e.detach()) * rmsd + float(orc.refs64[zt].sum()), (-g * rmsd).detach().numpy()


def energy_on(orc, z, pos, graph=None):
    zt = torch.as_tensor(np.asarray(z), dtype=torch.long)
    with torch.no_grad():
        e = orc.model_energy(zt, torch.as_tensor(np.asarray(pos, dtype=np.float64), dtype=orc.dtype), graph=graph)
    return float(e) * float(orc.p["normalizer.rmsd"][0]) + float(orc.refs64[zt].sum())


def swap_on(orc, pos, target=None):
    """A rank swap at ``orc.max_neigh`` in the geometry ``pos``: (target i, moved atom j, unit vector u from i to j's image, d_M, d_M+1).
    ``target=None``: the first target whose M-th and (M+1)-th candidates have different sources, neither of them the target itself."""
    m = orc.max_neigh
    wide = PeriodicOracle.__new__(PeriodicOracle)
    wide.__dict__.update(orc.__dict__)
    wide.max_neigh = None
    src, dst, shift, _ = graph_of(wide, pos)
    p = np.asarray(pos, dtype=np.float64)
    vec = p[src.numpy()] + shift.numpy() - p[dst.numpy()]
    dist = np.linalg.norm(vec, axis=1)
    for i in ([target] if target is not None else range(len(p))):
        rows = np.nonzero(dst.numpy() == i)[0]
        rows = rows[np.argsort(dist[rows], kind="stable")]
        if len(rows) <= m:
            continue
        a, b = rows[m - 1], rows[m]
        ja, jb = int(src[a]), int(src[b])
        if ja != jb and i not in (ja, jb) and dist[b] - dist[a] > 2 * INSIDE:
            return i, jb, vec[b] / dist[b], float(dist[a]), float(dist[b])
    raise AssertionError("no target with a clean rank swap in this geometry")


def swap_geometries(orc, pos, target=None):
    """(x_start, x_moved, x_swap, u, j) float32-rounded where stated by the issue: x_start the reference geometry, x_moved with atom j
    0.01 A inside the M-th neighbour of the target, x_swap with it exactly at the M-th's distance; u the unit vector of the line."""
    i, j, u, d_m, d_m1 = swap_on(orc, pos, target)
    x0 = np.asarray(pos, dtype=np.float32).astype(np.float64)
    moved, swap = x0.copy(), x0.copy()
    moved[j] = x0[j] - u * (d_m1 - (d_m - INSIDE))
    swap[j] = x0[j] - u * (d_m1 - d_m)
    return x0, moved.astype(np.float32).astype(np.float64), swap, u, j


def cluster_swap(weights):
    """The 12-atom case of the issue: ``make_cluster(12, seed=4)``, ``max_neigh=4``, target atom 0."""
    z, pos = synth.make_cluster(12, seed=4)
    orc = checker(weights)
    return (z, orc) + swap_geometries(orc, pos, target=0)


def triclinic_swap(weights):
    """A rank swap in the ``triclinic`` cell of ``stress_oracle.make_case`` (12 atoms, self images) at ``max_neigh=4``."""
    from stress_oracle import make_case

    z, imgs, cell, pbc = make_case("triclinic")
    orc = checker(weights, cell=cell, pbc=pbc)
    return (z, orc, cell, pbc) + swap_geometries(orc, imgs[0].astype(np.float64))
