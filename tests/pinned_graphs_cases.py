"""Cases of the per-image pinned-graph tests (tests/test_pinned_graphs_cpu.py, tests/test_gpu_pinned_graphs.py): sets of reference
images whose graphs differ in their edge counts, with the counts the float64 checker (``periodic_radius_graph`` at its own cutoff)
gives them.  The CPU test asserts the counts, the GPU tests hold ``pinned_graphs()`` to them -- so none of them can pass on references
that happen to share one graph.

The open sets scale one cluster: x 2.0 thins the graph, x 50 leaves no atom within the cutoff of another (an EMPTY reference).  The
12-atom counts (48, 0, 47) put several whole images into one 256-thread block of the replay, with the empty one between the other two;
the 40-atom counts (1206, 764, 288) are above 256 and no multiple of 64, so an image's edges cross block and wave boundaries.  The
periodic sets are the noisy copies of ``stress_oracle.make_case``; in the triclinic cell a cap of 50 binds on some atoms only.

Row parity.  The engine's GEMM operands alternate the sign of their ODD rows (umx_edge.h, "sign-alternating rows"), so the
rounding of an edge depends on whether its row in the chunk is even or odd.  With several references pinned the planner therefore ends
a chunk behind an odd number of edges, and every image is bitwise its evaluation alone; an UNPINNED batch keeps its chunks, so there an
image behind an odd count differs from the image alone by float32 rounding.  ``behind_odd`` names the sets in which, in reference
order, an image follows an odd count: only for those does the unpinned batch differ from its own singles.  ``open12_capped`` (48, 0, 47)
and ``triclinic_capped`` (596, 596, 595) have their odd count last, ``triclinic_mid`` (596, 595, 596) has it in the middle."""
import numpy as np

from pdb2reaction_amd import synth
from stress_oracle import make_case

ASSIGN = [2, 0, 0, 1, 2]          # test 2: repeats, not monotone, five images over three references

# name: (max_neigh, edges per reference, largest in-degree over the references)
EXPECTED = {
    "open12_capped": (4, (48, 0, 47), 4),
    "open12_even": (4, (48, 0, 10), 4),
    "triclinic_pair": (55, (610, 616), 55),            # images 0 and 3 of make_case("triclinic", k=4)
    "open40": (None, (1206, 764, 288), 39),
    "triclinic_capped": (50, (596, 596, 595), 50),      # copies 0, 2, 1 of make_case("triclinic", k=3)
    "triclinic_mid": (50, (596, 595, 596), 50),         # copies 0, 1, 2
    "slab": (None, (2914, 2926, 2928), 70),
}

# the table of the issue: (atoms, seed, scale, max_neigh) -> directed edges
TABLE = [
    ((12, 4, 1.0, 4), 48), ((12, 4, 2.0, 4), 47), ((12, 4, 50.0, 4), 0), ((12, 4, 1.0, None), 132),
    ((40, 1, 1.0, None), 1206), ((40, 1, 1.3, None), 764), ((40, 1, 2.0, None), 288),
]


def scaled_cluster(n, seed, scale):
    """(z, x float32): ``make_cluster(n, seed)`` rounded to float32, times ``scale`` in float32."""
    z, pos = synth.make_cluster(n, seed=seed)
    return z, pos.astype(np.float32) * np.float32(scale)


def reference_set(name):
    """(z, refs float32 [R,N,3], cell, pbc, max_neigh) of the set ``name``."""
    max_neigh = EXPECTED[name][0]
    if name in ("open12_capped", "open12_even"):
        z = scaled_cluster(12, 4, 1.0)[0]
        return z, np.stack([scaled_cluster(12, 4, s)[1] for s in (1.0, 50.0, 2.0 if name == "open12_capped" else 3.0)]), None, None, max_neigh
    if name == "triclinic_pair":
        z, imgs, cell, pbc = make_case("triclinic", k=4)
        return z, imgs[[0, 3]], cell, pbc, max_neigh
    if name == "open40":
        z = scaled_cluster(40, 1, 1.0)[0]
        return z, np.stack([scaled_cluster(40, 1, s)[1] for s in (1.0, 1.3, 2.0)]), None, None, max_neigh
    z, imgs, cell, pbc = make_case("slab" if name == "slab" else "triclinic", k=3)
    return z, (imgs[[0, 2, 1]] if name == "triclinic_capped" else imgs), cell, pbc, max_neigh


def behind_odd(edges):
    """Does, in this order, an image follow an odd number of edges?"""
    return any(sum(edges[:k]) % 2 for k in range(1, len(edges)))


def checker_counts(pos, cell, pbc, max_neigh, cutoff):
    """(directed edges, largest in-degree) of the checker's graph of ``pos``."""
    from periodic_oracle import periodic_radius_graph

    dst = periodic_radius_graph(np.asarray(pos, dtype=np.float64), cell, pbc, cutoff, max_neigh)[1].numpy()
    return len(dst), int(np.bincount(dst, minlength=len(pos)).max()) if len(dst) else 0


def displaced(refs, assign, seed=3, sigma=0.06):
    """Y[k] = refs[assign[k]] + N(0, sigma A) noise, float32: geometries near their own reference, each another one."""
    rng = np.random.default_rng(seed)
    return np.stack([refs[a] + sigma * rng.standard_normal(refs[a].shape).astype(np.float32) for a in assign]).astype(np.float32)


def strained_cells(cell):
    """Four cells near ``cell``: two volume strains, two shears."""
    out = []
    for a, b, h in ((0, 0, 0.01), (1, 1, -0.008), (0, 1, 0.006), (1, 2, -0.007)):
        e = np.zeros((3, 3))
        e[a, b] = h
        out.append(np.asarray(cell, dtype=np.float64) @ (np.eye(3) + e))
    return np.stack(out)

