"""The cell family of the per-image-cell tests (tests/test_cells_cpu.py, tests/test_gpu_cells.py) -- a helper, not a test.

Image k of a family takes the FRACTIONAL coordinates of a base case of tests/stress_oracle.py (``triclinic``: 12 atoms, ``slab``: 48)
into cell k and adds N(0, 0.02 A) noise, rounded to float32.  The cells are chosen so that the translation tables differ in size from
image to image (a strained cell crosses a threshold of N_k); the expected sizes come from ``periodic_oracle.lattice_translations``,
never from a number written down here.  The noise seeds were picked on the CPU so that every image satisfies
``periodic_oracle.assert_clear_of_the_pole_band`` (tests/test_cells_cpu.py asserts it for all of them)."""
import numpy as np

from periodic_oracle import assert_clear_of_the_pole_band, lattice_translations, periodic_radius_graph
from stress_oracle import SLAB, TRICLINIC, make_case
from pdb2reaction_amd import weights as W

SHEAR = np.eye(3)
SHEAR[0, 1], SHEAR[2, 0] = 0.08, -0.05

TTT, TTF = (True, True, True), (True, True, False)
# name: (base case, pbc, cells, noise seed of every image)
FAMILIES = {
    "triclinic": ("triclinic", TTT, [TRICLINIC, TRICLINIC * 1.3, TRICLINIC * 0.8, TRICLINIC @ SHEAR, TRICLINIC * 0.97], [300, 301, 302, 303, 304]),
    "slab": ("slab", TTF, [SLAB, SLAB * 0.7], [310, 311]),
}


def family(name, k=None):
    """(z, images float32 [K,N,3], cells float64 [K,3,3], pbc) of a family: all its cells, the first ``k``, or those of the index
    list ``k``.  An image depends on its cell and seed alone, not on the selection."""
    base, pbc, cells, seeds = FAMILIES[name]
    z, p32, cell0, _ = make_case(base)
    frac = p32[0].astype(np.float64) @ np.linalg.inv(cell0)
    pick = list(range(len(cells)))[:k] if k is None or isinstance(k, int) else list(k)
    cells, seeds = np.array([cells[i] for i in pick], dtype=np.float64), [seeds[i] for i in pick]
    imgs = [frac @ c + 0.02 * np.random.default_rng(s).standard_normal(frac.shape) for c, s in zip(cells, seeds)]
    return z, np.asarray(imgs, dtype=np.float32), cells, pbc


def table_entries(cell, pbc, cutoff=W.CUTOFF):
    """Entries of the translation table of a cell, the zero translation included."""
    return len(lattice_translations(cell, pbc, cutoff)[0])


def assert_image_is_clear(p32, cell, pbc, max_neigh=None):
    """The input condition of the oracle comparisons, from the oracle's own edges of one float32 image; returns the graph."""
    p64 = np.asarray(p32, dtype=np.float64)
    graph = periodic_radius_graph(p64, cell, pbc, W.CUTOFF, max_neigh)
    assert_clear_of_the_pole_band(p64[graph[0].numpy()] + graph[2].numpy() - p64[graph[1].numpy()])
    return graph
