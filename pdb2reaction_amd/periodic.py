"""Minimum-image vectors in a periodic cell, numpy float64 on the host -- what the path stack above the engine needs of a cell.

The engine wraps its own scratch copy of the positions and searches the lattice translations itself (``umx_set_cell``); a string of
images, however, must be CONTINUOUS in Cartesian space before it is interpolated: a product atom that a relaxation wrapped across the
boundary would otherwise be dragged through the whole cell.  :func:`min_image` is the one helper behind that unwrapping
(``gsm.GrowingStringDriver``), with the distance definition of ``umx_bond_changes_cell`` (``include/umx.h``): round to the nearest
lattice point in fractional coordinates, then search the translations around it, because in a skewed cell the rounded image is often not
the nearest one.  Units are the caller's: the cell has the unit of the vectors.
"""
from __future__ import annotations

import itertools
from typing import Optional, Tuple

import numpy as np

MAX_AXIS = 4          # translations searched per direction and periodic axis, the cap of the engine (PBC_MAX_AXIS)


def pbc_flags(pbc) -> Optional[Tuple[bool, bool, bool]]:
    """``pbc`` (None, a bool or three flags) as a tuple of three bools; None when it is None or no flag is set (open boundaries)."""
    if pbc is None:
        return None
    f = tuple(bool(x) for x in np.broadcast_to(np.asarray(pbc, dtype=bool), (3,)))
    return f if any(f) else None


def same_cell(cell_a, pbc_a, cell_b, pbc_b, rtol: float = 1e-9) -> bool:
    """Do two (cell, pbc) pairs describe the same boundary?  Open equals open; otherwise equal flags and lattice vectors that agree on
    the periodic axes to ``rtol`` of the largest entry."""
    fa, fb = pbc_flags(pbc_a) if cell_a is not None else None, pbc_flags(pbc_b) if cell_b is not None else None
    if fa is None or fb is None:
        return fa is None and fb is None
    if fa != fb:
        return False
    a, b = np.asarray(cell_a, dtype=np.float64).reshape(3, 3)[list(fa)], np.asarray(cell_b, dtype=np.float64).reshape(3, 3)[list(fb)]
    return bool(np.abs(a - b).max() <= rtol * np.abs(a).max())


def lattice(cell, pbc):
    """(a, b, h, M) of the periodic sub-lattice: lattice vectors ``a`` (3,3, rows; zero on open axes), dual vectors ``b`` within the
    periodic span (``b_k . a_l = delta_kl``; zero on open axes), plane distances ``h_k = 1 / |b_k|`` and the search range
    ``M_k = floor(R / h_k + 1/2)`` with ``R`` half the summed lengths of the periodic vectors (0 on open axes).  A difference rounded to
    fractional coordinates within 1/2 is no longer than R, and a translate with ``|m_k| > M_k`` is longer than R: the box of ``M`` holds
    the nearest image.  ``ValueError``: a non-finite entry, a degenerate periodic sub-lattice, or ``M_k > 4``."""
    c = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    flags = pbc_flags(pbc)
    if flags is None:
        raise ValueError("lattice: no periodic axis (pbc is None or has no flag set)")
    if not np.isfinite(c).all():
        raise ValueError("non-finite cell entry")
    on = np.array(flags)
    p = c[on]                                                   # (np, 3) periodic rows
    ln = np.linalg.norm(p, axis=1)
    gram = p @ p.T
    if not (ln > 0).all() or not abs(np.linalg.det(gram)) > (1e-6 * np.prod(ln)) ** 2:
        raise ValueError("degenerate cell: the periodic lattice vectors are linearly dependent")
    a, b = np.zeros((3, 3)), np.zeros((3, 3))
    a[on] = p
    b[on] = np.linalg.solve(gram, p)
    h = np.zeros(3)
    h[on] = 1.0 / np.linalg.norm(b[on], axis=1)
    m = np.zeros(3, dtype=int)
    m[on] = np.floor(0.5 * ln.sum() / h[on] + 0.5).astype(int)
    if (m > MAX_AXIS).any():
        raise ValueError(f"cell too skewed for the minimum-image search: it needs {m.max()} lattice translations per direction, more than {MAX_AXIS}")
    return a, b, h, m


def min_image(delta, cell, pbc) -> np.ndarray:
    """The shortest of ``delta + (any lattice translation)`` for every vector of ``delta`` (..., 3): ``n = rint(delta . b)``,
    ``d0 = delta - n a``, then the minimum of ``|d0 + m a|`` over ``|m_k| <= M_k`` (:func:`lattice`).  Open axes are left alone.  Among
    images of exactly equal length the first in the order of the search (axis c fastest, from -M to M) is returned."""
    d = np.asarray(delta, dtype=np.float64)
    a, b, _, m = lattice(cell, pbc)
    d0 = d - np.rint(d @ b.T) @ a
    t = np.array(list(itertools.product(*(range(-k, k + 1) for k in m))), dtype=np.float64) @ a          # (n_cand, 3)
    cand = d0[..., None, :] + t
    best = np.argmin((cand * cand).sum(-1), axis=-1)
    return np.take_along_axis(cand, best[..., None, None], axis=-2)[..., 0, :]


def unwrap_onto(ref, x, cell, pbc) -> np.ndarray:
    """``x`` moved atom by atom to the periodic image nearest to ``ref``: ``ref + min_image(x - ref)``; shapes (..., 3), or flat (3N,)."""
    r, y = np.asarray(ref, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return (r.reshape(-1, 3) + min_image((y - r).reshape(-1, 3), cell, pbc)).reshape(y.shape)
