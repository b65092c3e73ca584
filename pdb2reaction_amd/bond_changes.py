"""Bond-change detection between two geometries -- mirror of the reference's ``bond_changes`` module.

Reference: ``pdb2reaction/bond_changes.py`` -- ``compare_structures`` (:142-187, pairwise ``torch.cdist`` in float64 and
boolean masks), ``summarize_changes`` (:196-232), ``BondChangeResult`` (:93-100).  Here the two distance matrices and the
formed/broken classification come from ONE HIP kernel (``umx_bond_changes`` in ``include/umx.h``); there is no CPU path.
With ``cell=`` / ``pbc=`` the distances are minimum-image distances in that cell (``umx_bond_changes_cell``).
``compare_structures(matrices=False)`` and :func:`compare_path` take the event route instead (``umx_bond_events``): only the formed /
broken pairs and their two lengths come back, for any number of pairs of geometries from one engine call, with memory of order N.

Covalent radii: the reference takes ``pysisyphus.elem_data.COVALENT_RADII`` (third-party, absent here).  The table below
restates the published Cordero et al. 2008 single-bond radii (Dalton Trans. 2008, 2832) in Angstrom and converts them to
the unit of the coordinates (Bohr for pysisyphus geometries) -- [3P-UNVERIFIED against the pysisyphus table]; pass
``radii=`` to override.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Set, Tuple, Union

import numpy as np

from .uma_pysis import ANG2BOHR, BOHR2ANG

Pair = Tuple[int, int]

# Cordero 2008 covalent radii, Angstrom (C sp3; Mn/Fe/Co low-spin values)
COVALENT_RADII_ANG: Dict[str, float] = {
    "x": 0.00,
    "h": 0.31, "he": 0.28, "li": 1.28, "be": 0.96, "b": 0.84, "c": 0.76, "n": 0.71, "o": 0.66, "f": 0.57, "ne": 0.58,
    "na": 1.66, "mg": 1.41, "al": 1.21, "si": 1.11, "p": 1.07, "s": 1.05, "cl": 1.02, "ar": 1.06,
    "k": 2.03, "ca": 1.76, "sc": 1.70, "ti": 1.60, "v": 1.53, "cr": 1.39, "mn": 1.39, "fe": 1.32, "co": 1.26, "ni": 1.24,
    "cu": 1.32, "zn": 1.22, "ga": 1.22, "ge": 1.20, "as": 1.19, "se": 1.20, "br": 1.20, "kr": 1.16,
    "rb": 2.20, "sr": 1.95, "y": 1.90, "zr": 1.75, "nb": 1.64, "mo": 1.54, "tc": 1.47, "ru": 1.46, "rh": 1.42, "pd": 1.39,
    "ag": 1.45, "cd": 1.44, "in": 1.42, "sn": 1.39, "sb": 1.39, "te": 1.38, "i": 1.39, "xe": 1.40,
    "cs": 2.44, "ba": 2.15, "la": 2.07, "ce": 2.04, "pr": 2.03, "nd": 2.01, "pm": 1.99, "sm": 1.98, "eu": 1.98, "gd": 1.96,
    "tb": 1.94, "dy": 1.92, "ho": 1.92, "er": 1.89, "tm": 1.90, "yb": 1.87, "lu": 1.87,
    "hf": 1.75, "ta": 1.70, "w": 1.62, "re": 1.51, "os": 1.44, "ir": 1.41, "pt": 1.36, "au": 1.36, "hg": 1.32,
    "tl": 1.45, "pb": 1.46, "bi": 1.48, "po": 1.40, "at": 1.50, "rn": 1.50,
    "fr": 2.60, "ra": 2.21, "ac": 2.15, "th": 2.06, "pa": 2.00, "u": 1.96, "np": 1.90, "pu": 1.87, "am": 1.80, "cm": 1.69,
}


@dataclass
class BondChangeResult:
    """Zero-based (i < j) index pairs of formed / broken covalent bonds and the two N x N distance matrices
    (same unit as the input coordinates).  The event route leaves the matrices ``None`` and fills ``lengths``: for every formed or
    broken pair its length in the first and in the second geometry -- the entries the matrices would hold, bit for bit."""

    formed_covalent: Set[Pair]
    broken_covalent: Set[Pair]
    distances_1: Optional[np.ndarray] = None
    distances_2: Optional[np.ndarray] = None
    lengths: Optional[Dict[Pair, Tuple[float, float]]] = None


def element_radii(atoms: Iterable[str], unit_scale: float = ANG2BOHR, radii: Optional[Dict[str, float]] = None) -> Tuple[List[str], np.ndarray]:
    """Capitalised symbols and their covalent radii in coordinate units (``unit_scale`` = coordinate units per Angstrom)."""
    table = COVALENT_RADII_ANG if radii is None else {k.lower(): float(v) for k, v in radii.items()}
    elems = [str(a).capitalize() for a in atoms]
    try:
        cov = np.array([table[a.lower()] for a in elems], dtype=np.float64) * float(unit_scale)
    except KeyError as exc:
        raise KeyError(f"no covalent radius for element {exc.args[0]!r}") from None
    return elems, cov


_shared_engine = None


def _engine(device: str = "cuda"):
    """One light engine (no weights) per process for callers that do not hand one in."""
    global _shared_engine
    if _shared_engine is None:
        from .engine import Engine
        from .uma_pysis import _device_index

        _shared_engine = Engine(_device_index(device if str(device).lower().startswith("cuda") else "cuda"))
    return _shared_engine


def compare_structures(geom1, geom2, device: str = "cuda", bond_factor: float = 1.20, margin_fraction: float = 0.05,
                       delta_fraction: float = 0.05, *, engine=None, radii: Optional[Dict[str, float]] = None,
                       unit_scale: float = ANG2BOHR, cell=None, pbc=None, matrices: bool = True) -> BondChangeResult:
    """Formed / broken covalent bonds between two geometries with identical atoms (``.atoms``, ``.coords3d`` [N,3]).

    bonded(i,j) <=> D_ij <= T - margin_fraction*T with T = bond_factor*(r_i + r_j); a pair changes only when
    |D2 - D1| >= delta_fraction*T (reference bond_changes.py:160-176).  ``device`` is accepted for signature
    compatibility; the computation always runs on the engine's GPU.

    ``cell`` (3,3, rows as lattice vectors, IN THE UNIT OF THE COORDINATES -- Bohr for pysisyphus geometries) and ``pbc`` (a bool or
    three flags): D is the minimum-image distance over all lattice translations (``umx_bond_changes_cell``), so a bond across the
    boundary is a bond.  Without them the open-space call as it was.  No reference counterpart.

    ``matrices=False``: the event route (:func:`compare_path` on the one pair) -- the same sets, ``distances_1/2`` are ``None`` and
    ``lengths`` holds the two lengths of every changed pair; nothing of size N x N is formed on the device or the host.
    """
    if not matrices:
        return compare_path([geom1, geom2], [(0, 1)], device, bond_factor, margin_fraction, delta_fraction, engine=engine, radii=radii,
                            unit_scale=unit_scale, cell=cell, pbc=pbc)[0]
    if list(geom1.atoms) != list(geom2.atoms):
        raise AssertionError("Atom types and ordering must be identical.")
    _, cov = element_radii(geom1.atoms, unit_scale, radii)
    eng = engine if engine is not None else _engine(device)
    d1, d2, code = eng.bond_changes(np.asarray(geom1.coords3d, dtype=np.float64), np.asarray(geom2.coords3d, dtype=np.float64), cov,
                                    bond_factor, margin_fraction, delta_fraction, **({} if cell is None or pbc is None else {"cell": cell, "pbc": pbc}))
    formed = set(map(tuple, np.argwhere(code == 1).tolist()))
    broken = set(map(tuple, np.argwhere(code == 2).tolist()))
    return BondChangeResult(formed_covalent=formed, broken_covalent=broken, distances_1=d1, distances_2=d2)


def path_pairs(pairs: Union[str, Sequence[Pair]], n_geoms: int) -> List[Pair]:
    """The pairs of images :func:`compare_path` compares: ``"consecutive"`` (k, k + 1), ``"endpoints"`` (0, K - 1), ``"all"`` every
    a < b, or the given list as it is."""
    if isinstance(pairs, str):
        if pairs == "consecutive":
            return [(k, k + 1) for k in range(n_geoms - 1)]
        if pairs == "endpoints":
            return [(0, n_geoms - 1)]
        if pairs == "all":
            return [(a, b) for a in range(n_geoms) for b in range(a + 1, n_geoms)]
        raise ValueError(f"compare_path: pairs={pairs!r} is none of 'consecutive', 'endpoints', 'all'")
    return [(int(a), int(b)) for a, b in pairs]


def compare_path(geoms, pairs: Union[str, Sequence[Pair]] = "consecutive", device: str = "cuda", bond_factor: float = 1.20,
                 margin_fraction: float = 0.05, delta_fraction: float = 0.05, *, engine=None, radii: Optional[Dict[str, float]] = None,
                 unit_scale: float = ANG2BOHR, cell=None, pbc=None) -> List[BondChangeResult]:
    """Formed / broken covalent bonds between pairs of the geometries of a path, from ONE engine call (``umx_bond_events``).

    ``geoms``: geometries with identical atoms (``.atoms``, ``.coords3d``); ``pairs``: see :func:`path_pairs` -- pair (a, b) reports
    what forms or breaks going from ``geoms[a]`` to ``geoms[b]``.  One :class:`BondChangeResult` per pair, in the given order, with
    ``lengths`` filled and no matrices; the sets are those of :func:`compare_structures` on the same two geometries.  The other
    arguments as there: ``cell`` in the unit of the coordinates, and -- as there -- the cell is used only when BOTH ``cell`` and ``pbc``
    are given; one without the other is the open-space call.  Replaces the loops over ``_has_bond_change`` of the reference's ``path_search.py`` (:1015, :1200, :1310,
    :1361-1366)."""
    geoms = list(geoms)
    if not geoms:
        raise ValueError("compare_path: no geometries")
    atoms = list(geoms[0].atoms)
    if any(list(g.atoms) != atoms for g in geoms[1:]):
        raise AssertionError("Atom types and ordering must be identical.")
    todo = path_pairs(pairs, len(geoms))
    if not todo:
        return []
    _, cov = element_radii(atoms, unit_scale, radii)
    eng = engine if engine is not None else _engine(device)
    stack = np.stack([np.asarray(g.coords3d, dtype=np.float64).reshape(len(atoms), 3) for g in geoms])
    in_cell = {} if cell is None or pbc is None else {"cell": cell, "pbc": pbc}
    ev = eng.bond_events(stack, cov, todo, bond_factor, margin_fraction, delta_fraction, **in_cell)
    out = [BondChangeResult(formed_covalent=set(), broken_covalent=set(), lengths={}) for _ in todo]
    for p, i, j, code, d1, d2 in ev.tolist():
        (out[p].formed_covalent if code == 1 else out[p].broken_covalent).add((i, j))
        out[p].lengths[(i, j)] = (d1, d2)
    return out


def _bond_str(i: int, j: int, elems: Sequence[str], one_based: bool = True) -> str:
    o = 1 if one_based else 0
    return f"{elems[i]}{i + o}-{elems[j]}{j + o}"


def summarize_changes(geom, result: BondChangeResult, one_based: bool = True) -> str:
    """Text report in the reference's format ("Bond formed (n):" / "  - C1-O2 : 1.500 Å --> 1.360 Å" / "...: None");
    lengths are converted from Bohr to Angstrom (reference bond_changes.py:196-232).  They are read from the two matrices, or, when the
    result has none (the event route), from ``result.lengths``."""
    elems = [str(a).capitalize() for a in geom.atoms]
    d1, d2 = result.distances_1, result.distances_2
    have = isinstance(d1, np.ndarray) and isinstance(d2, np.ndarray) and d1.shape == d2.shape
    lengths = result.lengths if not have and result.lengths is not None else {}
    out: List[str] = []
    for title, pairs in (("Bond formed", result.formed_covalent), ("Bond broken", result.broken_covalent)):
        if not pairs:
            out.append(f"{title}: None")
            continue
        out.append(f"{title} ({len(pairs)}):")
        for i, j in sorted(pairs):
            ab = (d1[i, j], d2[i, j]) if have else lengths.get((i, j))
            tail = f" : {float(ab[0]) * BOHR2ANG:.3f} Å --> {float(ab[1]) * BOHR2ANG:.3f} Å" if ab is not None else ""
            out.append(f"  - {_bond_str(i, j, elems, one_based)}{tail}")
    return "\n".join(out)
