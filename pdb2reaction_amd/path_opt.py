"""The GSM branch of the reference's ``path-opt`` flow as ONE function on plain arrays: the caller of the hot path.

Reference ``path_opt.cli`` (``path_opt.py:669-1091``), GSM mode, does, with one shared calculator (``:823``):
optional endpoint pre-optimisation (``_optimize_single``, ``:826-868``) -> rigid alignment + staged anchor scan of the second endpoint
onto the first (``align_and_refine_sequence_inplace``, ``:871-886``) -> ``GrowingString`` + ``StringOptimizer.run()`` (``:949-977``) ->
``final_geometries.trj`` with the energies on the comment lines (``:983-1004``) -> highest-energy image ``hei.xyz`` (``:1033-1048``).
:func:`optimize_path_gsm` strings together this repository's counterparts of exactly those steps -- ``rfo.optimize_single``,
``prestep.align_and_refine_sequence``, ``gsm.GrowingStringDriver.from_calculator`` (device resident on the engine, every cycle ONE batched
evaluation, images sharded over ranks when torch.distributed is initialised), ``formats.write_trj_with_energy`` / ``write_xyz``,
``string.select_hei_index`` -- so that a ``path-opt`` run is one call.  Click options, YAML merging, PDB / GJF conversion and exit codes are
the reference's CLI plumbing and stay out of scope; failures raise.

Keyword defaults are the CLI's: ``max_nodes = 10`` (``GS_KW``), ``fix_ends = False`` (``--fix-ends`` default, ``:663-668,735-736``),
``max_cycles = 300`` for both ``opt.max_cycles`` and ``stop_in_when_full`` (``:731-732``), ``climb = True``, ``preopt = False``.
"""
from __future__ import annotations

import os
from typing import Any, Dict, Optional, Sequence

import numpy as np

from ._calculator_base import ANG2BOHR, BOHR2ANG
from . import formats
from .gsm import GS_KW, STOPT_KW, GrowingStringDriver
from .string import select_hei_index


def optimize_path_gsm(elem: Sequence[str], reactant_ang: np.ndarray, product_ang: np.ndarray, *, calc=None, calc_kw: Optional[Dict[str, Any]] = None,
                      freeze_atoms: Sequence[int] = (), max_nodes: int = GS_KW["max_nodes"], max_cycles: int = 300, climb: bool = True,
                      fix_ends: bool = False, thresh: Optional[str] = None, preopt: bool = False, preopt_max_cycles: int = 10000,
                      sopt_kind: str = "lbfgs", sopt_cfg: Optional[Dict[str, Any]] = None, align: bool = True, align_kw: Optional[Dict[str, Any]] = None,
                      gs_kw: Optional[Dict[str, Any]] = None, stopt_kw: Optional[Dict[str, Any]] = None, out_dir: Optional[str] = None,
                      group=None, log=None, cell=None, pbc=None, bond_changes: bool = False, bond_engine=None, hei_modes: int = 0, masses_amu=None,
                      hei_modes_kw: Optional[Dict[str, Any]] = None, hei_tsopt: bool = False, hei_tsopt_kw: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
    """Minimum-energy path between two endpoint geometries (Angstrom) by the growing-string method on the HIP engine.

    calc: a ``uma_pysis`` instance shared by every step (created from ``calc_kw`` + ``freeze_atoms`` when None, as ``path_opt.py:823``).
    Returns ``{"images_ang" (K, N, 3), "energies" (K,) Hartree, "hei_index", "converged", "cycles", "force_evaluations", "fully_grown",
    "preopt": [...], "align": [...], "files": {...}, "cell", "pbc"}``; with ``out_dir`` the reference's ``final_geometries.trj`` and ``hei.xyz``
    are written.

    cell (3,3) lattice vectors as rows in ANGSTROM, pbc a bool or three flags: the path in one fixed periodic cell.  The calculator is
    created with the cell, or a given one must carry the same cell (``ValueError`` otherwise; a calculator that carries a cell hands it
    over when none is passed).  The pre-optimisation runs as it is; the rigid alignment is NOT run -- a rotation is no symmetry of a
    lattice -- and reported as ``"align": [{"skipped": "periodic cell"}]``: the driver's minimum-image unwrapping of the product onto the
    reactant takes its place.  The images come back unwrapped, as the driver holds them; the file formats do not change.

    bond_changes=True: the result gains ``"bond_changes"`` (:func:`path_bond_changes`): the report text first image -> last image and,
    per neighbouring pair of final images, the formed / broken pairs -- one ``umx_bond_events`` call on ``bond_engine`` (default: the
    process's light engine), in a periodic run with the run's cell and flags.  False (default): exactly the keys above.

    hei_modes=k > 0: the result gains ``"hei_modes"``: ``{"freqs_cm" (k,) signed cm^-1, "converged" (k,) bool, "images": evaluations
    spent, "n_imaginary"}`` of the k lowest vibrational modes of the FINAL highest-energy image -- one ``calc.get_lowest_modes`` call
    after the run (block Davidson on Hessian-vector products, no Hessian), with the run's frozen atoms and in the run's cell;
    ``masses_amu`` (N,) as that method takes them, ``hei_modes_kw`` its further keywords.  A first-order saddle has exactly one negative
    entry.  0 (default): exactly the keys above; the run loop itself never asks for modes.

    hei_tsopt=True: after the run the final highest-energy image -- which is no stationary point -- is refined to a first-order saddle by
    one ``calc.get_ts`` call (a dimer on Hessian-vector products, ``dimer.refine_saddles``) with the string tangent there as the start
    direction (one-sided when the HEI is an end image; ``mode=None``, the lowest mode, when the string has no tangent), the run's frozen
    atoms and the run's cell; ``hei_tsopt_kw`` its further keywords.  The result gains ``"ts"``:
    ``{"coords_ang" (N,3), "energy" Hartree, "curvature" Hartree/Bohr^2, "converged", "cycles", "images"}``, and with ``hei_modes=k`` the
    frequencies are those of the refined geometry.  False (default): exactly the keys above."""
    log = log or (lambda s: None)
    elem = [str(e).capitalize() for e in elem]
    n = len(elem)
    freeze = sorted({int(i) for i in freeze_atoms})
    from . import periodic as PBC

    if cell is not None and PBC.pbc_flags(pbc) is None:
        cell = pbc = None                                        # no flag set: open boundaries
    if calc is None:
        from .uma_pysis import uma_pysis

        calc = uma_pysis(**{**(calc_kw or {}), "freeze_atoms": freeze, **({} if cell is None else {"cell": cell, "pbc": pbc})})
    elif cell is None:
        cell, pbc = getattr(calc, "cell", None), getattr(calc, "pbc", None)
    elif hasattr(calc, "cell") and not PBC.same_cell(cell, pbc, calc.cell, getattr(calc, "pbc", None)):
        raise ValueError(f"optimize_path_gsm: cell= / pbc= do not describe the cell the given calculator evaluates in ({getattr(calc, 'cell', None)}, "
                         f"pbc={getattr(calc, 'pbc', None)})")
    periodic = cell is not None and PBC.pbc_flags(pbc) is not None
    geoms = [np.asarray(reactant_ang, dtype=np.float64).reshape(n, 3) * ANG2BOHR, np.asarray(product_ang, dtype=np.float64).reshape(n, 3) * ANG2BOHR]

    # optional endpoint pre-optimisation (path_opt.py:826-868): a failure keeps the input geometry, as the reference does
    pre = []
    if preopt:
        from .rfo import optimize_single

        cfg = {"max_cycles": int(preopt_max_cycles), **(sopt_cfg or {})}
        for i in range(2):
            try:
                r = optimize_single(calc, elem, geoms[i], sopt_kind, cfg, freeze=freeze)
                geoms[i] = np.asarray(r["coords"], dtype=np.float64).reshape(n, 3)
                pre.append({"converged": bool(r["converged"]), "cycles": int(r["cycles"]), "energy": float(r["energy"])})
                log(f"[preopt] endpoint {i}: {sopt_kind} {'converged' if r['converged'] else 'stopped'} after {r['cycles']} cycles")
            except Exception as exc:     # noqa: BLE001 -- reference: "[preopt] WARNING: Failed to preoptimize endpoint" and carry on
                pre.append({"error": f"{type(exc).__name__}: {exc}"})
                log(f"[preopt] WARNING: endpoint {i} not pre-optimised: {exc}")

    # rigid alignment + staged anchor scan of the product onto the reactant (path_opt.py:871-886); skipped with a note on failure
    align_info = []
    if periodic:
        align_info = [{"skipped": "periodic cell"}]
    elif align:
        from .prestep import align_and_refine_sequence

        try:
            geoms, align_info = align_and_refine_sequence(calc, elem, geoms, [freeze, freeze], **(align_kw or {}))
        except Exception as exc:         # noqa: BLE001 -- reference: "[align] WARNING: alignment skipped"
            align_info = [{"error": f"{type(exc).__name__}: {exc}"}]
            log(f"[align] WARNING: alignment skipped: {exc}")

    g = {"max_nodes": int(max_nodes), "climb": bool(climb), "climb_lanczos": bool(climb) and GS_KW["climb_lanczos"], "fix_first": bool(fix_ends),
         "fix_last": bool(fix_ends), **(gs_kw or {})}
    o = {"max_cycles": int(max_cycles), "stop_in_when_full": int(max_cycles), **({"thresh": thresh} if thresh else {}), **(stopt_kw or {})}
    drv = GrowingStringDriver.from_calculator(elem, geoms[0].reshape(-1), geoms[1].reshape(-1), calc, group=group, gs_kw=g, stopt_kw=o, log=log,
                                              **({"cell": np.asarray(cell, dtype=np.float64).reshape(3, 3) * ANG2BOHR, "pbc": pbc} if periodic else {}))
    res = drv.run()
    images_ang = res.coords.reshape(len(res.coords), n, 3) * BOHR2ANG
    hei = select_hei_index(res.energies)                         # path_opt.py:259-273
    files: Dict[str, str] = {}
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        files["final_geometries"] = os.path.join(out_dir, "final_geometries.trj")
        formats.write_trj_with_energy(elem, images_ang, res.energies, files["final_geometries"])
        files["hei"] = os.path.join(out_dir, "hei.xyz")
        formats.write_xyz(elem, images_ang[hei], files["hei"], energy_hartree=float(res.energies[hei]))
    out = {"images_ang": images_ang, "energies": res.energies, "hei_index": int(hei), "converged": bool(res.converged), "cycles": int(res.cycles),
           "force_evaluations": int(res.force_evaluations), "fully_grown": bool(res.fully_grown), "history": res.history, "timing": res.timing,
           "device": str(drv.device), "preopt": pre, "align": align_info, "files": files, "defaults": {"GS_KW": dict(GS_KW), "STOPT_KW": dict(STOPT_KW)},
           "cell": None if not periodic else np.array(cell, dtype=np.float64).reshape(3, 3), "pbc": PBC.pbc_flags(pbc) if periodic else None}
    if bond_changes:
        out["bond_changes"] = path_bond_changes(elem, np.asarray(res.coords, dtype=np.float64).reshape(len(res.coords), n, 3), engine=bond_engine,
                                                **({"cell": np.asarray(cell, dtype=np.float64).reshape(3, 3) * ANG2BOHR, "pbc": pbc} if periodic else {}))
    at_bohr = np.asarray(res.coords[hei], dtype=np.float64).reshape(-1)      # where the modes are asked for: the HEI, or the saddle refined from it
    if hei_tsopt:
        pts = np.asarray(res.coords, dtype=np.float64).reshape(len(res.coords), -1)
        tangent = pts[min(hei + 1, len(pts) - 1)] - pts[max(hei - 1, 0)]      # central difference of the neighbours (one-sided at an end)
        if not tangent.any():                                                # a string of one point has no tangent: the lowest mode instead
            tangent = None
        ts = calc.get_ts(elem, at_bohr, tangent, **(hei_tsopt_kw or {}))
        at_bohr = np.asarray(ts["coords"], dtype=np.float64).reshape(-1)
        out["ts"] = {"coords_ang": at_bohr.reshape(n, 3) * BOHR2ANG, "energy": float(ts["energy"]), "curvature": float(ts["curvature"]),
                     "converged": bool(ts["converged"]), "cycles": int(ts["cycles"]), "images": int(ts["images"])}
    if int(hei_modes) > 0:
        m = calc.get_lowest_modes(elem, at_bohr, int(hei_modes), masses_amu, **(hei_modes_kw or {}))
        out["hei_modes"] = {"freqs_cm": np.asarray(m["freqs_cm"]), "converged": np.asarray(m["converged"]), "images": int(m["images"]),
                            "n_imaginary": int((np.asarray(m["freqs_cm"]) < 0.0).sum())}
    return out


def path_bond_changes(elem: Sequence[str], images_bohr: np.ndarray, *, engine=None, cell=None, pbc=None) -> Dict[str, Any]:
    """Which bonds change along a string, from ONE engine call (``bond_changes.compare_path``: the consecutive pairs of images plus
    first against last).  images_bohr (K, N, 3) and ``cell`` in Bohr.  ``{"endpoints": the reference's report text for image 0 ->
    image K - 1 (``summarize_changes``), "segments": [{"images": [k, k + 1], "formed": [[i, j], ...], "broken": [...]}, ...]}`` -- what
    the reference's path code reports after every string (``path_search.py:1200``, ``:1361-1366``)."""
    import types

    from . import bond_changes as BC

    geoms = [types.SimpleNamespace(atoms=list(elem), coords3d=x) for x in np.asarray(images_bohr, dtype=np.float64)]
    k = len(geoms)
    pairs = [(a, a + 1) for a in range(k - 1)] + [(0, k - 1)]
    res = BC.compare_path(geoms, pairs, engine=engine, **({} if cell is None or pbc is None else {"cell": cell, "pbc": pbc}))
    segs = [{"images": [a, b], "formed": [list(p) for p in sorted(r.formed_covalent)], "broken": [list(p) for p in sorted(r.broken_covalent)]}
            for (a, b), r in zip(pairs[:-1], res[:-1])]
    return {"endpoints": BC.summarize_changes(geoms[-1], res[-1]), "segments": segs}
