"""Fingerprint of every kind of launch plan: one line per configuration with the sha256 of the energies, the forces, the virial where
asked and, with captures on, of every debug capture in name order.  A host-code refactor must leave every line as it was: run it on both
trees (python tools/gpu_plan_fingerprint.py > out.txt) and compare the files.  An engine error prints as the line's result.
The ``S120x2`` lines run two lanes with one image of more than 4096 edges per chunk: the capped grids of the stream kernels loop twice.

The ``graph`` section (lines that start with "graph"; ``python tools/gpu_plan_fingerprint.py graph`` prints it alone, ``plans`` the
rest) holds the neighbour-graph stage: the six graph captures, energies and forces, ``graph_stats()`` and ``last_graph_shifts()`` of
every geometry of tests/graph_cases.py and tests/cells_cases.py, through every instantiation of the graph kernels."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pdb2reaction_amd import synth, weights as W            # noqa: E402
from pdb2reaction_amd.engine import Engine                  # noqa: E402
from pdb2reaction_amd.parallel import LocalEnginePool       # noqa: E402

MODES = ("bf16x3", "split-bf16", "split", "fp32")
# the last three reach the plane-GEMM instantiations the defaults leave out (umx_launch.h pl_kernels): LS and aligned planes on the complex
# products, their half-height forms, and the forms without LS, alignment or half height
ENVS = ({}, {"UMX_STREAMS": "2", "UMX_LANES_ONE_STREAM": "1"}, {"UMX_FORCE_PARTS": "3"},
        {"UMX_LOW_SEP": "2", "UMX_ALIGN_PLANES": "1"}, {"UMX_LOW_SEP": "2", "UMX_ALIGN_PLANES": "1", "UMX_GEMM_HALF": "3"},
        {"UMX_LOW_SEP": "0", "UMX_ALIGN_PLANES": "0", "UMX_GEMM_HALF": "0"})
VALUED = ("UMX_LOW_SEP", "UMX_ALIGN_PLANES", "UMX_GEMM_HALF")        # switches whose value is part of a line's label


def env_label(env):
    return "+".join(f"{k}={env[k]}" if k in VALUED else k for k in sorted(env))
STEMS = """row_ptr src dst out_ptr out_edge evec frame a2 a2q a2h rad x0 h1pre h2pre xn xrot hid hidq hidh y1q y1h hg msg xmid gridin gridout
xn2 ffg1 ffg2 x gspre ffh ffhg e_node pre1 pre2 xf g_pre2 g_sil1 g_pre1 g_xf g_xfinal g_gridout g_gsil2 g_ffg2 g_gsil1 g_ffg1 g_gridin g_xn2
g_xn2a g_ffhg g_ffh g_gs g_xmid gmsgq gmsgpl g_msg g_hid ghgq ghgpl g_hg g_y1 gradq gradpl g_xrot g_rad g_a2 dedd_rad g_xn g_xin dedd tau
gvec""".split()
NAMES = sorted(s + t for s in STEMS for t in ("", ".deg", ".0", ".1", ".2", ".3"))


def sha(*arrays):
    return " ".join("-" if a is None else hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16] for a in arrays)


def captures(eng):
    out = []
    for name in NAMES:
        try:
            out.append(f"{name}={sha(eng.debug_fetch(name, dtype=np.uint8))}")
        except Exception:                                     # no capture of this name in this mode
            pass
    return f"{len(out)} captures " + " ".join(out)


def line(label, fn):
    try:
        res = fn()
    except Exception as exc:                                  # the same error on both trees is the same fingerprint
        res = f"ERROR {str(exc)[:120]}"
    print(f"{label}: {res}", flush=True)


def engine_lines(label, eng, p, env, big=False):
    """The plan kinds of one engine created under `env`, for the system it has bound (big: the plain plan only, with its edge count)."""
    ef = lambda q=p: sha(*eng.energy_forces(q))              # noqa: E731
    if big:
        return line(f"{label} {env_label(env) or 'plain'}", lambda: ef() + f" {eng.graph_stats()[0]} edges")
    if env:
        line(f"{label} {env_label(env)}", ef)
        eng.set_recompute(2)
        line(f"{label} {env_label(env)} recompute2", ef)
        return eng.set_recompute(0)
    line(f"{label} plain", ef)
    line(f"{label} energy-only", lambda: sha(eng.energy_forces(p, forces=False)[0]))
    os.environ["UMX_MAX_CHUNK_IMAGES"] = "1"
    line(f"{label} chunk1", ef)
    del os.environ["UMX_MAX_CHUNK_IMAGES"]
    eng.debug_keep(True)
    line(f"{label} captures", lambda: ef() + " " + captures(eng))
    eng.debug_keep(False)
    eng.set_recompute(2)
    line(f"{label} recompute2", ef)
    eng.set_recompute(0)
    eng.pin_graph(p[0])
    line(f"{label} pinned", lambda: ef(p + np.float32(0.01)))
    eng.unpin_graph()
    eng.set_cell(np.eye(3) * 14.0, True)
    line(f"{label} cell+virial", lambda: sha(*eng.energy_forces_virial(p)))
    eng.set_cell(None)


def main():
    z40, p40, _ = synth.make_images(40, 3)
    systems = [("S40", z40, p40.astype(np.float32), {})]
    for name, n, mn in (("T17", 17, 3), ("T13", 13, 5)):     # the truncated systems of tests/test_gpu_edge_links.py, three jittered copies
        z, pos = synth.make_cluster(n)
        systems.append((name, z, np.stack([pos + 0.01 * k * np.sin(pos[:, ::-1]) for k in range(3)]).astype(np.float32), {"max_neigh": mn}))
    # one image with more than 32 640 directed edges: the smallest count at which a wide grid of the complex N = 128 products fills the
    # chip (choose_pl `fills`), so the wide complex forms without LS run
    z560, p560 = synth.make_cluster(560)
    systems.append(("S560", z560, p560[None].astype(np.float32), {}))
    for ff in ("spectral", "grid"):
        w = W.make_synthetic_weights(0, **({"ff_type": "grid"} if ff == "grid" else {}))
        for mode in MODES:
            for env in ENVS:                                  # (the switches are read when the engine is made and when it evaluates)
                os.environ.update(env)
                eng = Engine(0, precision=mode)
                eng.load_weights(w)
                for name, z, p, kw in systems:
                    eng.set_system(z, **kw)
                    engine_lines(f"{mode} {ff} {name}", eng, p, env, big=name == "S560")
                eng.close()
                [os.environ.pop(k) for k in env]
            with LocalEnginePool.create([0, 0], w, precision=mode) as pool:
                for name, z, p, kw in systems[:-1]:
                    pool.set_system(z, **kw)
                    line(f"{mode} {ff} {name} pool-gp", lambda: sha(*pool.energy_forces(p[:1])) + f" {pool.last_route}")
                    line(f"{mode} {ff} {name} pool-gp+virial", lambda: sha(*pool.energy_forces_virial(p[:1], graph_parallel=True)) + f" {pool.last_route}")
    # two lanes with one image per chunk, each image with more than 4096 edges: the capped grids of the throttled stream kernels (512
    # workgroups of 4 or 8 edges) walk their grid-stride loops twice -- nothing above does
    z120, p120, _ = synth.make_images(120, 2, seed=21)
    env = {"UMX_STREAMS": "2", "UMX_MAX_CHUNK_IMAGES": "1"}
    w = W.make_synthetic_weights(0)
    for mode in MODES:
        os.environ.update(env)
        eng = Engine(0, precision=mode)
        eng.load_weights(w)
        eng.set_system(z120)
        line(f"{mode} spectral S120x2 {env_label(env)}",
             lambda: sha(*eng.energy_forces(p120.astype(np.float32))) + f" {eng.graph_stats()[0]} edges {eng.last_lanes()} lanes")
        eng.close()
        [os.environ.pop(k) for k in env]


# ---- the neighbour-graph stage ---------------------------------------------------------------------------------------------------
GRAPH_NAMES = ("row_ptr", "src", "dst", "out_ptr", "out_edge", "evec")


def graph_line(label, eng, pos, double=False):
    """sha256 of the six graph captures, of the energies and forces, graph_stats() and last_graph_shifts() of one evaluation (several
    chunks: the captures are the last chunk's)"""
    def run():
        e, f = eng.energy_forces(pos, double_positions=double)
        caps = [eng.debug_fetch(n, np.uint8) for n in GRAPH_NAMES]
        return f"{sha(*caps)} E,F {sha(e, f)} stats {eng.graph_stats()} shifts {eng.last_graph_shifts()}"
    line(f"graph {label}{' f64' if double else ''}", run)


def graph_engine(w, env=None):
    os.environ.update(env or {})
    eng = Engine(0)
    [os.environ.pop(k) for k in env or {}]
    eng.load_weights(w)
    eng.debug_keep(True)
    return eng


def displaced(x):
    return x + 0.01 * np.sin(3.0 * x[..., ::-1])


def graph_main():
    """Every geometry of tests/graph_cases.py and the cell families of tests/cells_cases.py through every instantiation of the graph
    kernels: open / one cell / per-image cells x float / double x the truncating forms x the pinning fill and the replay."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import graph_cases as G
    import cells_cases as CC

    os.environ["UMX_DEBUG_ONLY"] = G.NAMES
    w = W.make_synthetic_weights(0)
    eng = graph_engine(w)
    for name in G.OPEN:
        z, pos, radius, mn = G.open_case(name)
        eng.set_system(z, radius=radius, max_neigh=mn)
        for dbl in (False, True):
            graph_line(f"open {name} cap {mn}", eng, pos, dbl)
    for n in (63, 64, 65, 129):
        z, pos = G.seam_case(n)
        for mn in (8, None):
            eng.set_system(z, radius=6.0, max_neigh=mn)
            for dbl in (False, True):
                graph_line(f"seam {n} cap {mn}", eng, pos, dbl)
    for n, k in ((205, 5), (129, 9)):
        z, imgs = G.batch_case(n, k)
        one = graph_engine(w, {"UMX_STREAMS": "1"})
        one.set_system(z, radius=6.0, max_neigh=20)
        for dbl in (False, True):
            graph_line(f"batch {k} x {n} cap 20", one, imgs, dbl)
        one.close()
    z, pos, radius, mn = G.open_case("G10")
    parts = graph_engine(w, {"UMX_FORCE_PARTS": "3"})
    parts.set_system(z, radius=radius, max_neigh=mn)
    for dbl in (False, True):
        graph_line("open G10 UMX_FORCE_PARTS=3", parts, pos, dbl)
    parts.close()
    # cells: one shared cell or identical per-image cells, two images; the binding cap reaches the truncating periodic form; Cap at 50
    # is refused (more candidates than the truncating fill ranks) and the refusal is the line's result
    for name in G.CELLS:
        z, pos, cell, pbc, radius = G.cell_case(name)
        p2 = np.stack([pos, pos])
        for mn in ((50, 2000) if name == "Cap" else (None, 20)):
            eng.set_system(z, radius=radius, max_neigh=mn)
            for how in ("set_cell", "set_cells"):
                eng.set_cell(cell, pbc) if how == "set_cell" else eng.set_cells(np.stack([cell, cell]), pbc)
                for dbl in (False, True):
                    graph_line(f"cells {name} cap {mn} {how}", eng, p2, dbl)
    eng.set_cell(None)
    # distinct per-image cells: in one chunk, and one image per chunk (a non-zero first image reaches the kernels)
    for fam in CC.FAMILIES:
        z, imgs, cells, pbc = CC.family(fam)
        eng.set_system(z)
        eng.set_cells(cells, pbc)
        for chunk in (None, "1"):
            if chunk:
                os.environ["UMX_MAX_CHUNK_IMAGES"] = chunk
            for dbl in (False, True):
                graph_line(f"family {fam} {len(cells)} cells{' chunk1' if chunk else ''}", eng, imgs, dbl)
            os.environ.pop("UMX_MAX_CHUNK_IMAGES", None)
    eng.set_cell(None)
    # pinned graph, evaluated on displaced geometries
    z, pos = G.seam_case(65)
    for mn in (None, 8):
        eng.set_system(z, radius=6.0, max_neigh=mn)
        for dbl in (False, True):
            eng.pin_graph(pos, double_positions=dbl)
            graph_line(f"pinned open seam 65 cap {mn}", eng, np.stack([pos, displaced(pos)]), dbl)
            eng.unpin_graph()
    z, imgs, cells, pbc = CC.family("triclinic")
    for mn in (None, 7):                                       # 7: the pinning fill truncates (TOUT with TRUNC)
        eng.set_system(z, max_neigh=mn)
        for dbl in (False, True):
            eng.set_cell(cells[0], pbc)
            eng.pin_graph(imgs[0], double_positions=dbl)
            graph_line(f"pinned one cell cap {mn}", eng, np.stack([imgs[0], displaced(imgs[0])]), dbl)
            eng.set_cell(cells[4], pbc)                        # the strained cell under the pin
            graph_line(f"pinned one cell cap {mn}, re-bound to the strained cell", eng, np.stack([imgs[4], displaced(imgs[4])]), dbl)
            eng.unpin_graph()
            eng.set_cells(cells[:1], pbc)
            eng.pin_graph(imgs[0], double_positions=dbl)
            eng.set_cells(cells, pbc)
            for chunk in (None, "1"):
                if chunk:
                    os.environ["UMX_MAX_CHUNK_IMAGES"] = chunk
                graph_line(f"pinned per-image cells cap {mn}{' chunk1' if chunk else ''}", eng, displaced(imgs), dbl)
                os.environ.pop("UMX_MAX_CHUNK_IMAGES", None)
            eng.unpin_graph()
    eng.close()


if __name__ == "__main__":
    if "graph" not in sys.argv[1:]:
        main()
    if "plans" not in sys.argv[1:]:
        graph_main()
