"""Fingerprint of every kind of launch plan: one line per configuration with the sha256 of the energies, the forces, the virial where
asked and, with captures on, of every debug capture in name order.  A host-code refactor must leave every line as it was: run it on both
trees (python tools/gpu_plan_fingerprint.py > out.txt) and compare the files.  An engine error prints as the line's result."""
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


if __name__ == "__main__":
    main()
