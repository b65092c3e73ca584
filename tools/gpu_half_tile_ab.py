"""A/B of the half-height split-precision GEMMs (UMX_GEMM_HALF, umx_launch.h choose_pl), alternating settings inside ONE process on one GPU:

    python3 tools/gpu_half_tile_ab.py [rounds [settings [configs]]]     # default: 3 rounds of UMX_GEMM_HALF = 0,1,2,3,4,5 on c3,c3-shard

Per setting and round: wall time of the device-resident batched E+F after two warm-up calls (as tools/gpu_r5_ab.py) and the bitwise comparison of
E and F against the very first run.  The repeats of one setting over the rounds are the A/A spread the gains are judged against.  In round 0
one more evaluation runs with the HIP-event brackets on and its per-launch GEMM times (UMX_PROFILE_DUMP) are printed per shape.
"""
import os
import sys
import tempfile
import time
from collections import OrderedDict

import numpy as np

sys.path.insert(0, ".")
from pdb2reaction_amd import synth, weights as W  # noqa: E402
from pdb2reaction_amd.engine import Engine  # noqa: E402

WEIGHTS = W.make_synthetic_weights(0)
SETTINGS = tuple(sys.argv[2].split(",")) if len(sys.argv) > 2 else ("0", "1", "2", "3", "4", "5")
CONFIGS = {"c3": (2000, 16, 4), "c3-shard": (2000, 2, 12), "c2": (500, 12, 20), "c1": (50, 8, 40)}      # atoms, images, timed repeats


def run(n, k, reps, half, per_launch):
    os.environ["UMX_GEMM_HALF"] = half
    eng = Engine(0)
    eng.load_weights(WEIGHTS)
    z, imgs, _ = synth.make_images(n, k)
    eng.set_system(z)
    eng.reserve_images(k)
    eng.energy_forces(imgs)
    eng.energy_forces(imgs)
    t = time.perf_counter()
    for _ in range(reps):
        e, f = eng.energy_forces(imgs)
    ms = (time.perf_counter() - t) / reps * 1e3
    ne, _ = eng.graph_stats()
    shapes = None
    if per_launch:
        with tempfile.NamedTemporaryFile(suffix=".csv") as tmp:
            eng.profile_enable(True)
            eng.energy_forces(imgs)
            os.environ["UMX_PROFILE_DUMP"] = tmp.name
            eng.profile_read()
            os.environ.pop("UMX_PROFILE_DUMP")
            eng.profile_enable(False)
            shapes = OrderedDict()
            for line in open(tmp.name):
                p = line.split(",")
                key = tuple(int(v) for v in p[:7])
                if key[5] > 0:           # the split-precision plane GEMMs
                    c = shapes.setdefault(key, [0, 0.0])
                    c[0] += 1
                    c[1] += float(p[7])
    eng.close()
    os.environ.pop("UMX_GEMM_HALF")
    return ms, ne, e, f, shapes


rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
for name in (sys.argv[3].split(",") if len(sys.argv) > 3 else ("c3", "c3-shard")):
    n, k, reps = CONFIGS[name]
    ref, times, tables = None, {s: [] for s in SETTINGS}, {}
    for rnd in range(rounds):
        for half in SETTINGS:
            ms, ne, e, f, shapes = run(n, k, reps, half, rnd == 0)
            same = ""
            if ref is None:
                ref = (e.copy(), f.copy())
            else:
                same = f"  bitwise == first run: E {bool((e == ref[0]).all())} F {bool((f == ref[1]).all())}"
            times[half].append(ms)
            if shapes is not None:
                tables[half] = shapes
            print(f"{name}: UMX_GEMM_HALF={half} round {rnd}: {ms:.2f} ms per E+F of {k} images ({ne} edges){same}", flush=True)
    base = times["0"]
    print(f"{name}: A/A spread of UMX_GEMM_HALF=0 over {rounds} rounds: {max(base) - min(base):.2f} ms (mean {np.mean(base):.2f})")
    for half in SETTINGS[1:]:
        print(f"{name}: UMX_GEMM_HALF={half}: mean {np.mean(times[half]):.2f} ms, {np.mean(times[half]) - np.mean(base):+.2f} ms against 0 "
              f"(spread {max(times[half]) - min(times[half]):.2f})")
    print(f"{name}: per-launch GEMM times of one profiled E+F (ms per launch; M N K cplx prec: launches | UMX_GEMM_HALF = {' / '.join(SETTINGS)})")
    for key in tables["0"]:
        M, N, K, _, cplx, prec, _ = key
        cells = " / ".join(f"{tables[s][key][1] / tables[s][key][0]:8.3f}" for s in SETTINGS)
        total = " / ".join(f"{tables[s][key][1]:8.2f}" for s in SETTINGS)
        print(f"  {M:8d} {N:5d} {K:5d} {cplx} {prec:2d}: {tables['0'][key][0]:3d} | {cells} | sum {total}", flush=True)
