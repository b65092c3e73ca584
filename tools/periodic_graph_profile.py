"""Step time and graph statistics of the periodic 2000-atom cube next to the open-boundary c3 image batch (profiles/periodic_graph.txt).

    python tools/periodic_graph_profile.py open|periodic [steps] [warmup]

The periodic workload: 2000 atoms at the BASELINE density (0.10 atoms / A^3) in a 27.1 A cube, pbc in all directions -- 2000 of the
13^3 sites of a jittered simple-cubic lattice commensurate with the cell -- 16 images with N(0, 0.02 A) noise, like c3 (2000-atom
cluster, 16 images).  Run under ``rocprofv3 --kernel-trace --stats`` (a run of its own) for the per-kernel times of the graph stage.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdb2reaction_amd import synth, weights as W           # noqa: E402
from pdb2reaction_amd.engine import Engine, workspace_bytes  # noqa: E402

EDGE = 27.1


def periodic_cube(n_atoms=2000, n_images=16, seed=1):
    rng = np.random.default_rng(seed)
    g = 13
    idx = np.stack(np.meshgrid(*[np.arange(g)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    idx = idx[np.sort(rng.choice(len(idx), size=n_atoms, replace=False))]
    pos = (idx + 0.5 + rng.uniform(-0.3, 0.3, size=idx.shape)) / g * EDGE
    z = rng.choice(np.array(synth.ELEMENT_Z, dtype=np.int32), size=n_atoms, p=np.array(synth.ELEMENT_P)).astype(np.int32)
    imgs = np.stack([pos + 0.02 * np.random.default_rng(seed + 1 + k).standard_normal(pos.shape) for k in range(n_images)])
    return z, imgs


def main():
    kind = sys.argv[1] if len(sys.argv) > 1 else "periodic"
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    eng = Engine(0)
    eng.load_weights(W.make_synthetic_weights(0))
    if kind == "periodic":
        z, imgs = periodic_cube()
        eng.set_system(z)
        eng.set_cell(np.eye(3) * EDGE, True)
    else:
        z, imgs, _ = synth.make_images(2000, 16)
        eng.set_system(z)
    p32 = np.asarray(imgs, dtype=np.float32)
    eng.reserve_images(len(p32))
    for _ in range(warmup):
        eng.energy_forces(p32)
    t0 = time.perf_counter()
    for _ in range(steps):
        e, f = eng.energy_forces(p32)
    dt = (time.perf_counter() - t0) / max(steps, 1)
    edges, maxdeg = eng.graph_stats()
    per_image = edges // len(p32)
    print(f"[{kind}] {len(z)} atoms x {len(p32)} images: step {dt * 1e3:.1f} ms ({steps} steps after {warmup} warm-up)  directed edges {edges} "
          f"({per_image / len(z):.1f} per atom, max degree {maxdeg})  lattice translations {eng.last_graph_shifts()}  "
          f"workspace per image {workspace_bytes(len(z), per_image, engine=eng) / 2**30:.2f} GiB  partitions {eng.last_partitions()}  "
          f"finite {bool(np.isfinite(e).all() and np.isfinite(f).all())}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
