"""What the virial costs on the graph-parallel route: the device time of the two reduction kernels in a two-engine evaluation of one
image, with and without the virial (profiles/gp_stress.txt).

    python tools/gp_stress_measure.py [evaluations]              both traces, each in a child process of its own
    python tools/gp_stress_measure.py trace virial|plain [n]     the workload only: what the kernel trace wraps

Workload: image 0 of the periodic cube of DESIGN.md section 4a (tools/periodic_graph_profile.py: 2000 atoms in a 27.1 A cube, pbc in all
directions, default mode bf16x3) over a ``LocalEnginePool`` of two engines, BOTH ON DEVICE 0: no number here involves a second physical
device.  Kernel time: ``rocprofv3 --kernel-trace --stats`` around a run of its own -- no counters in that run, and no step time is taken
from it (tracing slows the host).  No GPU: the engine raises, nothing is reported.
"""
import csv
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("k_virial_slab", "k_virial_image")


def trace_workload(virial, n_eval):
    from periodic_graph_profile import EDGE, periodic_cube
    from pdb2reaction_amd import weights as W
    from pdb2reaction_amd.parallel import LocalEnginePool

    z, imgs = periodic_cube(n_images=1)
    p32 = np.asarray(imgs[0], dtype=np.float32)
    with LocalEnginePool.create([0, 0], W.make_synthetic_weights(0)) as pool:
        pool.set_system(z)
        pool.set_cell(np.eye(3) * EDGE, True)
        for _ in range(n_eval):
            if virial:
                e, f, w = pool.energy_forces_virial(p32, graph_parallel=True)
            else:
                e, f = pool.energy_forces(p32)
        assert pool.last_route == "graph-parallel"
        edges = [eng.graph_stats()[0] for eng in pool.engines]
        print(f"[gp_stress_measure trace] {n_eval} evaluations {'with' if virial else 'without'} the virial, {len(z)} atoms, directed edges per engine "
              f"{edges}, mode {pool.precision_mode()}, E = {e[0]:.6f} eV" + (f", W_xx = {w[0, 0, 0]:+.6f} eV" if virial else ""), flush=True)


def kernel_times(virial, n_eval):
    """rocprofv3 around a fresh child (the program goes after --); the stats CSV is read, the trace itself is not kept."""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "gp_stress", "--",
               sys.executable, os.path.abspath(__file__), "trace", "virial" if virial else "plain", str(n_eval)]
        print("[gp_stress_measure] " + " ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, timeout=600)
        found = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError("rocprofv3 left no kernel_stats.csv")
        rows = list(csv.DictReader(open(found[0])))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    label = "with the virial" if virial else "without"
    print(f"[gp_stress_measure] {label}: all kernels of both engines {total / n_eval / 1e6:.2f} ms per evaluation ({n_eval} evaluations in the trace)")
    both = 0.0
    for k in KERNELS:
        hit = [r for r in rows if k in r["Name"]]
        if not virial:
            if hit:
                raise RuntimeError(f"{k} ran in an evaluation without a virial")
            print(f"[gp_stress_measure]   {k:16s}    0 calls")
            continue
        if not hit:
            raise RuntimeError(f"{k} is not in the kernel trace")
        ns, calls = sum(float(r["TotalDurationNs"]) for r in hit), sum(int(r["Calls"]) for r in hit)
        both += ns
        print(f"[gp_stress_measure]   {k:16s} {calls:4d} calls   {ns / n_eval / 1e3:8.1f} us per evaluation (both engines)   {ns / calls / 1e3:8.1f} us per call")
    if virial:
        print(f"[gp_stress_measure]   both              {both / n_eval / 1e3:8.1f} us per evaluation = {100.0 * both / total:.4f} % of the kernel time")
    return total / n_eval


def main():
    args = sys.argv[1:]
    if args and args[0] == "trace":
        trace_workload(args[1] == "virial", int(args[2]) if len(args) > 2 else 3)
        return
    n_eval = int(args[0]) if args else 3
    # this process never opens the GPU: each trace is a fresh child, one after the other
    plain = kernel_times(False, n_eval)
    withv = kernel_times(True, n_eval)
    print(f"[gp_stress_measure] kernel time per evaluation: {plain / 1e6:.2f} ms without, {withv / 1e6:.2f} ms with the virial")


if __name__ == "__main__":
    main()
