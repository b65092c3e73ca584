"""What the virial costs: step time through ``energy_forces`` and through ``energy_forces_virial`` on the same build, and the device time
of the two reduction kernels (profiles/stress.txt).

    python tools/stress_measure.py [steps] [warmup]          both measurements, each in a child process of its own
    python tools/stress_measure.py time [steps] [warmup]     the step times only (this process)
    python tools/stress_measure.py trace [steps] [warmup]    the workload only: what the kernel trace wraps

Workload: the periodic cube of DESIGN.md section 4a (tools/periodic_graph_profile.py: 2000 atoms in a 27.1 A cube, pbc in all directions,
16 images, default mode bf16x3).  Step time: host wall clock around the host-pointer entries, which return after a stream synchronise;
the two paths ALTERNATE step by step after a warm-up of both, so drift of the machine reaches both alike; mean and smallest step of each.
Kernel time: ``rocprofv3 --kernel-trace --stats`` around a run of its own that calls ``energy_forces_virial`` only -- no counters in that
run, and no step time is taken from it (tracing slows the host).  No GPU: the engine raises, nothing is reported.
"""
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("k_virial_slab", "k_virial_image")


def workload():
    from periodic_graph_profile import EDGE, periodic_cube
    from pdb2reaction_amd import weights as W
    from pdb2reaction_amd.engine import Engine

    eng = Engine(0)
    eng.load_weights(W.make_synthetic_weights(0))
    z, imgs = periodic_cube()
    eng.set_system(z)
    eng.set_cell(np.eye(3) * EDGE, True)
    p32 = np.asarray(imgs, dtype=np.float32)
    eng.reserve_images(len(p32))
    return eng, p32


def time_steps(steps, warmup):
    eng, p32 = workload()
    for _ in range(warmup):
        e0, f0 = eng.energy_forces(p32)
        e1, f1, w = eng.energy_forces_virial(p32)
    assert np.array_equal(e0, e1) and f0.tobytes() == f1.tobytes(), "the virial entry changed energies or forces"
    t = {"energy_forces": [], "energy_forces_virial": []}
    for _ in range(steps):
        for name, fn in (("energy_forces", eng.energy_forces), ("energy_forces_virial", eng.energy_forces_virial)):
            t0 = time.perf_counter()
            fn(p32)
            t[name].append((time.perf_counter() - t0) * 1e3)
    edges, maxdeg = eng.graph_stats()
    print(f"[stress_measure] {p32.shape[1]} atoms x {p32.shape[0]} images, {edges} directed edges (max degree {maxdeg}), mode {eng.precision_mode()}, "
          f"{steps} alternating steps after {warmup} warm-up of both", flush=True)
    for name, v in t.items():
        print(f"[stress_measure] {name:22s} mean {np.mean(v):8.2f} ms   smallest {np.min(v):8.2f} ms   largest {np.max(v):8.2f} ms", flush=True)
    d = np.array(t["energy_forces_virial"]) - np.array(t["energy_forces"])
    print(f"[stress_measure] difference of the means {np.mean(d):+.2f} ms, of the smallest steps {np.min(t['energy_forces_virial']) - np.min(t['energy_forces']):+.2f} ms "
          f"(step-to-step spread of one path: {np.std(t['energy_forces']):.2f} ms)", flush=True)
    print(f"[stress_measure] W_xx of image 0: {w[0, 0, 0]:+.6f} eV, largest asymmetry {np.abs(w - np.swapaxes(w, 1, 2)).max():.2e} eV", flush=True)
    eng.close()


def trace_workload(steps, warmup):
    eng, p32 = workload()
    for _ in range(warmup + steps):
        eng.energy_forces_virial(p32)
    edges, _ = eng.graph_stats()
    print(f"[stress_measure trace] {warmup + steps} evaluations of {edges} directed edges each", flush=True)
    eng.close()


def kernel_times(steps, warmup):
    """rocprofv3 around a fresh child (the program goes after --); the stats CSV is read, the trace itself is not kept."""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "stress", "--",
               sys.executable, os.path.abspath(__file__), "trace", str(steps), str(warmup)]
        print("[stress_measure] " + " ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, timeout=900)
        found = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError("rocprofv3 left no kernel_stats.csv")
        rows = list(csv.DictReader(open(found[0])))
    n_eval = steps + warmup
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print(f"[stress_measure] all kernels {total / n_eval / 1e6:.1f} ms per evaluation ({n_eval} evaluations in the trace)")
    both = 0.0
    for k in KERNELS:
        hit = [r for r in rows if k in r["Name"]]
        if not hit:
            raise RuntimeError(f"{k} is not in the kernel trace")
        ns, calls = sum(float(r["TotalDurationNs"]) for r in hit), sum(int(r["Calls"]) for r in hit)
        both += ns
        print(f"[stress_measure]   {k:16s} {calls:4d} calls   {ns / n_eval / 1e3:8.1f} us per evaluation   {ns / calls / 1e3:8.1f} us per call")
    print(f"[stress_measure]   both              {both / n_eval / 1e3:8.1f} us per evaluation = {100.0 * both / total:.4f} % of the kernel time")


def main():
    args = sys.argv[1:]
    mode = args.pop(0) if args and args[0] in ("time", "trace") else "all"
    steps = int(args[0]) if len(args) > 0 else 5
    warmup = int(args[1]) if len(args) > 1 else 1
    if mode == "time":
        time_steps(steps, warmup)
    elif mode == "trace":
        trace_workload(steps, warmup)
    else:       # this process never opens the GPU: each measurement is a fresh child
        subprocess.run([sys.executable, os.path.abspath(__file__), "time", str(steps), str(warmup)], check=True, timeout=900)
        kernel_times(min(steps, 2), 1)


if __name__ == "__main__":
    main()
