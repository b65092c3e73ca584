"""Workload of profiles/per_image_cells.txt: 16 images of the 125-atom ``cubic`` case of the periodic tests, evaluated with one shared
cell (``set_cell``) or with 16 identical per-image cells (``set_cells``); or the host time of one ``set_cells`` call.

    rocprofv3 --kernel-trace --stats -d <dir> -o <name> --output-format csv -- python tools/per_image_cells_profile.py cell  [evaluations]
    rocprofv3 --kernel-trace --stats -d <dir> -o <name> --output-format csv -- python tools/per_image_cells_profile.py cells [evaluations]
    python tools/per_image_cells_profile.py host
    python tools/per_image_cells_profile.py stats <name>_kernel_stats.csv <evaluations + 1>

``--tree DIR`` (last two arguments) takes the package and the test helpers from another checkout (the parent commit: mode ``cell`` only).
``stats`` sums the periodic graph kernels (k_wrap_cell, k_graph_count<P, Cells<P>>, k_graph_fill<., ., P, Cells<P>>; on a tree from before
csrc/umx_graph.h: k_graph_count<true, ...>, k_graph_fill<., true, ...>) of a kernel-stats file."""
import csv
import os
import re
import sys
import time

import numpy as np

args = sys.argv[1:]
tree = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in args:
    tree = os.path.abspath(args[args.index("--tree") + 1])
    args = args[:args.index("--tree")]
sys.path[:0] = [tree, os.path.join(tree, "tests")]

# the periodic instantiations take Cells<P> (csrc/umx_graph.h); before the graph stage had its own header they were <true, ...> / <., true, ...>
PERIODIC = re.compile(r"k_wrap_cell|k_graph_(count|fill)<[^()]*umx::Cells<|k_graph_count<true|k_graph_fill<(true|false), true")


def stats(path, evaluations):
    total, rows = 0.0, []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if PERIODIC.search(row["Name"]):
                name = re.search(r"k_\w+[^(]*", row["Name"]).group(0).replace("umx::", "")
                rows.append((name, int(row["Calls"]), float(row["TotalDurationNs"])))
                total += float(row["TotalDurationNs"])
    for name, calls, ns in sorted(rows):
        print(f"    {name:38s} {calls:5d} calls {ns / evaluations / 1e3:9.2f} us per evaluation")
    print(f"    periodic graph kernels                             {total / evaluations / 1e3:9.2f} us per evaluation")


def main():
    mode = args[0]
    if mode == "stats":
        return stats(args[1], int(args[2]))
    from stress_oracle import make_case
    from pdb2reaction_amd import weights as W
    from pdb2reaction_amd.engine import Engine

    z, p32, cell, pbc = make_case("cubic", k=16)
    eng = Engine(0)
    eng.load_weights(W.make_synthetic_weights(0))
    eng.set_system(z)
    try:
        if mode == "host":
            for k in (16, 64):
                cells = np.stack([cell * (1.0 + 0.001 * i) for i in range(k)])
                eng.set_cells(cells, pbc)
                t = []
                for _ in range(20):
                    t0 = time.perf_counter()
                    eng.set_cells(cells, pbc)
                    t.append(time.perf_counter() - t0)
                t1 = []
                for _ in range(20):
                    t0 = time.perf_counter()
                    eng.set_cell(cell, pbc)
                    t1.append(time.perf_counter() - t0)
                print(f"set_cells K = {k}: median {np.median(t) * 1e6:.1f} us, smallest {min(t) * 1e6:.1f} us of 20 calls (idle stream);  "
                      f"set_cell: median {np.median(t1) * 1e6:.1f} us")
            return
        n = int(args[1]) if len(args) > 1 else 20
        if mode == "cells":
            eng.set_cells(np.stack([cell] * 16), pbc)
        else:
            eng.set_cell(cell, pbc)
        e = None
        for _ in range(n + 1):                                  # the first one is the warm-up; it is profiled with the others
            e, f = eng.energy_forces(p32)
        print(f"{mode}: {n + 1} evaluations, E[0] = {e[0]:.6f} eV, shifts {eng.last_graph_shifts()}, (edges, maxdeg) {eng.graph_stats()}")
    finally:
        eng.close()


main()
