"""What float32 positions cost in accuracy, and what float64 positions cost in time (profiles/double_positions.txt).

    python tools/double_positions_measure.py cpu [atoms ...]        the float64 checker alone, no GPU (default: 14 and 500 atoms)
    python tools/double_positions_measure.py gpu [--tree DIR] [--entries float,double] [--steps N] [--warmup W]
    python tools/double_positions_measure.py isa --tree DIR         kernel by kernel, this build's device code against DIR's (no GPU)

cpu: for a synthetic cluster x and the rigid translations t = 0, 64 and 1024 A along (1, 1, 1) / sqrt(3), the checker (oracle/, float64
arithmetic throughout) evaluated at float32(x + t) against the same checker at x + t:  |dE| and max|dF|.  This is the error the engine's
float entries inherit from rounding the caller's geometry at the door, before any of their own arithmetic; the engine is not involved.

gpu: the step time of a c3-shaped batch (2000 atoms, 16 images, energies and forces, host-pointer entries, default precision mode)
through the float entry and through the double entry of ONE engine, steps interleaved float, double, float, ... after a warm-up, so
that clock and temperature drift hits both alike; median, minimum and maximum over the steps.  ``--tree DIR`` imports the package (and
its built library) from another checkout -- the parent commit's, for its float entry (``--entries float``: it has no other).  Wall
clock around the synchronous host entry: host-to-device copy, graph, model, copy back -- so "double - float" holds the copy of twice the
position bytes (768 kB against 384 kB for this batch) together with the three graph kernels; it is the difference a caller of the host
entry sees, not a kernel time.  The difference is reported as the difference of the medians and, step by step (float step i against the
double step i that follows it), as median, minimum and maximum.  No GPU: the engine raises, nothing is reported.

isa: the gfx950 code object of this checkout's built library against that of the checkout DIR (``build.device_disassembly`` of both),
kernel by kernel: which kernels have the same instructions line for line (under the same name, or under a new one: a kernel that gained
a template parameter), which differ, which exist on one side only.  This is what
"the float entries run the parent's device code" rests on, and the first place to look when the float entry's time moves.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cpu(sizes):
    sys.path.insert(0, ROOT)
    import torch
    from oracle.escn_md_oracle import Oracle
    from pdb2reaction_amd import synth, weights as W

    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    orc = Oracle(W.make_synthetic_weights(0))
    u = np.ones(3) / np.sqrt(3.0)
    for n in sizes:
        z, x = synth.make_cluster(n, seed=4)
        for t in (0.0, 64.0, 1024.0):
            p = x + t * u
            t0 = time.perf_counter()
            e64, f64 = orc.energy_forces(z, p)
            e32, f32 = orc.energy_forces(z, p.astype(np.float32).astype(np.float64))
            dr = float(np.abs(p.astype(np.float32).astype(np.float64) - p).max())
            print(f"[double_positions_measure cpu] {n:4d} atoms  t = {t:6.0f} A  max|float32(x+t) - (x+t)| = {dr:.3e} A  "
                  f"|dE| = {abs(e32 - e64):.3e} eV  max|dF| = {float(np.abs(f32 - f64).max()):.3e} eV/A  max|F| = {float(np.abs(f64).max()):.3f} eV/A  "
                  f"({time.perf_counter() - t0:.1f} s)", flush=True)


def gpu(tree, entries, steps, warmup):
    sys.path.insert(0, os.path.abspath(tree) if tree else ROOT)
    from pdb2reaction_amd import synth, weights as W
    from pdb2reaction_amd.engine import Engine

    z, imgs, _ = synth.make_images(2000, 16)
    p = {"float": np.ascontiguousarray(imgs, dtype=np.float32), "double": np.ascontiguousarray(imgs, dtype=np.float64)}
    eng = Engine(0)
    eng.load_weights(W.make_synthetic_weights(0))
    eng.set_system(z)

    def step(entry):
        t0 = time.perf_counter()
        e, f = eng.energy_forces(p[entry], **({"double_positions": True} if entry == "double" else {}))
        return (time.perf_counter() - t0) * 1e3, e

    for _ in range(warmup):
        for entry in entries:
            step(entry)
    ms, last = {entry: [] for entry in entries}, {}
    for _ in range(steps):
        for entry in entries:
            t, last[entry] = step(entry)
            ms[entry].append(t)
    where = os.path.dirname(sys.modules["pdb2reaction_amd"].__file__)
    print(f"[double_positions_measure gpu] package {where}, library digest {eng.lib.umx_build_digest().decode()[:12]}, mode {eng.precision_mode()}, "
          f"2000 atoms x 16 images, {eng.graph_stats()[0]} directed edges, {warmup} warm-up + {steps} timed steps per entry, interleaved")
    for entry in entries:
        v = ms[entry]
        print(f"[double_positions_measure gpu]   {entry:6s} entry: median {statistics.median(v):8.2f} ms  min {min(v):8.2f}  max {max(v):8.2f}  "
              f"(E[0] = {last[entry][0]:.6f} eV)")
    if len(entries) == 2:
        d = statistics.median(ms["double"]) - statistics.median(ms["float"])
        pair = [b - a for a, b in zip(ms["float"], ms["double"])]             # step i of one entry against step i of the other, back to back
        print(f"[double_positions_measure gpu]   double - float (medians): {d:+.2f} ms = {100.0 * d / statistics.median(ms['float']):+.3f} %;  "
              f"step by step: median {statistics.median(pair):+.2f} ms  min {min(pair):+.2f}  max {max(pair):+.2f};  "
              f"max |E_double - E_float| = {float(np.abs(last['double'] - last['float']).max()):.3e} eV")
    eng.close()


def kernels_of(lib_path):
    """{kernel name: its instructions, one string per line, addresses and encodings dropped} of a built library's gfx950 code object."""
    import re
    from pdb2reaction_amd.build import device_disassembly

    out, name = {}, None
    for line in device_disassembly(lib_path).splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.strip():
            out[name].append(line.split("//")[0].strip())
    return out


def isa(tree):
    sys.path.insert(0, ROOT)
    rel = os.path.join("pdb2reaction_amd", "libumx.so")
    new, old = kernels_of(os.path.join(ROOT, rel)), kernels_of(os.path.join(os.path.abspath(tree), rel))
    both = sorted(set(new) & set(old))
    differ = [k for k in both if new[k] != old[k]]
    print(f"[double_positions_measure isa] {len(new)} kernels in this build, {len(old)} in the other; {len(both)} in both, "
          f"{len(both) - len(differ)} of them with the same instructions line for line, {len(differ)} that differ")
    for k in differ:
        print(f"[double_positions_measure isa]   differs: {k}  ({len(old[k])} -> {len(new[k])} instructions)")
    # a kernel that gained a template parameter has another mangled name: pair the leftovers by their instructions
    left = sorted(set(new) - set(old))
    for k in sorted(set(old) - set(new)):
        twin = next((j for j in left if new[j] == old[k]), None)
        if twin:
            left.remove(twin)
            print(f"[double_positions_measure isa]   same instructions under a new name: {k} -> {twin}  ({len(old[k])} instructions)")
        else:
            print(f"[double_positions_measure isa]   only in the other build: {k}")
    for k in left:
        print(f"[double_positions_measure isa]   only in this build: {k}  ({len(new[k])} instructions)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="what", required=True)
    c = sub.add_parser("cpu")
    c.add_argument("atoms", nargs="*", type=int, default=[14, 500])
    g = sub.add_parser("gpu")
    g.add_argument("--tree", default=None)
    g.add_argument("--entries", default="float,double")
    g.add_argument("--steps", type=int, default=20)
    g.add_argument("--warmup", type=int, default=3)
    i = sub.add_parser("isa")
    i.add_argument("--tree", required=True)
    a = ap.parse_args()
    if a.what == "cpu":
        cpu(a.atoms)
    elif a.what == "isa":
        isa(a.tree)
    else:
        gpu(a.tree, a.entries.split(","), a.steps, a.warmup)


if __name__ == "__main__":
    main()
