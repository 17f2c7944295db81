#!/usr/bin/env python3
"""What the bonded-force pass costs: time per call of pse_bond_forces with observables and without (out8 = NULL) on
`--n` beads in FENE chains of `--beads`, each figure the time between one pair of events around `--calls` back-to-back calls after
three warm-up calls; `--windows` windows per variant, taken alternately in one process.  With it the bytes the pass has to move at
least -- per particle one row offset (4), its row entries (8 each), its position (32), its force row read and written (64); the
partners' positions are neighbours' rows that the caches serve -- and that traffic over the time as a fraction of the 8 TB/s HBM
peak.  Prints one JSON line.

  python tools/perf_bonds.py [--n 1000000] [--beads 20] [--calls 20] [--windows 4]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--beads", type=int, default=20)
    ap.add_argument("--phi", type=float, default=0.1)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=4)
    a = ap.parse_args()
    import math
    import torch
    import pse_amd
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
    from polymer_solution import build_chains
    beads, nchains = a.beads, a.n // a.beads
    n = nchains * beads
    L = (4.0 * math.pi * n / (3.0 * a.phi)) ** (1.0 / 3.0)
    box = (L, L, L, 0.0)
    xyz, pairs = build_chains(nchains, beads, box, 2.0, seed=5)
    p4 = np.zeros((n, 4))
    p4[:, :3] = xyz
    pos = torch.tensor(p4, dtype=torch.float64, device="cuda")
    eng = pse_amd.Engine(n, box)
    bl = eng.bonds(pairs, kinds="fene", k=7.5, r0=3.0, n=n)
    force = {name: torch.zeros((n, 4), dtype=torch.float64, device="cuda") for name in ("observables", "forces_only")}
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    variants = {
        "observables": lambda: bl.forces(pos, force["observables"], accumulate=False, out=out),
        "forces_only": lambda: bl.forces(pos, force["forces_only"], accumulate=False, observables=False),
    }
    for call in variants.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(a.windows):
        for name, call in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                call()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.calls)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    nbytes = 4 * (n + 1) + 8 * 2 * len(pairs) + 32 * n + 64 * n
    o = out.cpu().numpy()
    res = {
        "n": n, "beads": beads, "nbonds": int(len(pairs)), "calls": a.calls,
        "ms_per_call": {name: [round(x, 4) for x in v] for name, v in ms.items()},
        "median_ms": {name: round(v, 4) for name, v in med.items()},
        "model_bytes": nbytes, "model_bytes_per_particle": round(nbytes / n, 1),
        "fraction_of_hbm_peak": {name: round(nbytes / (v * 1e-3) / HBM_PEAK, 3) for name, v in med.items()},
        "nbonds_acted": float(o[7]), "U": float(o[0]), "overstretched": bl.overstretched,
        "max_force_difference": float((force["observables"] - force["forces_only"]).abs().max()),
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
