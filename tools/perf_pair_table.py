#!/usr/bin/env python3
"""What the tabulated pair potential costs next to the harmonic repulsion it generalises (docs/HISTORY.md): time per call of
pse_pair_repulsion, pse_pair_repulsion_virial, pse_pair_table with observables and pse_pair_table without (out8 = NULL) on the same
uniform random positions, the table being the harmonic repulsion itself at `--width` nodes.  Each figure is the time between one pair
of events around `--calls` back-to-back calls (sort + cell walk, as a stepping loop pays them) after three warm-up calls; `--windows`
windows per variant, taken alternately in one process.  Prints one JSON line.
The pair exclusions ride along: `table_excl` (with observables, against `table`) and `repulsion_excl` (forces only, against
`repulsion`) take an exclusion object of a chain topology over the particles -- consecutive indices bonded, the sets 1-2 + 1-3 + 1-4:
six entries per row; on uniform random positions next to none of those pairs is in range (a handful of three million: `npairs_excl`
against `npairs`), so every in-range pair pays a lookup and next to none is dropped -- and `*_excl_empty` an object with one pair,
whose rows are empty for all particles but two: what the exclusion kernels cost a run that excludes nothing; its forces and sums must
equal the plain ones bit for bit (`excl_empty_bit_identical`).

  python tools/perf_pair_table.py [--n 1000000] [--phi 0.2] [--width 1024] [--calls 20] [--windows 4]"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--phi", type=float, default=0.2)
    ap.add_argument("--k", type=float, default=40.0)
    ap.add_argument("--sigma", type=float, default=2.0)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=4)
    a = ap.parse_args()
    import torch
    import pse_amd
    n, k, sigma = a.n, a.k, a.sigma
    L = (4.0 * math.pi * n / (3.0 * a.phi)) ** (1.0 / 3.0)
    p4 = np.zeros((n, 4))
    p4[:, :3] = np.random.default_rng(5).uniform(-0.5 * L, 0.5 * L, size=(n, 3))
    pos = torch.tensor(p4, dtype=torch.float64, device="cuda")
    r = np.arange(a.width) * (sigma / (a.width - 1))
    table = torch.tensor(np.stack([0.5 * k * (sigma - r) ** 2, k * (sigma - r)], axis=1), dtype=torch.float64, device="cuda")
    eng = pse_amd.Engine(n, (L, L, L, 0.0))
    names = ("repulsion", "repulsion_virial", "table", "table_forces_only", "table_excl", "repulsion_excl", "table_excl_empty", "repulsion_excl_empty")
    force = {name: torch.zeros((n, 4), dtype=torch.float64, device="cuda") for name in names}
    out = {name: torch.zeros(8, dtype=torch.float64, device="cuda") for name in ("repulsion_virial", "table", "table_excl", "table_excl_empty")}
    idx = np.arange(n)
    chain = eng.exclusions(np.concatenate([np.stack([idx[:-q], idx[q:]], axis=1) for q in (1, 2, 3)]))
    empty = eng.exclusions([[0, 1]])
    variants = {
        "repulsion": lambda: eng.pair_repulsion(pos, force["repulsion"], k, sigma, accumulate=False),
        "repulsion_virial": lambda: eng.pair_repulsion_virial(pos, force["repulsion_virial"], k, sigma, accumulate=False, out=out["repulsion_virial"]),
        "table": lambda: eng.pair_table(pos, force["table"], table, 0.0, sigma, accumulate=False, out=out["table"]),
        "table_forces_only": lambda: eng.pair_table(pos, force["table_forces_only"], table, 0.0, sigma, accumulate=False, observables=False),
        "table_excl": lambda: eng.pair_table(pos, force["table_excl"], table, 0.0, sigma, accumulate=False, out=out["table_excl"], exclusions=chain),
        "repulsion_excl": lambda: eng.pair_repulsion(pos, force["repulsion_excl"], k, sigma, accumulate=False, exclusions=chain),
        "table_excl_empty": lambda: eng.pair_table(pos, force["table_excl_empty"], table, 0.0, sigma, accumulate=False, out=out["table_excl_empty"],
                                                   exclusions=empty),
        "repulsion_excl_empty": lambda: eng.pair_repulsion(pos, force["repulsion_excl_empty"], k, sigma, accumulate=False, exclusions=empty),
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
    f0 = force["repulsion"][:, :3]
    o_rep, o_tab = out["repulsion_virial"].cpu().numpy(), out["table"].cpu().numpy()
    res = {
        "n": n, "phi": a.phi, "k": k, "sigma": sigma, "width": a.width, "calls": a.calls,
        "ms_per_call": {name: [round(x, 4) for x in v] for name, v in ms.items()},
        "median_ms": {name: round(v, 4) for name, v in med.items()},
        "table_over_repulsion_virial": round(med["table"] / med["repulsion_virial"], 3),
        "table_forces_only_over_repulsion": round(med["table_forces_only"] / med["repulsion"], 3),
        "table_excl_over_table": round(med["table_excl"] / med["table"], 3),
        "repulsion_excl_over_repulsion": round(med["repulsion_excl"] / med["repulsion"], 3),
        "table_excl_empty_over_table": round(med["table_excl_empty"] / med["table"], 3),
        "repulsion_excl_empty_over_repulsion": round(med["repulsion_excl_empty"] / med["repulsion"], 3),
        "npairs_excl": float(out["table_excl"][7]),
        "excl_empty_bit_identical": {"table": bool(torch.equal(force["table_excl_empty"], force["table"]) and torch.equal(out["table_excl_empty"], out["table"])),
                                     "repulsion": bool(torch.equal(force["repulsion_excl_empty"], force["repulsion"]))},
        "max_force_difference": {name: float((force[name][:, :3] - f0).abs().max()) for name in ("table", "table_forces_only")},
        "max_force": float(f0.abs().max()),
        "npairs": [float(o_rep[7]), float(o_tab[7])],
        "U": [float(o_rep[0]), float(o_tab[0])],
        "U_bound": float(o_rep[7] * k * (sigma / (a.width - 1)) ** 2 / 8.0),
        "max_W_difference": float(np.abs(o_rep[1:7] - o_tab[1:7]).max()),
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
