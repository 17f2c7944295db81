"""What a sample of the pair-distance histogram costs next to the observables-only table pass: wall time per call, by stream events,
of pse_pair_hist_accumulate and of pse_pair_table with force = NULL and out8 set on the benchmark's configuration -- N particles at
volume fraction phi, uniform random positions -- both over the whole range of the cell list (rmax = rcut), so that they gather the
same pairs:
  table_obs        pse_pair_table, a Morse table of `--width` nodes on [0, rcut), observables only
  hist128, hist1   pse_pair_hist_accumulate, ntypes = 2 (random types), 128 bins and 1 bin
  hist36x227       ntypes = 8, 227 bins: 8172 counters, the most that fit (32 KB of LDS, one copy)
Each figure is the time between one pair of events around `--calls` back-to-back calls (sort + cell walk, as a sampling loop pays
them) after three warm-up calls; `--windows` windows per variant, taken alternately in one process.  The total of the one-bin
histogram must equal the table pass's npairs.  Prints one JSON line.

  python tools/perf_pair_hist.py [--n 1000000] [--phi 0.1] [--width 1000] [--calls 20] [--windows 5] [--only table_obs,hist128]"""
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
    ap.add_argument("--phi", type=float, default=0.1)
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated variants to run (a kernel trace then shows one variant per kernel name)")
    a = ap.parse_args()
    import torch
    import pse_amd
    n = a.n
    L = (4.0 * math.pi * n / (3.0 * a.phi)) ** (1.0 / 3.0)
    p4 = np.zeros((n, 4))
    p4[:, :3] = np.random.default_rng(5).uniform(-0.5 * L, 0.5 * L, size=(n, 3))
    pos = torch.tensor(p4, dtype=torch.float64, device="cuda")
    eng = pse_amd.Engine(n, (L, L, L, 0.0))
    rmax = eng.info()["rcut"]
    r = np.arange(a.width) * (rmax / (a.width - 1))
    e = np.exp(-2.0 * (r - 1.5))
    table = torch.tensor(np.stack([5.0 * ((1.0 - e) ** 2 - 1.0), -20.0 * (1.0 - e) * e], axis=1), dtype=torch.float64, device="cuda")
    out8 = torch.zeros(8, dtype=torch.float64, device="cuda")
    types = np.random.default_rng(7).integers(0, 2, n)
    hists = {"hist128": eng.pair_histogram(types, 2, 128, 0.0, rmax), "hist1": eng.pair_histogram(types, 2, 1, 0.0, rmax),
             "hist36x227": eng.pair_histogram(np.random.default_rng(7).integers(0, 8, n), 8, 227, 0.0, rmax)}
    counts = {name: torch.zeros((h.npt, h.nbins), dtype=torch.int64, device="cuda") for name, h in hists.items()}

    variants = {"table_obs": lambda: eng.pair_table(pos, None, table, 0.0, rmax, out=out8)}
    for name in hists:
        variants[name] = lambda name=name: eng.pair_hist_accumulate(pos, hists[name], counts[name])
    if a.only:
        variants = {name: call for name, call in variants.items() if name in a.only.split(",")}
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
    totals = {}
    for name in (h for h in hists if h in variants):   # one sample into zeroed counters: what the timed calls compute
        counts[name].zero_()
        variants[name]()
        totals[name] = int(counts[name].sum())
    res = {
        "n": n, "phi": a.phi, "rmax": rmax, "width": a.width, "calls": a.calls,
        "ms_per_call": {name: [round(x, 4) for x in v] for name, v in ms.items()},
        "median_ms": {name: round(v, 4) for name, v in med.items()},
        "min_ms": {name: round(min(v), 4) for name, v in ms.items()},
        "hist_pairs": totals,
    }
    if "table_obs" in variants:
        res["table_npairs"] = float(out8[7])
        res["pairs_agree"] = all(t == float(out8[7]) for t in totals.values())
        res["ratios"] = {f"{name}_over_table_obs": round(med[name] / med["table_obs"], 3) for name in variants if name != "table_obs"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
