"""What a bond-order sample costs next to a pair-distance histogram over the same pairs: wall time per call, by stream events, of
pse_bond_order_compute with the degrees (4, 6) and of pse_pair_hist_accumulate with ONE bin on [0, rnb) -- the same cell walk over the
same pairs, without the harmonics -- on N particles at volume fraction phi, uniform random positions, one type.
  full        pse_bond_order_compute, every output: sort, type mirror, pass 1 of both degrees, pass 2 of both (q-bar; solid bonds on 6)
  pass1       the same call with nnb and q alone: sort, type mirror, pass 1 of both degrees
  hist1       pse_pair_hist_accumulate, one bin, rmax = rnb
Each figure is the time between one pair of events around `--calls` back-to-back calls (sort + cell walk, as a sampling loop pays
them) after three warm-up calls; `--windows` windows per variant, taken alternately in one process.  `--rnb 0` means rcut.  The stats
row of the last full call is printed with the mean number of neighbours, the means of q_6 and q-bar_6 and the histogram's count, which is
the number of neighbour pairs (half the sum of nnb).  Prints one JSON line.

  python tools/perf_bond_order.py [--n 1000000] [--phi 0.1] [--rnb 3.0] [--calls 10] [--windows 5] [--only full]"""
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
    ap.add_argument("--rnb", type=float, default=3.0, help="0: the real-space cutoff")
    ap.add_argument("--calls", type=int, default=10)
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
    rcut = eng.info()["rcut"]
    rnb = rcut if a.rnb == 0 else a.rnb
    shells = eng.bond_order_shells(None, 1, rnb, (4, 6))
    h1 = eng.pair_histogram(None, 1, 1, 0.0, rnb)
    nnb = torch.zeros(n, dtype=torch.int32, device="cuda")
    nconn = torch.zeros(n, dtype=torch.int32, device="cuda")
    q = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    qbar = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    stats = torch.zeros((1, 2), dtype=torch.int64, device="cuda")
    counts = torch.zeros((1, 1), dtype=torch.int64, device="cuda")
    variants = {"full": lambda: eng.bond_order(pos, shells, nnb=nnb, q=q, qbar=qbar, solid=(6, 0.7, 7), nconn=nconn, stats=stats),
                "pass1": lambda: eng.bond_order(pos, shells, nnb=nnb, q=q),
                "hist1": lambda: eng.pair_hist_accumulate(pos, h1, counts)}
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
    res = {"n": n, "phi": a.phi, "rnb": rnb, "rcut": rcut, "calls": a.calls,
           "ms_per_call": {name: [round(x, 4) for x in v] for name, v in ms.items()},
           "median_ms": {name: round(v, 4) for name, v in med.items()},
           "min_ms": {name: round(min(v), 4) for name, v in ms.items()}}
    if "full" in variants:
        res["stats"] = dict(zip(("members", "solid_like"), stats.cpu().ravel().tolist()))
        res["mean_neighbours"] = round(float(nnb.double().mean()), 3)
        res["mean_q6"], res["mean_qbar6"] = round(float(q[:, 1].mean()), 4), round(float(qbar[:, 1].mean()), 4)
    if "hist1" in variants:
        counts.zero_()
        variants["hist1"]()
        res["pairs"] = int(counts.sum())
        if "full" in variants:
            res["pairs_agree"] = bool(2 * res["pairs"] == int(nnb.long().sum()))
    if len(variants) == 3:
        res["full_over_hist1"] = round(med["full"] / med["hist1"], 3)
        res["pass1_over_hist1"] = round(med["pass1"] / med["hist1"], 3)
        res["pass2_over_pass1"] = round((med["full"] - med["pass1"]) / med["pass1"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
