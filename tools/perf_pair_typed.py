"""What the typed pair tables cost next to the plain table pass: wall time per call, by stream events, of pse_pair_table and
pse_pair_table_typed on the benchmark's configuration -- N particles at volume fraction phi, uniform random positions, a Morse table
of `--width` nodes on [0.7, 3) -- each with the eight observables and with forces only:
  table, table_forces_only        pse_pair_table
  typed1, typed1_forces_only      pse_pair_table_typed, ntypes = 1: the same table; what the kernel itself costs
  typed2, typed2_forces_only      ntypes = 2, random types, the same table three times: a stage of 3 x width entries (48 KB at width
                                  1000, half the workgroups per CU of the plain pass), one type load per pair in range
Each figure is the time between one pair of events around `--calls` back-to-back calls (sort + cell walk, as a stepping loop pays
them) after three warm-up calls; `--windows` windows per variant, taken alternately in one process.  The typed variants must give
the plain pass's forces and sums to rounding (`max_force_difference`, `npairs`).  On a build without the typed pass only the two
plain variants run, so that one script times the plain pass before and after.  Prints one JSON line.

  python tools/perf_pair_typed.py [--n 1000000] [--phi 0.1] [--width 1000] [--calls 20] [--windows 5]"""
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
    a = ap.parse_args()
    import torch
    import pse_amd
    n, rmin, rmax = a.n, 0.7, 3.0
    L = (4.0 * math.pi * n / (3.0 * a.phi)) ** (1.0 / 3.0)
    p4 = np.zeros((n, 4))
    p4[:, :3] = np.random.default_rng(5).uniform(-0.5 * L, 0.5 * L, size=(n, 3))
    pos = torch.tensor(p4, dtype=torch.float64, device="cuda")
    r = rmin + np.arange(a.width) * ((rmax - rmin) / (a.width - 1))
    e = np.exp(-2.0 * (r - 1.5))
    host = np.stack([5.0 * ((1.0 - e) ** 2 - 1.0), -20.0 * (1.0 - e) * e], axis=1)
    table = torch.tensor(host, dtype=torch.float64, device="cuda")
    eng = pse_amd.Engine(n, (L, L, L, 0.0))
    has_typed = hasattr(eng, "pair_table_typed")
    names = ["table", "table_forces_only"] + (["typed1", "typed1_forces_only", "typed2", "typed2_forces_only"] if has_typed else [])
    force = {name: torch.zeros((n, 4), dtype=torch.float64, device="cuda") for name in names}
    out = {name: torch.zeros(8, dtype=torch.float64, device="cuda") for name in names if not name.endswith("_forces_only")}
    variants = {
        "table": lambda: eng.pair_table(pos, force["table"], table, rmin, rmax, accumulate=False, out=out["table"]),
        "table_forces_only": lambda: eng.pair_table(pos, force["table_forces_only"], table, rmin, rmax, accumulate=False, observables=False),
    }
    if has_typed:
        one = (host, rmin, rmax)
        t1 = eng.typed_table(np.zeros(n, dtype=np.int64), {(0, 0): one})
        t2 = eng.typed_table(np.random.default_rng(7).integers(0, 2, n), {(0, 0): one, (0, 1): one, (1, 1): one})
        for name, t in (("typed1", t1), ("typed2", t2)):
            variants[name] = lambda name=name, t=t: eng.pair_table_typed(pos, force[name], t, accumulate=False, out=out[name])
            variants[name + "_forces_only"] = lambda name=name, t=t: eng.pair_table_typed(pos, force[name + "_forces_only"], t, accumulate=False,
                                                                                           observables=False)
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
    f0 = force["table"][:, :3]
    res = {
        "n": n, "phi": a.phi, "width": a.width, "rmin": rmin, "rmax": rmax, "calls": a.calls, "typed": has_typed,
        "ms_per_call": {name: [round(x, 4) for x in v] for name, v in ms.items()},
        "median_ms": {name: round(v, 4) for name, v in med.items()},
        "min_ms": {name: round(min(v), 4) for name, v in ms.items()},
        "npairs": {name: float(o[7]) for name, o in out.items()},
        "U": {name: float(o[0]) for name, o in out.items()},
        "max_force": float(f0.abs().max()),
        "max_force_difference": {name: float((force[name][:, :3] - f0).abs().max()) for name in names[1:]},
    }
    if has_typed:
        res["ratios"] = {"typed1_over_table": round(med["typed1"] / med["table"], 3),
                         "typed1_forces_only_over_table_forces_only": round(med["typed1_forces_only"] / med["table_forces_only"], 3),
                         "typed2_over_table": round(med["typed2"] / med["table"], 3),
                         "typed2_forces_only_over_table_forces_only": round(med["typed2_forces_only"] / med["table_forces_only"], 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
