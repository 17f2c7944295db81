"""What a sample of the static structure factor costs, against the formulation a user writes without it: wall time per call, by stream
events, of pse_structure_factor_accumulate and of a torch baseline in the same process on the benchmark's configuration -- N
particles at volume fraction phi, uniform random positions -- for two mode lists and one and two types:
  axes        analyze.axis_modes(256): 768 modes on three lines, the recurrence's best case
  scattered   4096 seeded modes with |m_i| <= 256: no two on a line, one reduced-phase evaluation per (particle, mode) and more
  torch_*     the same rho in torch: chunks of the (N, nk) table of phases pos_frac @ modes.T, cos and sin, summed over the particles
              (16 N nk bytes of traffic and more; the phase is NOT reduced exactly, which is good enough at these |m| and |s| <= 1/2)
Each figure is the time between one pair of events around `--calls` back-to-back calls after three warm-up calls; `--windows`
windows per variant, taken alternately in one process.  The baseline's rho must agree with the kernel's within the bound of the
tests, tol(m) = N (2e-14 + 4e-15 s_max sum |m_i|) on top of the baseline's own phase rounding N 2 pi 2^-52 sum |m_i| s_max.
Prints one JSON line.

  python tools/perf_structure_factor.py [--n 1000000] [--phi 0.1] [--calls 5] [--windows 5] [--only axes1,torch_axes1]"""
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
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=65536, help="particles per chunk of the torch baseline")
    ap.add_argument("--only", default="", help="comma-separated variants to run (a kernel trace then shows one variant per kernel name)")
    a = ap.parse_args()
    import torch
    import pse_amd
    from pse_amd import analyze
    n = a.n
    L = (4.0 * math.pi * n / (3.0 * a.phi)) ** (1.0 / 3.0)
    box = (L, L, L, 0.0)
    p4 = np.zeros((n, 4))
    p4[:, :3] = np.random.default_rng(5).uniform(-0.5 * L, 0.5 * L, size=(n, 3))
    pos = torch.tensor(p4, dtype=torch.float64, device="cuda")
    eng = pse_amd.Engine(n, box)
    types = {1: None, 2: np.random.default_rng(7).integers(0, 2, n)}
    lists = {"axes": analyze.axis_modes(256), "scattered": np.random.default_rng(9).integers(-256, 257, size=(4096, 3)).astype(np.int32)}
    frac = pos[:, :3] / L                                   # (tilt 0)
    masks = {1: [None], 2: [torch.tensor(types[2] == t, device="cuda") for t in (0, 1)]}

    objs, rho, variants = {}, {}, {}
    for lname, modes in lists.items():
        mt = torch.tensor(modes.T.astype(np.float64), device="cuda")
        for nt in (1, 2):
            key = f"{lname}{nt}"
            objs[key] = eng.structure_factor(types[nt], nt, modes)
            rho[key] = torch.zeros((nt, len(modes), 2), dtype=torch.float64, device="cuda")
            rho["torch_" + key] = torch.zeros((nt, len(modes), 2), dtype=torch.float64, device="cuda")
            variants[key] = lambda key=key: eng.structure_factor_accumulate(pos, objs[key], rho=rho[key])

            def baseline(key=key, mt=mt, nt=nt):
                out = rho["torch_" + key]
                out.zero_()
                for c0 in range(0, n, a.chunk):
                    ph = (2.0 * math.pi) * (frac[c0:c0 + a.chunk] @ mt)
                    c, s = torch.cos(ph), torch.sin(ph)
                    for t, mask in enumerate(masks[nt]):
                        if mask is None:
                            out[t, :, 0] += c.sum(dim=0)
                            out[t, :, 1] -= s.sum(dim=0)
                        else:
                            w = mask[c0:c0 + a.chunk].to(torch.float64)
                            out[t, :, 0] += w @ c
                            out[t, :, 1] -= w @ s
            variants["torch_" + key] = baseline
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
    res = {
        "n": n, "phi": a.phi, "L": L, "calls": a.calls, "modes": {k: int(len(v)) for k, v in lists.items()},
        "ms_per_call": {name: [round(x, 4) for x in v] for name, v in ms.items()},
        "median_ms": {name: round(v, 4) for name, v in med.items()},
        "min_ms": {name: round(min(v), 4) for name, v in ms.items()},
    }
    agree, ratios = {}, {}
    for key in objs:
        if key in variants and "torch_" + key in variants:
            m = np.abs(lists[key[:-1]]).sum(axis=1).astype(np.float64)
            bound = n * (2e-14 + 4e-15 * 0.5 * m) + n * 2.0 * math.pi * 2.0 ** -52 * 0.5 * m
            err = (rho[key] - rho["torch_" + key]).abs().amax(dim=(0, 2)).cpu().numpy()
            agree[key] = {"worst_error_over_bound": float((err / bound).max()), "within": bool((err <= bound).all())}
            ratios[f"torch_over_{key}"] = round(med["torch_" + key] / med[key], 2)
    res["baseline_agrees"], res["ratios"] = agree, ratios
    print(json.dumps(res))


if __name__ == "__main__":
    main()
