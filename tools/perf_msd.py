"""What a sample of the displacement moments costs, against the formulation a user writes without it: wall time per call, by stream
events, of pse_msd_accumulate and of a torch baseline in the same process -- N particles at volume fraction phi, uniform random
positions and images, displacements of order one -- against 1, 8 and 64 origins per call:
  msd{K}        one pse_msd_accumulate against K stored origins, one type (msd64_t3: three types)
  torch{K}      the same sums in torch: the unwrapped positions once, then per origin the difference to a (3, N) table of stored
                unwrapped positions, the ten moments as a (10, N) table and its sum over the particles (per-type: a (ntypes, N) mask
                matrix times the table)
The pass is a stream over N (45 + 24 K) bytes -- pos, image and type once, three doubles per origin -- and `tb_per_s` is that over the
median time.  Each figure is the time between one pair of events around `--calls` back-to-back calls after three warm-up calls;
`--windows` windows per variant, taken alternately in one process.  The baseline's sums must agree with the kernel's to 1e-10
relative in the moments that do not cancel (dx^2, dy^2, dz^2, |d|^4).  Prints one JSON line.

  python tools/perf_msd.py [--n 1000000] [--phi 0.1] [--calls 5] [--windows 5] [--only msd64,torch64]"""
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
    ap.add_argument("--only", default="", help="comma-separated variants to run (a kernel trace then shows one variant per kernel name)")
    a = ap.parse_args()
    import torch
    import pse_amd
    n, K = a.n, 64
    L = (4.0 * math.pi * n / (3.0 * a.phi)) ** (1.0 / 3.0)
    rng = np.random.default_rng(5)
    p4 = np.zeros((n, 4))
    p4[:, :3] = rng.uniform(-0.5 * L, 0.5 * L, size=(n, 3))
    pos = torch.tensor(p4, dtype=torch.float64, device="cuda")
    image = torch.tensor(rng.integers(-2, 3, size=(n, 3)).astype(np.int32), device="cuda")
    strain = 1.3
    eng = pse_amd.Engine(n, (L, L, L, 0.0))
    types3 = rng.integers(0, 3, n)
    objs = {1: eng.msd_origins(None, 1, K), 3: eng.msd_origins(types3, 3, K)}

    def unwrap(p, im):
        imd = im.to(torch.float64)
        return torch.stack([p[:, 0] + imd[:, 0] * L + imd[:, 1] * (strain * L), p[:, 1] + imd[:, 1] * L, p[:, 2] + imd[:, 2] * L])

    planes = torch.empty((K, 3, n), dtype=torch.float64, device="cuda")     # the baseline's origins
    for k in range(K):
        old = pos.clone()
        old[:, :3] += torch.randn((n, 3), dtype=torch.float64, device="cuda") * (0.2 + 0.05 * k)
        for o in objs.values():
            eng.msd_store(old, image, o, k, strain)
        planes[k] = unwrap(old, image)
    masks = {1: None, 3: torch.stack([torch.tensor(types3 == t, device="cuda") for t in range(3)]).to(torch.float64)}

    sums, variants, bytes_per_call = {}, {}, {}
    for name, nt, k in (("msd1", 1, 1), ("msd8", 1, 8), ("msd64", 1, 64), ("msd64_t3", 3, 64)):
        sums[name] = torch.zeros((k, nt, 10), dtype=torch.float64, device="cuda")
        variants[name] = lambda name=name, nt=nt, k=k: eng.msd_accumulate(pos, image, objs[nt], strain, list(range(k)), list(range(k)), sums[name])
        bytes_per_call[name] = n * (45 + 24 * k)

        def baseline(name=name, nt=nt, k=k):
            out = sums["torch_" + name]
            ru = unwrap(pos, image)
            for q in range(k):
                d = ru - planes[q]
                r2 = (d * d).sum(dim=0)
                tab = torch.stack([d[0], d[1], d[2], d[0] * d[0], d[1] * d[1], d[2] * d[2], d[0] * d[1], d[0] * d[2], d[1] * d[2], r2 * r2])
                out[q] += tab.sum(dim=1)[None, :] if masks[nt] is None else masks[nt] @ tab.T
        sums["torch_" + name] = torch.zeros((k, nt, 10), dtype=torch.float64, device="cuda")
        variants["torch_" + name] = baseline
    if a.only:
        variants = {name: call for name, call in variants.items() if name in a.only.split(",")}
    for call in variants.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    ncalls = {name: 3 for name in variants}
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
            ncalls[name] += a.calls
    med = {name: float(np.median(v)) for name, v in ms.items()}
    res = {
        "n": n, "phi": a.phi, "L": L, "calls": a.calls,
        "ms_per_call": {name: [round(x, 4) for x in v] for name, v in ms.items()},
        "median_ms": {name: round(v, 4) for name, v in med.items()},
        "min_ms": {name: round(min(v), 4) for name, v in ms.items()},
        "bytes_per_call": {name: b for name, b in bytes_per_call.items() if name in variants},
        "tb_per_s": {name: round(b / (med[name] * 1e-3) / 1e12, 3) for name, b in bytes_per_call.items() if name in variants},
    }
    agree, ratios = {}, {}
    for name in bytes_per_call:
        if name in variants and "torch_" + name in variants:
            cols = [3, 4, 5, 9]                                # the moments that do not cancel: dx^2, dy^2, dz^2, |d|^4
            x, y = sums[name][..., cols] / ncalls[name], sums["torch_" + name][..., cols] / ncalls["torch_" + name]
            agree[name] = float(((x - y).abs() / y.abs()).max())
            ratios[f"torch_over_{name}"] = round(med["torch_" + name] / med[name], 2)
    res["baseline_relative_difference"], res["ratios"] = agree, ratios
    print(json.dumps(res))


if __name__ == "__main__":
    main()
