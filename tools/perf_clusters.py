"""What a cluster labelling costs next to a pair-distance histogram over the same pairs: wall time per call, by stream events, of
pse_clusters_label (label, size, stats and hist all written) and of pse_pair_hist_accumulate with ONE bin on [0, rlink) -- the same
cell walk over the same pairs, without the union-find -- on N particles at volume fraction phi, uniform random positions, one type.
  clusters    pse_clusters_label: sort, type mirror, init, link, flatten, write
  hist1       pse_pair_hist_accumulate, one bin, rmax = rlink
  span        (with --span) pse_clusters_span on the same object, all eight outputs written: the union-find with image offsets
Each figure is the time between one pair of events around `--calls` back-to-back calls (sort + cell walk, as a sampling loop pays
them) after three warm-up calls; `--windows` windows per variant, taken alternately in one process.  `--rlink 0` means rcut.  The
stats row of the last labelling is printed with a host-side check of its labels and sizes (label[label] == label, size ==
bincount(label)[label]) and the histogram's count, which is the number of links.  `--host` adds a host baseline once, for the sense of
scale: the positions on the host, the pair list below rlink in the periodic cube (scipy's cKDTree), scipy's connected_components.
`--span` adds the third variant to the alternation, checks that its label, size and stats equal those of pse_clusters_label, and
prints its eight percolation words and the ratio span / clusters.
Prints one JSON line.

  python tools/perf_clusters.py [--n 1000000] [--phi 0.1] [--rlink 2.2] [--calls 20] [--windows 5] [--only clusters] [--host] [--span]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def host_baseline(p3, L, rlink):
    """Seconds for: positions to the host, the pair list below rlink in the periodic cube (cKDTree), connected_components."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    t0 = time.time()
    x = np.mod(p3 + 0.5 * L, L)
    pairs = cKDTree(x, boxsize=L).query_pairs(rlink, output_type="ndarray")
    t1 = time.time()
    n = len(x)
    ncomp, _ = connected_components(coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n)), directed=False)
    return {"pairs_s": round(t1 - t0, 3), "components_s": round(time.time() - t1, 3), "links": int(len(pairs)), "clusters": int(ncomp)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--phi", type=float, default=0.1)
    ap.add_argument("--rlink", type=float, default=2.2, help="0: the real-space cutoff")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated variants to run (a kernel trace then shows one variant per kernel name)")
    ap.add_argument("--host", action="store_true", help="also time the host baseline once")
    ap.add_argument("--span", action="store_true", help="also time pse_clusters_span (percolation), alternated with the others")
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
    rlink = rcut if a.rlink == 0 else a.rlink
    links = eng.clusters(None, 1, rlink)
    h1 = eng.pair_histogram(None, 1, 1, 0.0, rlink)
    label = torch.zeros(n, dtype=torch.int32, device="cuda")
    size = torch.zeros(n, dtype=torch.int32, device="cuda")
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    hist = torch.zeros(n, dtype=torch.int64, device="cuda")
    counts = torch.zeros((1, 1), dtype=torch.int64, device="cuda")
    variants = {"clusters": lambda: eng.cluster_label(pos, links, label=label, size=size, stats=stats, hist=hist),
                "hist1": lambda: eng.pair_hist_accumulate(pos, h1, counts)}
    if a.span:
        label2, size2, stats2 = torch.zeros_like(label), torch.zeros_like(size), torch.zeros_like(stats)
        hist2 = torch.zeros_like(hist)
        span = torch.zeros(n, dtype=torch.int32, device="cuda")
        image = torch.zeros((n, 3), dtype=torch.int32, device="cuda")
        rg2 = torch.zeros(n, dtype=torch.float64, device="cuda")
        pstats = torch.zeros(8, dtype=torch.int64, device="cuda")
        variants["span"] = lambda: eng.cluster_span(pos, links, label=label2, size=size2, stats=stats2, hist=hist2, span=span, image=image,
                                                    rg2=rg2, pstats=pstats)
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
    res = {"n": n, "phi": a.phi, "rlink": rlink, "rcut": rcut, "calls": a.calls,
           "ms_per_call": {name: [round(x, 4) for x in v] for name, v in ms.items()},
           "median_ms": {name: round(v, 4) for name, v in med.items()},
           "min_ms": {name: round(min(v), 4) for name, v in ms.items()}}
    if "clusters" in variants:
        res["stats"] = dict(zip(("clusters", "largest", "sum_s2", "N"), stats.cpu().tolist()))
        res["status"] = links.status()
        sz, lab = size.cpu().numpy(), label.cpu().numpy()
        res["labels_consistent"] = bool((lab[lab] == lab).all() and (np.bincount(lab, minlength=n)[lab] == sz).all())
    if "hist1" in variants:
        counts.zero_()
        variants["hist1"]()
        res["links"] = int(counts.sum())
    if "span" in variants:
        res["pstats"] = dict(zip(("spanning", "spanning_members", "span_a1", "span_a2", "span_a3", "span_all", "largest_finite", "sum_s2_finite"),
                                 pstats.cpu().tolist()))
        res["status"] = links.status()
        if "clusters" in variants:
            res["span_equals_label"] = bool(torch.equal(label, label2) and torch.equal(size, size2) and torch.equal(stats, stats2))
            res["span_over_clusters"] = round(med["span"] / med["clusters"], 3)
        r = rg2.cpu().numpy()
        res["rg2_max"] = float(r.max())
        res["spanning_rows_marked"] = bool(((r == -1.0) == (span.cpu().numpy() != 0)).all())
    if "clusters" in variants and "hist1" in variants:
        res["clusters_over_hist1"] = round(med["clusters"] / med["hist1"], 3)
    if a.host:
        res["host"] = host_baseline(p4[:, :3], L, rlink)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
