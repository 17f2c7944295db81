"""What a sample of the chain conformations costs, against the host path it replaces: wall time per call, by stream events, of
pse_molecules_compute as analyze.Conformations issues it (sums and sample; `--rows`: the per-molecule rows as well) for `--chains`
linear chains of `--beads` beads with bonds of length 2 in a cubic box at volume fraction phi, and the wall time of the examples'
private function on the same positions: the device-to-host copy of the positions plus the NumPy unfolding and reduction.
The pass must move 32 bytes gathered per bead, the member and parent words (8 bytes per bead), 4 bytes per molecule of its root and
4 of its ends and type, and its outputs (one row of 14 doubles per tile and type, the sums; with --rows 112 bytes per molecule):
`model_bytes`, and `stream_ms`, the time those bytes take at the 5.5 TB/s that a plain streaming pass reaches on this device
(DESIGN.md).  Each figure is the time between one pair of events around `--calls` back-to-back calls after three warm-up calls,
`--windows` windows, the median reported.  The mean Rg of the two paths must agree to 1e-12 relative.  Prints one JSON line.

  python tools/perf_conformations.py [--chains 200] [--beads 20] [--phi 0.1] [--calls 20] [--windows 5] [--rows]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def radius_of_gyration(pos, box, nchains, beads):
    """The function of examples/polymer_solution.py."""
    Lx, Ly, Lz, xy = box
    p = pos.reshape(nchains, beads, 3)
    d = p[:, 1:] - p[:, :-1]
    n = np.rint(d[..., 2] / Lz); d[..., 2] -= n * Lz
    n = np.rint(d[..., 1] / Ly); d[..., 1] -= n * Ly; d[..., 0] -= n * xy * Ly
    n = np.rint(d[..., 0] / Lx); d[..., 0] -= n * Lx
    chain = np.concatenate([np.zeros((nchains, 1, 3)), np.cumsum(d, axis=1)], axis=1)
    chain -= chain.mean(axis=1, keepdims=True)
    return float(np.sqrt((chain ** 2).sum(axis=2).mean(axis=1)).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=200)
    ap.add_argument("--beads", type=int, default=20)
    ap.add_argument("--phi", type=float, default=0.1)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rows", action="store_true", help="write the per-molecule rows as well")
    a = ap.parse_args()
    import torch
    import pse_amd
    nchains, beads = a.chains, a.beads
    n = nchains * beads
    L = (4.0 * math.pi * n / (3.0 * a.phi)) ** (1.0 / 3.0)
    box = (L, L, L, 0.25)
    rng = np.random.default_rng(5)
    u = rng.normal(size=(nchains, beads - 1, 3))
    u *= 2.0 / np.linalg.norm(u, axis=2)[:, :, None]
    start = (rng.uniform(size=(nchains, 1, 3)) - 0.5) * L
    p = np.concatenate([start, start + np.cumsum(u, axis=1)], axis=1).reshape(-1, 3)
    k = np.floor(p[:, 2] / L + 0.5); p[:, 2] -= k * L
    k = np.floor(p[:, 1] / L + 0.5); p[:, 1] -= k * L; p[:, 0] -= k * box[3] * L
    k = np.floor((p[:, 0] - box[3] * p[:, 1]) / L + 0.5); p[:, 0] -= k * L
    first = (np.arange(nchains)[:, None] * beads + np.arange(beads - 1)[None, :]).reshape(-1)
    pairs = np.stack([first, first + 1], axis=1)
    p4 = np.zeros((n, 4)); p4[:, :3] = p
    pos = torch.tensor(p4, dtype=torch.float64, device="cuda")
    eng = pse_amd.Engine(n, box)
    mol = eng.molecule_topology(pairs)
    sums = torch.zeros((1, 14), dtype=torch.float64, device="cuda")
    sample = torch.zeros((1, 14), dtype=torch.float64, device="cuda")
    rows = torch.zeros((mol.nmol, 14), dtype=torch.float64, device="cuda")

    def device():
        eng.molecules_compute(pos, mol, rows=rows if a.rows else None, sums=sums, sample=sample)

    def host():
        return radius_of_gyration(pos[:, :3].cpu().numpy(), box, nchains, beads)

    for _ in range(3):
        device()
    torch.cuda.synchronize()
    dev_ms = []
    for _ in range(a.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            device()
        e1.record()
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1) / a.calls)
    host_ms = []
    for _ in range(a.windows):
        t0 = time.perf_counter()
        rg_host = host()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    eng.molecules_compute(pos, mol, rows=rows)
    rg_dev = float(torch.sqrt(rows[:, 9]).mean())
    assert abs(rg_dev - rg_host) <= 1e-12 * rg_host, (rg_dev, rg_host)
    ntiles = -(-nchains // (1024 // beads))
    model = n * (32 + 8) + mol.nmol * 8 + ntiles * 14 * 8 * 2 + 14 * 8 * 3 + (mol.nmol * 112 if a.rows else 0)
    print(json.dumps(dict(chains=nchains, beads=beads, n=n, tiles=ntiles, rows=bool(a.rows), device_ms=round(float(np.median(dev_ms)), 5),
                          device_ms_windows=[round(v, 5) for v in dev_ms], host_ms=round(float(np.median(host_ms)), 4),
                          model_bytes=model, stream_ms=round(model / 5.5e12 * 1e3, 6),
                          ratio_to_stream=round(float(np.median(dev_ms)) / (model / 5.5e12 * 1e3), 2), rg_device=rg_dev, rg_host=rg_host)))
    mol.close()
    eng.close()


if __name__ == "__main__":
    main()
