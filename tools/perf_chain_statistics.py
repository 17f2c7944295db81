"""What a sample of the chain statistics costs, against the host path it replaces: wall time per call, by stream events, of
pse_molecule_pairs_compute as analyze.ChainStatistics issues it (curves, sums and sample, ns = the chain length) for `--chains` linear
chains of `--beads` beads with bonds of length 2 in a cubic box at volume fraction phi, and the wall time of the host path on the same
positions: one pse_molecules_compute for the unfolded positions (what Conformations.unfolded() runs), their device-to-host copy, and
NumPy pair sums over the separations -- 1/Rh, D(s) and C(s) of every chain.  `pairs` is the number of pair terms of one call.
Each device figure is the time between one pair of events around `--calls` back-to-back calls after three warm-up calls, `--windows`
windows, the median reported; the host path is timed `--host-windows` times.  The mean 1/Rh and the curves of the two paths must
agree to 1e-11 relative.  Prints one JSON line.

  python tools/perf_chain_statistics.py [--chains 200] [--beads 20] [--phi 0.1] [--calls 20] [--windows 5] [--host-windows 3]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def host_pair_sums(unfolded, nchains, beads):
    """(1/Rh per chain, D (beads,), C (beads,)) from the unfolded positions, one NumPy pass per separation."""
    u = unfolded[:, :3].reshape(nchains, beads, 3)
    b = u[:, 1:] - u[:, :-1]
    h, D, C = np.zeros(nchains), np.zeros(beads), np.zeros(beads)
    C[0] = (b * b).sum()
    for s in range(1, beads):
        r2 = ((u[:, s:] - u[:, :-s]) ** 2).sum(axis=2)
        h += (1.0 / np.sqrt(r2)).sum(axis=1)
        D[s] = r2.sum()
        if s < beads - 1:
            C[s] = (b[:, s:] * b[:, :-s]).sum()
    return 2.0 * h / beads ** 2, D, C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=200)
    ap.add_argument("--beads", type=int, default=20)
    ap.add_argument("--phi", type=float, default=0.1)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--host-windows", type=int, default=3)
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
    mp = eng.molecule_pairs(pairs, ns=beads)
    mol = eng.molecule_topology(pairs)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")   # noqa: E731
    curves, sums, sample, inv = z(1, beads, 2), z(1, 2), z(1, 2), z(mp.nmol)
    unfolded = z(n, 4)

    def device():
        eng.molecule_pairs_compute(pos, mp, curves=curves, sums=sums, sample=sample)

    def host():
        eng.molecules_compute(pos, mol, unfolded=unfolded)
        return host_pair_sums(unfolded.cpu().numpy(), nchains, beads)

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
    for _ in range(a.host_windows):
        t0 = time.perf_counter()
        h, D, C = host()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    curves.zero_()
    eng.molecule_pairs_compute(pos, mp, inv_rh=inv, curves=curves)
    got = curves.cpu().numpy()[0]
    inv_dev = float(inv.mean())
    assert abs(inv_dev - h.mean()) <= 1e-11 * h.mean(), (inv_dev, h.mean())
    assert np.all(np.abs(got[:, 0] - D) <= 1e-11 * D.max()) and np.all(np.abs(got[:, 1] - C) <= 1e-11 * np.abs(C).max())
    print(json.dumps(dict(chains=nchains, beads=beads, n=n, tiles=-(-nchains // (1024 // beads)), pairs=nchains * beads * (beads - 1) // 2,
                          device_ms=round(float(np.median(dev_ms)), 5), device_ms_windows=[round(v, 5) for v in dev_ms],
                          host_ms=round(float(np.median(host_ms)), 3), host_ms_windows=[round(v, 3) for v in host_ms],
                          inv_rh_device=inv_dev, inv_rh_host=float(h.mean()))))
    mp.close(); mol.close()
    eng.close()


if __name__ == "__main__":
    main()
