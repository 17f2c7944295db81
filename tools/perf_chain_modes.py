"""What a sample of the chain normal modes costs, against the host path it replaces and against the bytes it must move: wall time per
sample, by stream events, of pse_chain_modes_compute + pse_chain_modes_correlate + pse_chain_modes_store as analyze.RouseModes issues
them (nmodes = `--modes` Rouse modes and the end-to-end row, static sums, `--origins` live origins) for `--chains` linear chains of
`--beads` beads with bonds of length 2 in a cubic box at volume fraction phi; each of the three passes alone; and the wall time of the
host path on the same positions: one pse_molecules_compute for the unfolded positions (what Conformations.unfolded() runs), their
device-to-host copy, and the NumPy projection onto the same weights and correlation with the same number of origins.
`bytes`: what each pass must move at the least -- compute: the positions (32 B a bead), the three index words of a member slot
(12 B) and the current buffer (24 K B a chain); correlate: the current buffer and every listed origin once; store: the buffer read and
written -- and `floor_ms`, that at 5.5 TB/s.  Each device figure is the time between one pair of events around `--calls` back-to-back
samples after three warm-up samples, `--windows` windows, the median reported; the host path is timed `--host-windows` times.  The
modes and the correlation of the two paths must agree to 1e-11 of their largest entry.  Prints one JSON line.

  python tools/perf_chain_modes.py [--chains 200] [--beads 20] [--modes 8] [--origins 16] [--phi 0.1] [--calls 20] [--windows 5]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM = 5.5e12   # bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=200)
    ap.add_argument("--beads", type=int, default=20)
    ap.add_argument("--modes", type=int, default=8)
    ap.add_argument("--origins", type=int, default=16)
    ap.add_argument("--phi", type=float, default=0.1)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--host-windows", type=int, default=3)
    a = ap.parse_args()
    import torch
    import pse_amd
    nchains, beads, K, norg = a.chains, a.beads, a.modes + 1, a.origins
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
    w = pse_amd.host_rouse_weights(beads, K)
    cm = eng.chain_modes(pairs, [beads], [w], norigins=norg)
    mol = eng.molecule_topology(pairs)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")   # noqa: E731
    sums, corr, modes, unfolded = z(1, K, 6), z(norg, 1, K, 3, 3), z(nchains, K, 3), z(n, 4)
    slots, rows = list(range(norg)), list(range(norg))
    eng.chain_modes_compute(pos, cm, sums=sums)
    for s in slots:
        eng.chain_modes_store(cm, s)
    passes = dict(compute=lambda: eng.chain_modes_compute(pos, cm, sums=sums), correlate=lambda: eng.chain_modes_correlate(cm, slots, rows, corr),
                  store=lambda: eng.chain_modes_store(cm, 0))

    def sample():
        for f in passes.values():
            f()

    def timed(f):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / a.calls)
        return ms

    dev = dict(sample=timed(sample), **{name: timed(f) for name, f in passes.items()})
    origins = None

    def host():
        eng.molecules_compute(pos, mol, unfolded=unfolded)
        uu = unfolded.cpu().numpy()[:, :3].reshape(nchains, beads, 3)
        X = np.einsum("kq,jqc->jkc", w, uu - uu[:, :1])
        org = origins if origins is not None else np.broadcast_to(X, (norg,) + X.shape)
        return X, np.einsum("jka,ojkb->okab", X, org), np.einsum("jka,jkb->kab", X, X)

    host_ms = []
    for _ in range(a.host_windows):
        t0 = time.perf_counter()
        X, C, _ = host()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    corr.zero_()
    eng.chain_modes_compute(pos, cm, out=modes)
    eng.chain_modes_correlate(cm, slots, rows, corr)       # (every slot holds the modes of these positions)
    got_x, got_c = modes.cpu().numpy(), corr.cpu().numpy()[:, 0]
    assert np.abs(got_x - X).max() <= 1e-11 * np.abs(X).max(), np.abs(got_x - X).max()
    assert np.abs(got_c - C).max() <= 1e-11 * np.abs(C).max(), np.abs(got_c - C).max()
    buf = 24.0 * K * nchains
    nbytes = dict(compute=44.0 * n + buf, correlate=(1 + norg) * buf, store=2 * buf)
    nbytes["sample"] = sum(nbytes.values())
    med = lambda v: round(float(np.median(v)), 5)   # noqa: E731
    print(json.dumps(dict(chains=nchains, beads=beads, n=n, K=K, origins=norg, tiles=-(-nchains // (1024 // beads)),
                          device_ms={name: med(v) for name, v in dev.items()}, device_ms_windows=[round(v, 5) for v in dev["sample"]],
                          bytes={name: int(v) for name, v in nbytes.items()},
                          floor_ms={name: round(v / HBM * 1e3, 5) for name, v in nbytes.items()},
                          host_ms=round(float(np.median(host_ms)), 3), host_ms_windows=[round(v, 3) for v in host_ms])))
    cm.close(); mol.close()
    eng.close()


if __name__ == "__main__":
    main()
