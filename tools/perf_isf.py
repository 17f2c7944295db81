"""What a sample of the intermediate scattering functions costs, against the host path it replaces and against the structure-factor
pass on the same mode list: wall time per call, by stream events, of pse_isf_sample, of pse_isf_correlate (self part alone, collective
part alone, both) against `--pairs` stored origins and of pse_isf_store, for `--n` particles at seeded positions in a cubic box with
tilt 0.25 and one type, on `--modes` modes: "axis" = the 3 x (modes / 3) modes of analyze.axis_modes, "scattered" = seeded triples
within +-64.  `per_term_ns`: the time of the self part over n x modes x pairs terms, next to the same figure of
pse_structure_factor_accumulate (n x modes terms) on the same list.  The host path on the same inputs: the copy of the positions to
the host and, in NumPy, the fractional coordinates, their differences against `--pairs` origins kept on the host and the sums of
cos and sin of 2 pi m.ds over the particles, timed on `--host-n` particles (default: all of them) and scaled to n.
Each device figure is the time between one pair of events around `--calls` back-to-back calls after three warm-up calls, `--windows`
windows, the median reported.  The self part of the two paths must agree to 1e-9 n.  Prints one JSON line.

  python tools/perf_isf.py [--n 1000000] [--modes 96] [--kind axis] [--pairs 16] [--calls 10] [--windows 5] [--host-n N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--modes", type=int, default=96)
    ap.add_argument("--kind", choices=("axis", "scattered"), default="axis")
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--host-n", type=int, default=0)
    a = ap.parse_args()
    import torch
    import pse_amd
    from pse_amd import analyze
    n, npairs = a.n, a.pairs
    L = (4.0 * np.pi * n / (3.0 * 0.1)) ** (1.0 / 3.0)
    box = (L, L, L, 0.25)
    rng = np.random.default_rng(5)
    modes = analyze.axis_modes(a.modes // 3) if a.kind == "axis" else rng.integers(-64, 65, size=(a.modes, 3)).astype(np.int32)
    nk = len(modes)

    def frame():
        s = rng.uniform(-0.5, 0.5, size=(n, 3))
        p = np.zeros((n, 4))
        p[:, 1], p[:, 2] = s[:, 1] * L, s[:, 2] * L
        p[:, 0] = s[:, 0] * L + box[3] * p[:, 1]
        return p

    org, now = frame(), frame()
    now[:, :3] = org[:, :3] + 0.3 * rng.normal(size=(n, 3))                   # a displacement of a fraction of a radius
    eng = pse_amd.Engine(n, box)
    isf = eng.isf_origins(None, 1, modes, npairs)
    sf = eng.structure_factor(None, 1, modes)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")   # noqa: E731
    s_sums, c_sums, static, rho = z(npairs, 1, nk, 2), z(npairs, 1, 1, nk), z(1, nk), z(1, nk, 2)
    dorg, dnow = torch.tensor(org, device="cuda"), torch.tensor(now, device="cuda")
    slots = rows = list(range(npairs))
    eng.isf_sample(dorg, isf)
    for k in slots:
        eng.isf_store(isf, k)
    eng.isf_sample(dnow, isf)
    passes = dict(sample=lambda: eng.isf_sample(dnow, isf, static_sums=static),
                  self_part=lambda: eng.isf_correlate(isf, slots, rows, s_sums, None),
                  collective=lambda: eng.isf_correlate(isf, slots, rows, None, c_sums),
                  correlate=lambda: eng.isf_correlate(isf, slots, rows, s_sums, c_sums),
                  store=lambda: eng.isf_store(isf, 0),
                  structure_factor=lambda: eng.structure_factor_accumulate(dnow, sf, rho=rho, sums=static))

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

    eng.isf_correlate(isf, slots, rows, s_sums, None)     # (for the comparison below, before the timed store overwrites slot 0)
    got = s_sums.cpu().numpy()[:, 0]
    dev = {name: timed(f) for name, f in passes.items()}
    # the host path: the copy, s, and per origin the differences and the phasors (blocks of modes keep the table of phases small)
    hn = a.host_n or n
    inv = np.array([1.0 / L, 1.0 / L, 1.0 / L])

    def frac(p):
        return np.stack([(p[:, 0] - box[3] * p[:, 1]), p[:, 1], p[:, 2]], axis=1) * inv

    s_org = frac(org[:hn])
    mt = modes.astype(np.float64).T
    t0 = time.perf_counter()
    host_now = dnow.cpu().numpy()
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    s_now = frac(host_now[:hn])
    host_self = np.zeros((npairs, nk), dtype=np.complex128)
    for k in range(npairs):
        ds = s_now - s_org
        for q0 in range(0, nk, 32):
            t = 2.0 * np.pi * (ds @ mt[:, q0:q0 + 32])
            host_self[k, q0:q0 + 32] = np.cos(t).sum(axis=0) - 1j * np.sin(t).sum(axis=0)
    t_numpy = time.perf_counter() - t0
    if hn == n:
        err = np.abs((got[..., 0] + 1j * got[..., 1]) - host_self).max()
        assert err <= 1e-9 * n, err
    med = lambda v: round(float(np.median(v)), 5)   # noqa: E731
    ms = {name: med(v) for name, v in dev.items()}
    print(json.dumps(dict(n=n, kind=a.kind, nk=nk, pairs=npairs, device_ms=ms, device_ms_windows={k: [round(x, 5) for x in v] for k, v in dev.items()},
                          per_term_ns=dict(self_part=round(ms["self_part"] * 1e6 / (float(n) * nk * npairs), 6),
                                           structure_factor=round(ms["structure_factor"] * 1e6 / (float(n) * nk), 6)),
                          host_n=hn, host_copy_ms=round(t_copy * 1e3, 3), host_numpy_ms=round(t_numpy * 1e3 * n / hn, 1),
                          host_numpy_scaled=hn != n)))
    isf.close(); sf.close()
    eng.close()


if __name__ == "__main__":
    main()
