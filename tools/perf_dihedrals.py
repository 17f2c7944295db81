#!/usr/bin/env python3
"""What the dihedral-force pass costs: time per call of pse_dihedral_forces with observables and without (out8 = NULL),
for the harmonic and the OPLS kind, against pse_angle_forces (harmonic) on the SAME chains in the same process -- `--n` beads in
helices of `--beads` (examples/helical_polymers.py build_topology; 20 beads: 17 dihedrals and 18 angles per chain).  Each figure is
the time between one pair of events around `--calls` back-to-back calls after three warm-up calls; `--windows` windows per variant,
taken alternately.  With it the ratio of each dihedral variant to the harmonic-angle pass, forces only (the bar: 4), and the bytes the
dihedral pass has to move at least -- per particle one row offset (4), its row entries (16 + 4 each), its position (32), its force
row read and written (64); the other members' positions are neighbours' rows that the caches serve.  Prints one JSON line.

  python tools/perf_dihedrals.py [--n 1000000] [--beads 20] [--calls 200] [--windows 4]"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--beads", type=int, default=20)
    ap.add_argument("--phi", type=float, default=0.1)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=4)
    a = ap.parse_args()
    import torch
    import pse_amd
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
    from helical_polymers import build_topology
    beads, nchains = a.beads, a.n // a.beads
    n = nchains * beads
    L = (4.0 * math.pi * n / (3.0 * a.phi)) ** (1.0 / 3.0)
    box = (L, L, L, 0.0)
    xyz, pairs, triples, quads = build_topology(nchains, beads, box, 2.0, seed=5)
    p4 = np.zeros((n, 4))
    p4[:, :3] = xyz
    pos = torch.tensor(p4, dtype=torch.float64, device="cuda")
    eng = pse_amd.Engine(n, box)
    al = eng.angles(triples, kinds="harmonic", k=20.0, theta0=1.9, n=n)
    lists = {"harmonic": eng.dihedrals(quads, kinds="harmonic", params=(10.0, -1.0, 1.0, 1.0), n=n),
             "harmonic3": eng.dihedrals(quads, kinds="harmonic", params=(10.0, 1.0, 3.0, 0.5), n=n),
             "opls": eng.dihedrals(quads, kinds="opls", params=(3.0, -1.0, 2.0, 0.5), n=n)}
    out = {name: torch.zeros(8, dtype=torch.float64, device="cuda") for name in ("angles",) + tuple(lists)}
    names = ["angles_forces_only", "angles_observables"] + [f"{k}_{v}" for k in lists for v in ("forces_only", "observables")]
    force = {name: torch.zeros((n, 4), dtype=torch.float64, device="cuda") for name in names}
    variants = {
        "angles_forces_only": lambda: al.forces(pos, force["angles_forces_only"], accumulate=False, observables=False),
        "angles_observables": lambda: al.forces(pos, force["angles_observables"], accumulate=False, out=out["angles"]),
    }
    for kind, dl in lists.items():
        variants[f"{kind}_forces_only"] = lambda dl=dl, kind=kind: dl.forces(pos, force[f"{kind}_forces_only"], accumulate=False, observables=False)
        variants[f"{kind}_observables"] = lambda dl=dl, kind=kind: dl.forces(pos, force[f"{kind}_observables"], accumulate=False, out=out[kind])
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
    nbytes = 4 * (n + 1) + 20 * 4 * len(quads) + 32 * n + 64 * n
    o = {name: t.cpu().numpy() for name, t in out.items()}
    res = {
        "n": n, "beads": beads, "nangles": int(len(triples)), "ndihedrals": int(len(quads)), "calls": a.calls,
        "ms_per_call": {name: [round(x, 4) for x in v] for name, v in ms.items()},
        "median_ms": {name: round(v, 4) for name, v in med.items()},
        "ratio_to_angles_forces_only": {name: round(med[name] / med["angles_forces_only"], 2) for name in med if name.endswith("forces_only")},
        "ratio_to_angles_observables": {name: round(med[name] / med["angles_observables"], 2) for name in med if name.endswith("observables")},
        "dihedral_model_bytes": nbytes, "dihedral_model_bytes_per_particle": round(nbytes / n, 1),
        "fraction_of_hbm_peak": {name: round(nbytes / (v * 1e-3) / HBM_PEAK, 3) for name, v in med.items() if not name.startswith("angles")},
        "ndihedrals_acted": {k: float(o[k][7]) for k in lists}, "U": {k: float(o[k][0]) for k in lists},
        "trace_W": {k: float(o[k][1] + o[k][4] + o[k][6]) for k in lists},
        "max_force_difference": {k: float((force[f"{k}_observables"] - force[f"{k}_forces_only"]).abs().max()) for k in lists},
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
