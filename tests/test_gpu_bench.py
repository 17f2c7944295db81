"""bench.py as every pull request runs it: a plain run times exactly --steps steps (in each of the two forms of the step) after
--warmup steps and nothing else, and --dump-outputs writes the state the last host-checked timed step left -- the same as a caller
of the step gets from the same steps -- and the state the queue-only steps after them left."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_steps_and_dumps_what_they_computed(tmp_path):
    n, grid, phi, warmup, steps = 20_000, 64, 0.1, 2, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PSE_FORCE_SHARDED")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--n", str(n), "--grid", str(grid), "--phi", str(phi), "--dump-outputs", str(tmp_path)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["n_gpus"] == 1 and set(d["step_modes"]) == {"host_checked", "queue_only"}
    assert d["ms_per_step"] == d["step_modes"][d["step_mode"]]["ms_per_step"] <= d["step_modes"]["host_checked"]["ms_per_step"]
    assert d["ms_per_step"] > 0 and abs(d["value"] - n / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["unit"] == "particle-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["roofline"] is None and "ms_per_step_percentiles" not in d and "reference_rule_grid" not in d and "config4_single_gpu" not in d
    names = ("positions", "velocities", "images", "lanczos_m")
    got = {name: np.load(tmp_path / (name + ".npy")) for name in names}
    queued = {name: np.load(tmp_path / ("queue_only_" + name + ".npy")) for name in names}
    assert all(a.dtype in (np.float32, np.float64) for a in list(got.values()) + list(queued.values()))
    assert not (tmp_path / "rows.npy").exists()      # (far below the budget: every particle)
    # the queue-only steps went on from the host-checked end state, ended at the count the line reports, and moved every particle
    assert queued["lanczos_m"].tolist() == [float(d["step_modes"]["queue_only"]["lanczos_m"])]
    assert all(queued[k].shape == got[k].shape for k in ("positions", "velocities", "images"))
    assert np.isfinite(queued["positions"]).all() and np.isfinite(queued["velocities"]).all()
    assert (np.abs(queued["positions"] - got["positions"]).max(axis=1) > 0).all()

    # the same W + K steps by a caller of the step, from the suspension bench.py builds
    import torch
    import pse_amd  # noqa: F401
    from pse_amd import distributed as pdist
    sys.path.insert(0, ROOT)
    import bench
    pos, force, L = bench.suspension(n, phi)
    xi = math.pi * grid / (2.0 * L * math.sqrt(-math.log(1e-3)))
    sim = pdist.make_simulation(n, (L, L, L, 0.0), xi=xi, error=1e-3, seed=1, grid=(grid,) * 3)
    sim.load(pos, force, mass=1.0)
    m = 2
    for it in range(warmup + steps):
        m = sim.step(1.0, 1e-3, it, lanczos_m=m)
    torch.cuda.synchronize()
    p = sim.pos[:, :3].cpu().numpy()
    assert got["lanczos_m"].tolist() == [float(m)]
    assert np.array_equal(got["images"], sim.image.cpu().numpy().astype(np.float32))
    # (the steps move a particle by ~0.03 each; two runs of them differ by summation order only)
    assert np.abs(got["positions"] - p).max() < 1e-6 and np.abs(got["positions"] - pos).max() > 1e-3
    v = sim.vel[:, :3].cpu().numpy()
    assert np.linalg.norm(got["velocities"] - v) / np.linalg.norm(v) < 1e-6
