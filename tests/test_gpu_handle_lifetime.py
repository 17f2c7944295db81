"""What an engine handle and a team acquire they release: create, use, close, again and again, and the device's free memory stays where
it was.  Through the public Python API only.

Protocol of every configuration: one warm-up cycle (code objects, rocFFT kernels, allocator pools), synchronise, read the free device
memory; four more cycles; synchronise, read again.  The drop must stay below HALF of one engine's info()["device_bytes"] (a team: one
member's).  The factor is a condition, not a measurement: a handle leaked whole costs 4 x device_bytes over the four cycles, and
either of the two largest single items of these shapes -- the Lanczos basis V of 101 n_max rows of 32 bytes, the far-field grids --
alone costs more than half of device_bytes (the test prints device_bytes and the drop).  A forgotten array of a few kilobytes is below
what free memory resolves: that is ruled out by construction -- every acquisition of a handle goes through one of its owners
(pse_handle.h) -- not here."""
import gc
import os

import numpy as np
import pytest

from conftest import make_suspension, to4

pytestmark = pytest.mark.gpu

CYCLES = 4
SMALL = dict(n=2000, box=(24.0, 24.0, 24.0, 0.0), kw=dict(xi=0.5, error=1e-3, seed=3))   # single GPU
TEAM = dict(n=3000, phi=0.1, kw=dict(xi=0.5, error=1e-3, seed=77, grid=(48, 48, 40)))      # the smallest team of test_gpu_slabs.py
LOCAL = dict(n=24_000, phi=0.1, grid=64, world=2)                                          # the smallest of test_gpu_local.py


def _free():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _drop_over_cycles(cycle, cycles=CYCLES):
    """(drop of free memory over `cycles` cycles after one warm-up cycle, what the warm-up cycle returned)"""
    out = cycle()
    gc.collect()
    before = _free()
    for _ in range(cycles):
        cycle()
    gc.collect()
    return before - _free(), out


def _check(name, drop, device_bytes):
    print(f"{name}: device_bytes {device_bytes}, free memory dropped by {drop} bytes over {CYCLES} cycles (bound {device_bytes // 2})")
    assert device_bytes > 0 and drop < device_bytes / 2, (name, drop, device_bytes)


@pytest.mark.parametrize("skin", [None, "0"])
def test_single_engine_cycles_leave_free_memory_where_it_was(skin):
    """skin "0": PSE_SKIN=0 around the create -- a handle without the arrays of the kept neighbour list."""
    import pse_amd
    n, box = SMALL["n"], SMALL["box"]
    pos, force, _ = make_suspension(n, L=box[0])
    dpos, dF = to4(pos, 1.0), to4(force)
    vel = to4(np.zeros((n, 3)))

    def cycle():
        old = os.environ.get("PSE_SKIN")
        if skin is not None:
            os.environ["PSE_SKIN"] = skin
        try:      # (the developer switches are read in pse_create)
            eng = pse_amd.Engine(n, box, **SMALL["kw"])
        finally:
            if skin is not None:
                if old is None:
                    os.environ.pop("PSE_SKIN", None)
                else:
                    os.environ["PSE_SKIN"] = old
        assert (eng.neighbor_stats()[0] > 0.0) == (skin is None)
        eng.brownian_velocity(dpos, dF, 1.0, 1e-3, 7, vel=vel)       # the pair list and, with a skin, the kept list
        b0 = eng.info()["device_bytes"]
        eng.set_lanczos_operator("fp64")                             # the fp64 plane of the pair list, allocated now
        eng.brownian_velocity(dpos, dF, 1.0, 1e-3, 7, vel=vel)
        b1 = eng.info()["device_bytes"]
        assert b1 > b0
        eng.close()
        return b1

    drop, device_bytes = _drop_over_cycles(cycle)
    _check(f"single engine, PSE_SKIN={skin}", drop, device_bytes)


@pytest.mark.parametrize("world", [2, 3])
def test_loopback_team_cycles_leave_free_memory_where_they_were(world):
    """world 2: the far field replicated on both ranks (the second pair of Lanczos vectors, the mapped boundary buffer); world 3: the
    grid in slabs (send and receive buffers, the x plans)."""
    from pse_amd.sharded import LoopbackSimulation
    n = TEAM["n"]
    pos, force, box = make_suspension(n, phi=TEAM["phi"])

    def cycle():
        sim = LoopbackSimulation(n, box, world, **TEAM["kw"])
        sim.load(pos, force)
        sim.mobility()
        device_bytes = sim.engines[0].info()["device_bytes"]
        sim.team.close()
        for e in sim.engines:
            e.close()
        return device_bytes

    drop, device_bytes = _drop_over_cycles(cycle)
    _check(f"loopback team of {world}", drop, device_bytes)


def _local_kw(box):
    import math
    grid = LOCAL["grid"]
    xi = math.pi * grid / (2.0 * box[0] * math.sqrt(-math.log(1e-3)))       # (as test_gpu_local.py: xi from the fixed grid)
    return dict(xi=xi, error=1e-3, seed=5, grid=(grid,) * 3)


def _local_cycle(n, pos, force, box, world, kw):
    from pse_amd.sharded import LocalLoopbackSimulation
    sim = LocalLoopbackSimulation(n, box, world, **kw)
    sim.load(pos, force)
    sim.step(0.0, 1e-3, 0, integrate=False)
    sim.redistribute()                                                   # its buffers are allocated at the first call
    assert sim.team.local_status() == [0] * world
    device_bytes = sim.engines[0].info()["device_bytes"]
    sim.team.close()
    for e in sim.engines:
        e.close()
    return device_bytes


def test_local_team_cycles_and_refused_creates_leave_free_memory_where_it_was():
    """An owned-particle team of two: one step and one redistribution per cycle.  Then a create that is refused AFTER it has allocated
    (a row capacity too small for the rank's layers): four times the same refusal, and free memory within the same bound."""
    from pse_amd import PSEError
    from pse_amd.sharded import LocalLoopbackSimulation
    n, world = LOCAL["n"], LOCAL["world"]
    pos, force, box = make_suspension(n, phi=LOCAL["phi"])
    kw = _local_kw(box)
    drop, device_bytes = _drop_over_cycles(lambda: _local_cycle(n, pos, force, box, world, kw))
    _check(f"owned-particle team of {world}", drop, device_bytes)

    texts = []

    def refused():
        with pytest.raises(PSEError, match="too small a row capacity") as ei:
            LocalLoopbackSimulation(n, box, world, n_max=500, **kw)
        texts.append(str(ei.value))

    drop, _ = _drop_over_cycles(refused)
    assert len(set(texts)) == 1, texts
    _check("refused owned-particle create", drop, device_bytes)
