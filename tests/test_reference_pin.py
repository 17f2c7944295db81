"""The oracle, the C++ host classes and (with -m gpu) the device table against tests/golden/reference_arithmetic.json: the
values the reference's OWN expression text takes (PSEv1/Stokes.cc:102,135-236,319,348-406, PSEv1/Helper.cu:326,
PSEv1/SpecificShearFunction.h, PSEv1/VariantShearFunction.h:47), generated in the build container by
tests/golden/make_reference_fixture.py, which reads that text from /root/reference at run time.  This is the pin of the
oracle to the reference: everything else in the test suite is pinned to the oracle."""
import json
import math
import os

import numpy as np
import pytest

FIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_arithmetic.json")))


def test_realspace_closed_forms_of_the_reference(oracle):
    """f = Imrr, g = rr of PSEv1/Stokes.cc:348-406 -- all three branches, incl. r = 2a exactly and deep overlap.  'exact' is
    the reference's expression in 50-digit arithmetic; for r < 0.25 the oracle switches to a quadrature of the defining
    Fourier integral, which this fixture checks independently of anything in the repo."""
    worst = 0.0
    for row in FIX["realspace"]["rows"]:
        f, g = oracle.fg_real(np.array([row["r"]]), row["xi"])
        worst = max(worst, abs(f[0] - row["Imrr_exact"]), abs(g[0] - row["rr_exact"]))
        assert abs(f[0] - row["Imrr_exact"]) < 2e-14 and abs(g[0] - row["rr_exact"]) < 2e-14, (row, f[0], g[0])
        # the reference's own double-precision evaluation of the same text: ill-conditioned at small r (it says so itself,
        # PSEv1/Stokes.cc:305-307), so only compared where its cancellation error is below 1e-12
        if row["r"] >= 0.5:
            assert abs(f[0] - row["Imrr_fp64"]) < 1e-12 and abs(g[0] - row["rr_fp64"]) < 1e-12, row
    assert worst < 2e-14


def test_self_mobility_of_the_reference(oracle):
    for row in FIX["realspace"]["self"]:
        assert abs(oracle.self_mobility(row["xi"]) - row["exact"]) < 2e-16 * 4
        assert abs(oracle.self_mobility(row["xi"]) - row["as_written"]) < 1e-11   # its sqrt(pi) has 12 digits (Stokes.cc:315)


def test_parameter_rule_of_the_reference(oracle):
    from pse_amd import engine
    for row in FIX["parameter_rule"]["rows"]:
        box = (row["L"],) * 3 + (0.0,)
        for p in (oracle.select_params(box, row["xi"], row["error"], row["max_strain"]),
                  None):
            if p is None:   # the product's rule (pse_host_select_params, host only)
                i = engine.host_select_params(box, xi=row["xi"], error=row["error"], max_strain=row["max_strain"])
                got = dict(rcut=i["rcut"], N=i["Nx"], lam=i["lam"], gaussm=i["gaussm"], P=i["P"], eta=i["eta"])
            else:
                got = dict(rcut=p["rcut"], N=p["grid"][0], lam=p["lambda"], gaussm=p["gaussm"], P=p["P"], eta=p["eta"])
            assert got["N"] == row["N"] and got["P"] == row["P"], (row, got)
            assert abs(got["rcut"] - row["rcut"]) < 1e-13 and abs(got["lam"] - row["lambda"]) < 1e-14
            assert abs(got["gaussm"] - row["gaussm"]) < 1e-12 and abs(got["eta"] - row["eta"]) < 1e-13 * row["eta"] + 1e-15, (row, got)


def test_seed_hash_of_the_reference(oracle):
    for row in FIX["seed_hash"]["rows"]:
        assert oracle.hash_seed(row["seed"]) == row["hashed"]


def test_wave_scale_of_the_reference(oracle):
    """gridk.w of PSEv1/Helper.cu:326 with exact pi against the oracle's w(k); as written (pi = 3.1415926536) it differs by
    the 3e-12 relative error of that constant -- the documented deliberate difference."""
    for row in FIX["wave_scale"]["rows"]:
        k2, xi, eta, ng = row["k2"], row["xi"], row["eta"], row["Ng"]
        q = k2 / (4 * xi * xi)
        w = 6.0 * math.pi * (1.0 + q) * math.exp(-(1.0 - eta) * q) / k2 / ng     # oracle/pse_port.py kvectors()
        assert abs(w - row["exact_pi"]) < 4e-16 * w
        assert abs(w - row["as_written"]) < 1e-11 * w
    # and the oracle's array version at one node: box 2 pi => k = integer index
    n = 8
    p = {"grid": (n, n, n), "xi": 0.5, "eta": 0.6}
    kx, ky, kz, k2, w, sinc = oracle.kvectors((2 * math.pi,) * 3 + (0.0,), p)
    assert abs(k2[1, 2, 3] - 14.0) < 1e-13
    q = 14.0 / (4 * 0.25)
    assert abs(w[1, 2, 3] - 6 * math.pi * (1 + q) * math.exp(-0.4 * q) / 14.0 / n ** 3) < 1e-18


def _objects(kind, make):
    f = FIX["shear"]["functions"]
    out = {}
    for name, cls in (("sine", "sin"), ("sine_offset", "sin"), ("steady", "steady"), ("chirp", "chirp"), ("tukey", "tukey")):
        out[name] = make(cls, f[name]["args"])
    out["windowed_chirp_tukey"] = make("windowed", (out["chirp"], out["tukey"]))
    return out


def _check_shear(objs, rate, strain):
    f = FIX["shear"]["functions"]
    for name, o in objs.items():
        ts = f[name]["timesteps"]
        for variant, tol in (("exact_constants", 2e-13), ("as_written", 2e-6)):
            # as written the reference uses pi = 3.1415926536 and a single-precision log (SpecificShearFunction.h:45,113-117):
            # the build uses exact pi and log, which moves the chirp phase by ~1e-7 relative
            for t, r_ref, s_ref in zip(ts, f[name][variant]["shear_rate"], f[name][variant]["strain"]):
                assert abs(rate(o, t) - r_ref) <= tol * max(1.0, abs(r_ref)), (name, variant, t, rate(o, t), r_ref)
                assert abs(strain(o, t) - s_ref) <= tol * max(1.0, abs(s_ref)), (name, variant, t, strain(o, t), s_ref)


def test_oracle_shear_functions_against_the_reference(oracle):
    def make(cls, a):
        return {"sin": oracle.SinShear, "steady": oracle.SteadyShear, "chirp": oracle.ChirpShear, "tukey": oracle.TukeyWindow,
                "windowed": oracle.Windowed}[cls](*a)
    _check_shear(_objects("oracle", make), lambda o, t: o.shear_rate(t), lambda o, t: o.strain(t))
    for row in FIX["shear"]["wrapValue"]:
        class S:
            offset = 0
            def strain(self, t): return row["value"]
        assert abs(oracle.variant_value(S(), 1, 10, row["min"], row["min"] + row["range"]) - row["wrapped"]) < 1e-15


def test_cpp_shear_functions_against_the_reference():
    from pse_amd import build
    build.build_all()
    from pse_amd import _PSEv1 as mod

    def make(cls, a):
        if cls == "windowed":
            return mod.WindowedFunction(*a)
        a = list(a)
        ctor = {"sin": mod.SinShearFunction, "steady": mod.SteadyShearFunction, "chirp": mod.ChirpShearFunction,
                "tukey": mod.TukeyWindowFunction}[cls]
        off = {"sin": 2, "steady": 1, "chirp": 4, "tukey": 2}[cls]
        a[off] = int(a[off])
        return ctor(*a)
    _check_shear(_objects("cpp", make), lambda o, t: o.getShearRate(t), lambda o, t: o.getStrain(t))
    for row in FIX["shear"]["wrapValue"]:
        class Const(mod.ShearFunction):
            def __init__(self):
                mod.ShearFunction.__init__(self)
            def getStrain(self, t):
                return row["value"]
        c = Const()   # kept alive: the C++ side calls back into it
        v = mod.VariantShearFunction(c, 10, row["min"], row["min"] + row["range"])
        assert abs(v.getValue(1) - row["wrapped"]) < 1e-15
    for row in FIX["seed_hash"]["rows"]:
        s = mod.Stokes(10, 20.0, 20.0, 20.0, 0.0, mod.VariantConst(1.0), row["seed"], 0.5, 1e-3, 1e-3)
        assert s.hashedSeed() == row["hashed"]


@pytest.mark.gpu
def test_device_realspace_table_against_the_reference():
    """pse_eval_realspace (the device's replacement of the m_ewaldC1 table) against the reference's closed forms."""
    import pse_amd
    by_xi = {}
    for row in FIX["realspace"]["rows"]:
        by_xi.setdefault(row["xi"], []).append(row)
    for xi, rows in by_xi.items():
        rcut = 10.0
        eng = pse_amd.Engine(64, (40.0, 40.0, 40.0, 0.0), xi=xi, error=1e-3, rcut=rcut)
        r = np.array([q["r"] for q in rows])
        f, g = eng.eval_realspace(r)
        # 2e-13: the table's contract for xi <= XI_TABLE = 4 (tests/test_realspace_table_cpu.py: the format allows it there, no further);
        # the fixture's xi are 0.27 .. 0.8
        assert np.abs(f - [q["Imrr_exact"] for q in rows]).max() < 2e-13
        assert np.abs(g - [q["rr_exact"] for q in rows]).max() < 2e-13
        eng.close()
