#!/usr/bin/env python3
"""What the reference's shear-function classes return AS BUILT (oracle/_ref/libpse_ref_shear.so, which `make -C oracle ref` compiles
where the reference tree is mounted) at the inputs of tests/golden/reference_arithmetic.json: shear rate and strain at every timestep
of every function, and its offset.  The fixture is data: those numbers.  tests/test_reference_build.py compares against it, and
checks it against the library wherever the library has been built.

  python3 tests/golden/make_built_shear_fixture.py      # rewrites tests/golden/reference_shear_built.json
"""
import ctypes
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "libpse_ref_shear.so")
OUT = os.path.join(HERE, "reference_shear_built.json")
FUNCTIONS = json.load(open(os.path.join(HERE, "reference_arithmetic.json")))["shear"]["functions"]
KIND = {"sine": 0, "sine_offset": 0, "steady": 1, "chirp": 2, "tukey": 3}


def library():
    """value(name, t, what) of the built library: what = 0 shear rate, 1 strain, 2 offset."""
    L = ctypes.CDLL(LIB)
    L.pse_ref_shear.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_uint, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    L.pse_ref_shear_windowed.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                         ctypes.c_uint, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]

    def args(a):
        return (ctypes.c_double * len(a))(*[float(x) for x in a])

    def value(name, t, what):
        f = FUNCTIONS
        out = ctypes.c_double()
        if name == "windowed_chirp_tukey":
            rc = L.pse_ref_shear_windowed(2, args(f["chirp"]["args"]), 3, args(f["tukey"]["args"]), t, what, ctypes.byref(out))
        else:
            rc = L.pse_ref_shear(KIND[name], args(f[name]["args"]), t, what, ctypes.byref(out))
        assert rc == 0
        return out.value
    return value


def values(value):
    return {name: {"shear_rate": [value(name, t, 0) for t in rows["timesteps"]], "strain": [value(name, t, 1) for t in rows["timesteps"]],
                   "offset": value(name, 0, 2)} for name, rows in FUNCTIONS.items()}


def main():
    with open(OUT, "w") as f:
        json.dump(values(library()), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
