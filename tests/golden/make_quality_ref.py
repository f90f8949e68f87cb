"""Writes tests/golden/quality_ref.json: for every case of tests/quality_cases.py the figures that the REFERENCE's own
sperr::calc_stats<T> and sperr::calc_mean_var<T> return (oracle/_ref/libSPERR_ref.so, called through ctypes on the
mangled instantiations), as hex bit patterns of T -- plus mse, which the reference does not return: the numpy model's
value, recorded only after the model's other seven figures matched the reference's bits (psnr within 8 ulp).

Run where oracle/_ref is built:  python tests/golden/make_quality_ref.py
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import quality_cases as qc   # noqa: E402

REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libSPERR_ref.so")


class RefStats:
    """calc_stats / calc_mean_var of the reference build; std::array<T, N> comes back as a struct of N values"""

    def __init__(self, path=REF_LIB):
        self.lib = C.CDLL(path)
        self.fn = {}
        for key, ct in (("f32", C.c_float), ("f64", C.c_double)):
            m = "f" if key == "f32" else "d"
            ret5 = type("Arr5" + m, (C.Structure,), {"_fields_": [("v", ct * 5)]})
            ret2 = type("Arr2" + m, (C.Structure,), {"_fields_": [("v", ct * 2)]})
            stats = getattr(self.lib, f"_ZN5sperr10calc_statsI{m}EESt5arrayIT_Lm5EEPKS2_S5_mm")
            stats.restype, stats.argtypes = ret5, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
            mv = getattr(self.lib, f"_ZN5sperr13calc_mean_varI{m}EESt5arrayIT_Lm2EEPKS2_mm")
            mv.restype, mv.argtypes = ret2, [C.c_void_p, C.c_size_t, C.c_size_t]
            self.fn[key] = (stats, mv)

    def __call__(self, a, b):
        """{rmse, linfty, psnr, min, max, mean, var} as values of a's dtype"""
        key = "f32" if a.dtype == np.float32 else "f64"
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        stats, mv = self.fn[key]
        s = stats(a.ctypes.data, b.ctypes.data, a.size, 1).v
        m = mv(a.ctypes.data, a.size, 1).v
        T = a.dtype.type
        return dict(zip(qc.FIGURES[:7], [T(x) for x in list(s) + list(m)]))


def record(ref, a, b):
    key = "f32" if a.dtype == np.float32 else "f64"
    got, mod = ref(a, b), qc.model(a, b)
    for f in qc.FIGURES[:7]:
        if f == "psnr":
            assert qc.ulp_distance(got[f], mod[f], a.dtype.type) <= 8, (f, got[f], mod[f])
        elif f in ("min", "max"):
            assert got[f] == mod[f], (f, got[f], mod[f])
        else:
            assert qc.to_hex(got[f]) == qc.to_hex(mod[f]), (f, got[f], mod[f])
    rec = {"dtype": key, "n": int(a.size)}
    rec.update({f: qc.to_hex(got[f]) for f in qc.FIGURES[:7]})
    rec["mse"] = qc.to_hex(mod["mse"])
    return rec


def main():
    from oracle.pyoracle import Oracle
    ref = RefStats()
    out = {}
    for name, make in qc.cases(Oracle()).items():
        a, b = make()
        out[name] = record(ref, a, b)
        print(name, {f: float(qc.from_hex(out[name][f], a.dtype.type)) for f in ("rmse", "psnr", "mse")})
    with open(qc.FIXTURE, "w") as f:
        json.dump({"generator": "tests/golden/make_quality_ref.py",
                   "reference": "sperr::calc_stats<T>, sperr::calc_mean_var<T> (src/sperr_helper.cpp)",
                   "cases": out}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
