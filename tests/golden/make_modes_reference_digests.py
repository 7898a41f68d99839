#!/usr/bin/env python3
"""Digests of the two numpy statements of the mode fits (tests/modes_reference.py, tests/scene_modes_reference.py) for test_modes_cpu.py and
test_scene_modes_cpu.py: the sha256 of the raw bytes of every array that modes_f32 / modes_f64 and scene_modes_f32 / scene_modes_f64 return
(`margin` is kept as floats) on every entry of both SHAPES lists, at both units, under the planted scores and under equal weights, t_end = T_pred.

Run at the commit whose statements are the reference (the parent of a change that restates them); needs no GPU:

    python tests/golden/make_modes_reference_digests.py       # writes tests/golden/modes_reference_digests.json
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
PATH = os.path.join(HERE, "modes_reference_digests.json")


def digest(c):
    """{weighting/precision: {key: sha256 of (dtype, shape, bytes)}} of a case that holds c["scored"] and c["uniform"], each {"f32", "f64"}."""
    out = {}
    for tag in ("scored", "uniform"):
        for prec, res in c[tag].items():
            out[tag + "/" + prec] = r = {}
            for key, v in sorted(res.items()):
                a = np.ascontiguousarray(v)
                r[key] = a.astype(np.float64).tolist() if key == "margin" else hashlib.sha256(("%s %s " % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()
    return out


def name(call, shape, unit):
    return "%s/n%d_m%d_K%d_T%d_n%d/%s" % ((call,) + tuple(shape) + (("norm", "px")[unit],))


def main():
    from tests import scene_modes_reference as S
    from tests import test_modes_cpu as M
    from tests.modes_reference import SHAPES
    out = {}
    for unit in (0, 1):
        for s in SHAPES:
            out[name("modes", s, unit)] = digest(M.case(s, unit))
            print(name("modes", s, unit), flush=True)
        for s in S.SHAPES:
            out[name("scene_modes", s, unit)] = digest(S.case(s, unit))
            print(name("scene_modes", s, unit), flush=True)
    with open(PATH, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", PATH)


if __name__ == "__main__":
    main()
