#!/usr/bin/env python3
"""What desire_amd.evaluate's walk prints, and what it calls the model with, on the stub model and videos of tests/evaluate_walk_cases.py, for
tests/test_evaluate_walk_cpu.py.  Needs no GPU.

Run at the commit whose evaluate() is the reference (the parent of the change under test):

    python tests/golden/make_evaluate_walk_golden.py        # writes tests/golden/evaluate_walk.json

Per command line: "text" = json.dumps(result, indent=1), byte for byte what main() prints, and "calls" = the sorted log of the model calls.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import evaluate_walk_cases as WC  # noqa: E402


def main():
    out = {}
    for tag, extra in WC.CASES.items():
        text, calls = WC.walk(extra)
        out[tag] = {"text": text, "calls": calls}
        res = json.loads(text)
        print("%-16s windows %d  agents %s  calls %d" % (tag, res["windows"], res["agents"], len(calls)))
    path = os.path.join(HERE, "evaluate_walk.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
