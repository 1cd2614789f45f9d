"""Writes tests/golden/ease_plan.npz: the tables of tests/test_ease_plan.py run through record() of that module on
tests/golden/ease_plan_parent_harness.cpp -- the arithmetic of csrc/ease.hip and csrc/ease_pivot.hip as it stood before
csrc/ease_plan.h, copied line by line, with a handle of plain numbers, behind the extern "C" interface of tests/ease_plan_shim.cpp.
The harness does not include ease_plan.h: the fixture is independent of the header the test checks against it.

    python tests/golden/make_ease_plan_fixture.py [--source OTHER.cpp]
"""
import argparse
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import test_ease_plan as T      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", default=os.path.join(HERE, "ease_plan_parent_harness.cpp"))
    ap.add_argument("--out", default=T.GOLDEN)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        arrays = T.record(T.build_shim(d, a.source))
    np.savez_compressed(a.out, **arrays)
    print("written %s: %d arrays, %d bytes" % (a.out, len(arrays), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
