"""Writes tests/golden/partial_sums.npz: the bits of every bias, gamma, beta and mask-token gradient at the cases of
tests/partial_sums_cases.py, as the built library computes them.  Run it BEFORE a change to those kernels that must keep their
bits.  Needs a GPU.   usage: python tests/golden/make_partial_sums.py [output.npz]"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import partial_sums_cases as cases  # noqa: E402
from ssl4polyp_amd.engine import Kernels  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "partial_sums.npz")
    frozen = cases.freeze(cases.outputs(functools.lru_cache(maxsize=None)(Kernels)))
    np.savez(path, **frozen)
    print(len(frozen), "arrays ->", path)


if __name__ == "__main__":
    main()
