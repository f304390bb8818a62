"""Writes tests/golden/meth_dae_truth.npz: the methanation DAE's solution at t = 0.5, 5 and 75 for 12 (experiment, parameter) runs by
backward Euler on nested graded grids with Richardson extrapolation (tests/meth_dae_truth.py) - on the CPU, from the pinned
residual oracle.methanation.reaction alone.

    python tests/golden/make_meth_dae_truth.py
"""
import os
import sys

os.environ.setdefault("OMP_NUM_THREADS", "1")          # 12 independent runs in a process pool: one thread each
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np

import meth_dae_truth as T


def main():
    d = T.generate()
    worst = d["bar"].max()
    print("error bars (units), run x time:\n", d["bar"])
    if worst > T.BAR_MAX:
        raise SystemExit(f"error bar {worst} units > {T.BAR_MAX}: refine the grid or add a level")
    np.savez_compressed(T.FIXTURE, **d)
    print(f"wrote {T.FIXTURE}: {os.path.getsize(T.FIXTURE)} bytes, worst error bar {worst:.3g} units")


if __name__ == "__main__":
    main()
