"""Writes tests/golden/likelihood_terms_truth.npz: the likelihood terms of tests/likelihood_terms_truth.py (the grids, the planted
models and the formulas are there) at 60 digits with mpmath, rounded to float64.

    python tests/golden/make_likelihood_terms_truth.py        # a few seconds; needs mpmath (1.3.0 wrote the committed file)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import likelihood_terms_truth as T      # noqa: E402


def main():
    out = {}
    for name, shape in T.shapes().items():
        a = np.empty(shape)
        for idx in np.ndindex(shape):
            a[idx] = T.entry(name, idx)
        out[name] = a
        fin = a[np.isfinite(a)]
        print(f"{name:10s} {str(shape):14s} {fin.size} finite of {a.size}, |value| from {np.abs(fin).min():.3g} to {np.abs(fin).max():.3g}")
    np.savez_compressed(T.FIXTURE, **out)
    print(f"wrote {T.FIXTURE}: {os.path.getsize(T.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
