"""Records tests/golden/reference_ot.npz: the exact optimal-transport cost of the pure expression problem of anchor (a)
(tests/test_ot.py), from scipy's ``linear_sum_assignment`` - with uniform marginals and n = m the transport polytope's
vertices are the permutation matrices over n, so the optimum is the assignment optimum over n.  The file holds seeds and
scalars only; the cost matrices are rebuilt from the seeds by tests/ot_util.py.  Needs scipy; the tests do not.

usage: python tests/golden/make_ot_golden.py"""
import os
import sys

import numpy as np
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ot_util as U  # noqa: E402

SEEDS, N, P = (0, 1, 2), 60, 8

if __name__ == "__main__":
    exact, m_inf = [], []
    for seed in SEEDS:
        _, YA, _, YB = U.assignment_case(seed, N, P)
        M = U.expr_cost(YA, YB, "kl")
        r, c = linear_sum_assignment(M)
        exact.append(M[r, c].sum() / N)
        m_inf.append(np.abs(M).max())
        print(f"seed {seed}: exact transport cost {exact[-1]:.12f}, |M|_inf {m_inf[-1]:.6f}")
    np.savez(os.path.join(HERE, "reference_ot.npz"), seeds=np.array(SEEDS), n=np.array(N), P=np.array(P),
             exact=np.array(exact), m_inf=np.array(m_inf))
