#!/usr/bin/env python
"""Write tests/golden/f26_w1.npz, the fixture family of the exact W1 (tests/w1_refs.py holds the case table, the recipes of the
inputs, the cost and the mirror).  Per table case and ground:
    <case>.x, <case>.y              the float32 inputs (shared by both grounds)
    <case>.<ground>.w_opt           (1 / n) * the optimal assignment cost of the fp64 cost matrix, by scipy.optimize.linear_sum_assignment,
                                    its n terms added exactly (math.fsum)
    <case>.<ground>.q_opt           the optimum of the INTEGER matrix q by linear_sum_assignment (int64)
    <case>.<ground>.w_brute, .q_brute   the same two optima by brute force over all n! permutations, n <= 7
What the fixture is: the reference's COST DEFINITION (compute_mean_lploss with lploss = 1 between single points, and the Euclidean
norm) solved exactly as an assignment problem.  The reference's own branch, compute_wasserstein_distance(..., manual_compute=True)
of bem/evaluate/wasserstein.py:23-46, cannot be run here: it needs `pyemd`, which is not installed; by DESIGN 3.22 its 2N-bin
transport optimum equals the assignment optimum / N.
The tool also checks that no table case needs more than w1_refs.MAX_TABLE_ROUNDS rounds of the mirror, and prints the counts.

Usage: python tools/make_w1_fixtures.py [--out tests/golden/f26_w1.npz]"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import w1_refs as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=R.FIXTURE)
    a = ap.parse_args()
    out, worst = {}, 0
    for name, (n, D, seed) in R.CASES.items():
        x, y = R.case_inputs(name)
        out[name + '.x'], out[name + '.y'] = x, y
        for g in R.GROUNDS:
            c = R.costs(x, y, g)
            q, e, cmax = R.quantise(c)
            terms, _ = R.scipy_optimum(c)
            out['%s.%s.w_opt' % (name, g)] = np.float64(math.fsum(terms.tolist()) / n)
            out['%s.%s.q_opt' % (name, g)] = np.int64(R.scipy_optimum(q)[0].sum())
            if n <= 7:
                out['%s.%s.w_brute' % (name, g)] = np.float64(R.brute_optimum(c) / n)
                out['%s.%s.q_brute' % (name, g)] = np.int64(R.brute_optimum(q))
            if (name, g) in R.PAIRS:
                m = R.mirror(name, g)
                worst = max(worst, m['rounds'])
                assert m['rounds'] <= R.MAX_TABLE_ROUNDS, '%s %s: %d rounds -- pick another seed' % (name, g, m['rounds'])
                print('%-12s %-10s e %3d rounds %6d phases %2d w %.17g w_opt %.17g' % (name, g, e, m['rounds'], m['phases'], m['w'],
                                                                                      out['%s.%s.w_opt' % (name, g)]))
    np.savez(a.out, **out)
    print('wrote %s: %d arrays, %d bytes; most rounds %d' % (a.out, len(out), os.path.getsize(a.out), worst))


if __name__ == '__main__':
    main()
