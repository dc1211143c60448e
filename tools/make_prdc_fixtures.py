"""Fixture family f20: tests/golden/f20_prdc.npz, the PRDC cases of tests/test_prdc_cpu.py / tests/test_gpu_prdc.py.

    python tools/make_prdc_fixtures.py

Every case is (n1, n2, D, k) with rows from a seed (`gauss_rows` / `lattice_rows` of tests/test_prdc_cpu.py) and the
counts, radii and decision gap that `np_prdc` -- the definition in numpy fp64 with direct differences -- gives on them.  For a Gaussian
case the fake set's scale and shift are searched on a small grid, in a fixed order, for the first pair at which
  (a) no decision is closer than 1e-9: min |d2(R_i, G_j) - r_i^2|, |d2 - g_j^2| over ALL pairs, relative to |c_i|^2 + |c_j|^2, and
  (b) at least three of the four figures lie in (0.05, 0.95)
and what was used is stored.  Stored per case: `<name>.meta` = (n1, n2, D, k, seed),
`<name>.params` = (scale, shift), `.counts` int64 [4], `.radii_real`, `.radii_fake` fp64, `.gap`, `.digest` = the fp64 sums of the two
row sets, and the rows themselves (`.real`, `.fake`, float32) up to D = 64; the 2048-wide case stores seed and recipe only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

SHIFTS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0)
SCALES = (1.0, 0.98, 1.02, 0.95, 1.05, 0.9, 1.1, 0.8, 1.25)


def main():
    import test_prdc_cpu as T
    out = {'names': np.array(T.ALL_NAMES)}

    def store(name, meta, params, real, fake, res, gap):
        counts, fig, rr, rf, _ = res
        out[name + '.meta'] = np.array(meta, np.int64)
        out[name + '.params'] = np.array(params, np.float64)
        out[name + '.counts'] = counts
        out[name + '.radii_real'], out[name + '.radii_fake'] = rr, rf
        out[name + '.gap'] = np.float64(gap)
        out[name + '.digest'] = np.array([real.astype(np.float64).sum(), fake.astype(np.float64).sum()])
        if real.shape[1] <= T.STORED_ROWS_MAX_D:
            out[name + '.real'], out[name + '.fake'] = real, fake
        print('%-24s scale %.2f shift %.1f  counts %s  %s  gap %.3g' % (name, params[0], params[1], counts.tolist(),
                                                                    ' '.join('%s %.4f' % kv for kv in fig.items()), gap))

    for index, (n1, n2, D, k) in enumerate(T.GAUSS_CASES):
        seed, found = index + 1, None
        for shift in SHIFTS:
            for scale in SCALES:
                real, fake = T.gauss_rows(seed, n1, n2, D, scale, shift)
                res = T.np_prdc(real, fake, k)
                gap = T.decision_gap(real, fake, res[4])
                if sum(0.05 < v < 0.95 for v in res[1].values()) >= 3 and gap >= T.MIN_GAP:
                    found = (scale, shift, real, fake, res, gap)
                    break
            if found:
                break
        assert found, 'no (scale, shift) of the grid meets both conditions for %s' % ((n1, n2, D, k),)
        scale, shift, real, fake, res, gap = found
        store(T.case_name(n1, n2, D, k), (n1, n2, D, k, seed), (scale, shift), real, fake, res, gap)
    n1, n2, D, k = T.LATTICE_CASE
    seed = 20
    real, fake = T.lattice_rows(seed, n1, n2, D)
    res = T.np_prdc(real, fake, k)
    store(T.case_name(n1, n2, D, k, lattice=True), (n1, n2, D, k, seed), (1.0, 0.0), real, fake, res, 0.0)
    path = os.path.join(ROOT, 'tests', 'golden', 'f20_prdc.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
