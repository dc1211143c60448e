#!/usr/bin/env python3
"""Time per exact-W1 call (dlpm_amd.metrics.w1_device, both inputs on the device) against scipy.optimize.linear_sum_assignment on
the host on the SAME fp64 costs (tests/w1_refs.costs), for N in {256, 1024, 4096} (--sizes) at D = 2, both grounds, and two kinds of
sets: `gauss` (N(0, 1) against 1.2 N(0, 1) + 0.3) and `cauchy` (a Cauchy set clipped to [-50, 50] against N(0, 1)).  Per
configuration and tail_threshold in {0, 4, 16, 64}: one warm-up call, then REPEATS timed calls (host clock around the call and a
device synchronise; the call itself waits on the stream once per batch of rounds), the thresholds visited in alternation.  Recorded:
the median / min / max time, rounds, phases, the rounds run by the one-workgroup kernel, W, and -- where scipy ran (N <=
--scipy-max-n) -- scipy's time, its optimum and W - optimum against the bound 2^-e + n 2^-52 cmax.  Results are the same bits under
every threshold; the tool asserts it.  One JSON line per (configuration, threshold); reported, not gated.  No speed is promised.

--host-only runs the scipy side alone (no GPU needed) and prints its times and optima.

Usage: python tools/bench_w1.py [--sizes 256 1024 4096] [--repeats 3] [--thresholds 0 4 16 64] [--scipy-max-n 1024] [--host-only]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import w1_refs as R  # noqa: E402

THRESHOLDS = (0, 4, 16, 64)


def sets(kind, n, seed):
    g = np.random.default_rng(seed)
    if kind == 'gauss':
        return g.standard_normal((n, 2)).astype(np.float32), (1.2 * g.standard_normal((n, 2)) + 0.3).astype(np.float32)
    return np.clip(g.standard_cauchy((n, 2)), -50.0, 50.0).astype(np.float32), g.standard_normal((n, 2)).astype(np.float32)


def host_side(x, y, ground):
    c = R.costs(x, y, ground)
    t0 = time.perf_counter()
    terms, _ = R.scipy_optimum(c)
    dt = time.perf_counter() - t0
    return dt, math.fsum(terms.tolist()) / len(x)


def main():
    global THRESHOLDS
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 1024, 4096])
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--scipy-max-n', type=int, default=1024)
    ap.add_argument('--host-only', action='store_true')
    ap.add_argument('--thresholds', type=int, nargs='+', default=list(THRESHOLDS))
    a = ap.parse_args()
    THRESHOLDS = tuple(a.thresholds)
    configs = [(kind, n, g) for n in a.sizes for kind in ('gauss', 'cauchy') for g in R.GROUNDS]
    R.scipy_optimum(np.zeros((2, 2)))                        # scipy's import and first call are not part of any timing
    if a.host_only:
        for kind, n, ground in configs:
            x, y = sets(kind, n, 7 * n + 1)
            dt, opt = host_side(x, y, ground)
            print(json.dumps({'config': '%s_%d_%s' % (kind, n, ground), 'scipy_s': round(dt, 4), 'scipy_optimum': opt}), flush=True)
        return
    import torch
    from dlpm_amd import metrics
    assert torch.cuda.is_available(), 'bench_w1.py needs the MI355X'
    for kind, n, ground in configs:
        hx, hy = sets(kind, n, 7 * n + 1)
        x, y = torch.from_numpy(hx).cuda(), torch.from_numpy(hy).cuda()
        times, outs = {t: [] for t in THRESHOLDS}, {}
        for t in THRESHOLDS:                                 # warm-up of every variant
            outs[t] = metrics.w1_device(x, y, ground, tail_threshold=t)
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for t in THRESHOLDS:
                t0 = time.perf_counter()
                outs[t] = metrics.w1_device(x, y, ground, tail_threshold=t)
                torch.cuda.synchronize()
                times[t].append((time.perf_counter() - t0) * 1e3)
        first = [v.cpu().numpy() for v in outs[THRESHOLDS[0]]]
        host = host_side(hx, hy, ground) if n <= a.scipy_max_n else None
        for t in THRESHOLDS:
            o, perm, prices = (v.cpu().numpy() for v in outs[t])
            assert o[:7].tobytes() == first[0][:7].tobytes() and (perm == first[1]).all() and (prices == first[2]).all(), (kind, n, ground, t)
            res = {'config': '%s_%d_%s' % (kind, n, ground), 'tail_threshold': t, 'status': int(o[6]), 'w1': float(o[0]),
                   'ms_median': round(statistics.median(times[t]), 3), 'ms_min': round(min(times[t]), 3), 'ms_max': round(max(times[t]), 3),
                   'rounds': int(o[3]), 'phases': int(o[4]), 'tail_rounds': int(o[7]), 'scale_exponent': int(o[2]), 'cmax': float(o[5])}
            if host is not None:
                res.update(scipy_s=round(host[0], 4), scipy_optimum=host[1], excess=float(o[0]) - host[1],
                           bound=R.w_bound(int(o[2]), n, float(o[5])))
            print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
