#!/usr/bin/env python3
"""Time per tail-figure call (dlpm_amd.metrics.tail_device, both inputs on the device) against the numpy mirror's sort-based
computation (tests/tail_refs.mirror) on the host of the same machine, at xi = 0.95 and 100 levels, both marginals, for the shapes
[15000, 1, 2] (the 2-D config's eval.data_to_generate), [1000000, 1, 2] and [10000, 3, 32, 32] (--shapes picks by row count).  The
sets are heavy-tailed: Student-t with 1.5 degrees of freedom against a second draw scaled by 1.2.

Per (shape, marginal), one JSON line with
  * ms per call: one warm-up call, then REPEATS calls each between two device events (the call has no host synchronisation of its own);
    median, min and max;
  * the breakdown of ONE further call by the library's own event brackets (dlpm_prof_enable): tail_values, tail_select, tail_compact,
    tail_sort, tail_figures, and whether the sort takes more than the select and the compaction together;
  * the mirror's time on the host (one run; --no-host skips it), and the agreement: quantiles, k and thresholds equal bit for bit,
    msle and the Hill indices inside the bound of tail_refs.
Reported, not gated.  No speed is promised.

Usage: python tools/bench_tail.py [--shapes 15000 1000000 10000] [--repeats 5] [--no-host]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tail_refs as R  # noqa: E402

SHAPES = {15000: (15000, 1, 2), 1000000: (1000000, 1, 2), 10000: (10000, 3, 32, 32)}
SCOPES = ('tail_values', 'tail_select', 'tail_compact', 'tail_sort', 'tail_figures')
XI, LEVELS = 0.95, 100


def sets(shape, seed):
    g = np.random.default_rng(seed)
    return g.standard_t(1.5, shape).astype(np.float32), (1.2 * g.standard_t(1.5, shape)).astype(np.float32)


def breakdown(L, metrics, torch, x, y, marginal):
    L.dlpm_prof_enable(1)
    try:
        metrics.tail_device(x, y, XI, LEVELS, marginal)
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 16)
        assert L.dlpm_prof_report(buf, len(buf)) == 0
    finally:
        L.dlpm_prof_enable(0)
    ms = {k: 0.0 for k in SCOPES}
    for line in buf.value.decode().splitlines():
        name, _, t = line.split()[:3]
        if name in ms:
            ms[name] += float(t)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', type=int, nargs='+', default=list(SHAPES))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-host', action='store_true')
    a = ap.parse_args()
    import torch
    from dlpm_amd import _lib, metrics
    assert torch.cuda.is_available(), 'bench_tail.py needs the MI355X'
    L = _lib.lib()
    for rows in a.shapes:
        shape = SHAPES[rows]
        hx, hy = sets(shape, rows + 1)
        x, y = torch.from_numpy(hx).cuda(), torch.from_numpy(hy).cuda()
        for marginal in R.MARGINALS:
            out, q = metrics._tail_run(x, y, XI, LEVELS, marginal, True)               # the warm-up, and the values that are compared
            torch.cuda.synchronize()
            times = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                metrics.tail_device(x, y, XI, LEVELS, marginal)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            ms = breakdown(L, metrics, torch, x, y, marginal)
            o = out.cpu().numpy()
            res = {'shape': list(shape), 'marginal': marginal, 'xi': XI, 'levels': LEVELS, 'status': int(o[7]), 'msle': float(o[0]),
                   'hill': [float(o[1]), float(o[2])], 'k': [int(o[3]), int(o[5])], 'ms_median': round(statistics.median(times), 4),
                   'ms_min': round(min(times), 4), 'ms_max': round(max(times), 4), 'ms_scopes': {k: round(v, 4) for k, v in ms.items()},
                   'sort_dominates': ms['tail_sort'] > ms['tail_select'] + ms['tail_compact']}
            if not a.no_host:
                t0 = time.perf_counter()
                m = R.mirror(hx, hy, XI, LEVELS, marginal)
                res['host_mirror_ms'] = round((time.perf_counter() - t0) * 1e3, 2)
                res['bitwise'] = bool(q.cpu().numpy().tobytes() == m['quantiles'].tobytes() and [int(o[3]), int(o[5])] == m['k'] and
                                      [float(o[4]), float(o[6])] == [float(t) for t in m['threshold']])
                res['msle_error'], res['msle_bound'] = abs(float(o[0]) - m['msle']), R.msle_bound(m)
                res['hill_rel_error'] = [abs(float(o[1 + w]) - m['hill'][w]) / m['hill'][w] for w in (0, 1)]
                res['hill_rel_bound'] = [R.hill_rel_bound(m, w) for w in (0, 1)]
            print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
