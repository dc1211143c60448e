#!/usr/bin/env python3
"""Time per PRD call (dlpm_amd.metrics.prd_device, both inputs on the device) at the toy config's own size, N = 15000 with K = 100
clusters, and at N = 2000 with K = 20; 201 angles, 10 runs x 10 inits, up to 100 Lloyd rounds -- the reference's
compute_precision_recall_curve at its defaults.  Every shape runs in a child process of its own under its own time limit (a shape that
fails or runs out of time ends the tool): one warm-up call, then 5 calls timed one by one with device events; the median is reported.
One further call under the library's per-phase timing (dlpm_prof_*) gives the time of the k-means++ seeding, of the Lloyd rounds and
of the rest; a k-means call with the same settings gives the rounds the selected inits used.  Launches per call are counted from the
enqueue sequence: 3 + (2 K - 1) seeding + 2 max_iter Lloyd + 2 finishing + 2 curve.  One JSON line per shape.
Usage: python tools/bench_prd.py [--timeout 240] [--shape N K]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

SHAPES = [(15000, 100), (2000, 20)]
CALLS = 5
ANGLES, RUNS, INITS, MAX_ITER = 201, 10, 10, 100


def one_shape(N, K):
    import torch
    from dlpm_amd import _lib, metrics
    assert torch.cuda.is_available(), 'bench_prd.py needs the MI355X'
    g = torch.Generator(device='cuda').manual_seed(1)
    x, y = torch.randn(N, 2, device='cuda', generator=g), torch.randn(N, 2, device='cuda', generator=g) + 0.3
    kw = dict(num_clusters=K, num_angles=ANGLES, num_runs=RUNS, n_init=INITS, max_iter=MAX_ITER)
    out = metrics.prd_device(x, y, **kw)                # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = metrics.prd_device(x, y, **kw)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    L = _lib.lib()
    _lib.check(L.dlpm_prof_enable(1))
    metrics.prd_device(x, y, **kw)
    buf = C.create_string_buffer(1 << 16)
    _lib.check(L.dlpm_prof_report(buf, len(buf)))
    _lib.check(L.dlpm_prof_enable(0))
    phases = {}
    for line in buf.value.decode().splitlines():
        f = line.split()
        if len(f) >= 5 and f[0].startswith('prd_'):
            phases[f[0]] = round(float(f[2]), 4)
    total = sum(phases.values()) or 1.0
    iters = metrics.kmeans(torch.cat([x, y]), K, n_init=INITS, max_iter=MAX_ITER, runs=RUNS)[3]
    o = out.cpu().numpy()
    res = {'shape': [N, N, 2], 'clusters': K, 'angles': ANGLES, 'runs': RUNS, 'n_init': INITS, 'max_iter': MAX_ITER,
           'ms_median': round(statistics.median(ms), 4), 'ms_all': [round(v, 4) for v in ms],
           'launches': 3 + (2 * K - 1) + 2 * MAX_ITER + 2 + 2, 'iterations_of_selected_inits': [int(v) for v in iters],
           'phases_ms': phases, 'share_seeding': round(phases.get('prd_seed', 0.0) / total, 4),
           'share_lloyd': round(phases.get('prd_lloyd', 0.0) / total, 4),
           'f_pair': [float(o[2 * ANGLES]), float(o[2 * ANGLES + 1])]}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--timeout', type=int, default=240, help='seconds per shape')
    ap.add_argument('--shape', type=int, nargs=2, default=None, metavar=('N', 'K'))
    a = ap.parse_args()
    if a.shape:
        return one_shape(*a.shape)
    for shape in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--shape'] + [str(v) for v in shape], timeout=a.timeout)
        if r.returncode != 0:
            sys.exit('shape %s ended with status %d' % (shape, r.returncode))


if __name__ == '__main__':
    main()
