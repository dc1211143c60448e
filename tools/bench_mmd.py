#!/usr/bin/env python3
"""Time per MMD call (dlpm_amd.metrics.mmd_device, both inputs on the device) at the toy config's own size, (15000, 15000, 2) -- the
direct form -- and at CIFAR size, (10000, 10000, 3072) -- the Gram form.  Every shape runs in a child process of its own under its own
time limit (a shape that fails or runs out of time ends the tool): one warm-up call, then 5 calls timed one by one with device
events; the median is reported.  One further call under the library's per-launch timing (dlpm_prof_*) gives the time of each pass,
and for the Gram pass the multiply-adds it executes (the upper-triangle tiles, 128 x 128 x D each) / time against the fp32 matrix
peak of 157.3 TFLOP/s.  One JSON line per shape.
Usage: python tools/bench_mmd.py [--timeout 240] [--shape N1 N2 D]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

SHAPES = [(15000, 15000, 2), (10000, 10000, 3072)]
FP32_MATRIX_PEAK = 157.3e12
CALLS = 5


def one_shape(n1, n2, D):
    import torch
    from dlpm_amd import _lib, metrics
    assert torch.cuda.is_available(), 'bench_mmd.py needs the MI355X'
    g = torch.Generator(device='cuda').manual_seed(1)
    if D <= 16:
        x, y = torch.randn(n1, D, device='cuda', generator=g), torch.randn(n2, D, device='cuda', generator=g) + 0.1
    else:
        x, y = torch.rand(n1, D, device='cuda', generator=g), torch.rand(n2, D, device='cuda', generator=g) ** 1.1
    out = metrics.mmd_device(x, y)                      # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = metrics.mmd_device(x, y)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    L = _lib.lib()
    _lib.check(L.dlpm_prof_enable(1))
    metrics.mmd_device(x, y)
    buf = C.create_string_buffer(1 << 16)
    _lib.check(L.dlpm_prof_report(buf, len(buf)))
    _lib.check(L.dlpm_prof_enable(0))
    passes = {}
    for line in buf.value.decode().splitlines():
        f = line.split()
        if len(f) >= 5 and f[0].startswith('mmd_'):
            passes[f[0]] = {'ms': round(float(f[2]) / int(f[1]), 4), 'flop': float(f[3]) / int(f[1])}
    res = {'shape': [n1, n2, D], 'form': 'direct' if D <= 16 else 'gram', 'ms_median': round(statistics.median(ms), 4),
           'ms_all': [round(v, 4) for v in ms], 'mmd': float(out[0]), 'bandwidth': float(out[1]),
           'passes_ms': {k: v['ms'] for k, v in passes.items()}}
    if 'mmd_gram' in passes:
        rate = passes['mmd_gram']['flop'] / (passes['mmd_gram']['ms'] * 1e-3)
        res['gram_tflops_executed'] = round(rate / 1e12, 2)
        res['gram_fraction_of_fp32_matrix_peak'] = round(rate / FP32_MATRIX_PEAK, 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--timeout', type=int, default=240, help='seconds per shape')
    ap.add_argument('--shape', type=int, nargs=3, default=None, metavar=('N1', 'N2', 'D'))
    a = ap.parse_args()
    if a.shape:
        return one_shape(*a.shape)
    for shape in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--shape'] + [str(v) for v in shape], timeout=a.timeout)
        if r.returncode != 0:
            sys.exit('shape %s ended with status %d' % (shape, r.returncode))


if __name__ == '__main__':
    main()
