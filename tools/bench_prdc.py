#!/usr/bin/env python3
"""Time per PRDC call (dlpm_amd.metrics.prdc_device, both inputs on the device, k = 5) at [50 000, 2], [10 000, 2048] and -- if free
memory allows its workspace -- [50 000, 2048], each set against a second one of the same shape; run by hand on the MI355X.

Per size, one JSON line with
  * ms per call: every size is warmed up, then REPEATS rounds visit the sizes in alternation, every call timed with device events;
    median and range;
  * the share of the three passes (radii of the real set + radii of the fake set, the cross walk, everything else: centring, norms,
    selection of the survivors, init and final) from `rocprofv3 --kernel-trace --stats` in a RUN OF ITS OWN: this script starts itself
    as a child process under the profiler, before it touches the GPU itself (`--only NAME --child`), and reads the kernel statistics;
  * for the Gram form the executed fp64-MFMA rate of the radii and cross kernels, 2 * 128 * 128 * ceil16(D) FLOP per tile, in TFLOP/s
    and as a fraction of the fp64 matrix peak (PEAK_F64_MATRIX below);
  * the obvious device baseline in the same process: torch.cdist in fp64, kthvalue per row and the four broadcast comparisons, its
    three n x n matrices alive together as in the package, at every size where they fit in half of the free memory.
Reported, not gated.
Usage: python tools/bench_prdc.py [--repeats 3] [--only NAME] [--no-passes] [--no-baseline]"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

SIZES = [('toy_50000x2', 50000, 2), ('feat_10000x2048', 10000, 2048), ('feat_50000x2048', 50000, 2048)]
K = 5
# AMD's published peak of the MI355X's fp64 matrix pipe, in FLOP/s (78.6 TFLOP/s = 32 FLOP per clock and SIMD on 256 CUs x 4 SIMDs at
# 2.4 GHz; the fp32 matrix pipe is twice that)
PEAK_F64_MATRIX = 78.6e12


def sets(torch, n, D):
    g = torch.Generator(device='cuda').manual_seed(n + D)
    real = torch.randn(n, D, device='cuda', generator=g)
    fake = torch.randn(n, D, device='cuda', generator=g) * 1.02 + 0.1 / D ** 0.5
    return real, fake


def pass_of(kernel):
    if 'k_prdc_direct' in kernel or 'k_prdc_gram' in kernel:
        return 'cross' if ('true>' in kernel.replace(' ', '') or ', true' in kernel) else 'radii'
    shared = ('k_colstats', 'k_colmean', 'k_nonfinite')         # of metrics_common.h
    return 'rest' if ('k_prdc_' in kernel or any(s in kernel for s in shared)) else None


def profile_passes(name, calls=2):
    """Kernel time per pass of `calls` calls at size `name`, measured by rocprofv3 in a child process."""
    tmp = tempfile.mkdtemp(prefix='prdc_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '--', sys.executable, os.path.abspath(__file__),
               '--only', name, '--child', '--repeats', str(calls)]
        print('profiling %s under rocprofv3 ...' % name, file=sys.stderr, flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            return {'error': (r.stdout + r.stderr)[-400:]}
        files = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
        if not files:
            return {'error': 'no kernel_stats.csv written'}
        ns, launches = {'radii': 0.0, 'cross': 0.0, 'rest': 0.0}, {'radii': 0, 'cross': 0, 'rest': 0}
        for row in csv.DictReader(open(files[0])):
            p = pass_of(row['Name'])
            if p:
                ns[p] += float(row['TotalDurationNs'])
                launches[p] += int(row['Calls'])
        total = sum(ns.values())
        per_call = calls + 1                              # the child's warm-up call is in the trace too
        return {'kernel_ms_per_call': {p: round(v / per_call * 1e-6, 4) for p, v in ns.items()},
                'share': {p: round(v / total, 4) for p, v in ns.items()} if total else {}, 'launches': launches}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def baseline(torch, real, fake, k):
    """compute_prdc as the package writes it, on the device in fp64; returns the four figures."""
    real, fake = real.double(), fake.double()
    rr, gg, rg = torch.cdist(real, real), torch.cdist(fake, fake), torch.cdist(real, fake)
    r = rr.kthvalue(k + 1, dim=1).values
    g = gg.kthvalue(k + 1, dim=1).values
    inside = rg < r[:, None]
    precision = inside.any(dim=0).double().mean()
    recall = (rg < g[None, :]).any(dim=1).double().mean()
    density = inside.sum(dim=0).double().mean() / k
    coverage = (rg.min(dim=1).values < r).double().mean()
    return torch.stack([precision, recall, density, coverage])


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--only', default=None)
    ap.add_argument('--child', action='store_true', help='the profiled run: warm-up + REPEATS calls of one size, nothing else')
    ap.add_argument('--no-passes', action='store_true')
    ap.add_argument('--no-baseline', action='store_true')
    a = ap.parse_args()
    sizes = [s for s in SIZES if a.only in (None, s[0])]
    passes = {}
    if not a.child and not a.no_passes:                   # before this process opens the GPU
        for name, n, D in sizes:
            passes[name] = profile_passes(name)
    import torch
    from dlpm_amd import _lib, metrics
    assert torch.cuda.is_available(), 'bench_prdc.py needs the MI355X'
    L = _lib.lib()
    data, skipped = {}, {}
    for name, n, D in sizes:
        need = L.dlpm_prdc_workspace_bytes(n, n, D, K) + 2 * 4 * n * D
        free = torch.cuda.mem_get_info()[0]
        if need > 0.5 * free:
            skipped[name] = 'workspace + inputs %d bytes, %d free' % (need, free)
            continue
        data[name] = sets(torch, n, D)
    outs, times = {}, {name: [] for name in data}
    for name, (x, y) in data.items():                     # warm-up
        outs[name] = metrics.prdc_device(x, y, K)
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for name, (x, y) in data.items():
            ms, outs[name] = timed(torch, lambda: metrics.prdc_device(x, y, K))
            times[name].append(ms)
    if a.child:
        return
    for name, n, D in sizes:
        if name in skipped:
            print(json.dumps({'config': name, 'skipped': skipped[name]}), flush=True)
            continue
        x, y = data[name]
        o, c = outs[name][0].cpu().numpy(), outs[name][1].cpu().numpy()
        res = {'config': name, 'n': n, 'D': D, 'k': K, 'figures': [float(v) for v in o[:4]], 'counts': c.tolist(), 'status': int(o[6]),
               'ms_median': round(statistics.median(times[name]), 3), 'ms_min': round(min(times[name]), 3),
               'ms_max': round(max(times[name]), 3), 'workspace_bytes': int(L.dlpm_prdc_workspace_bytes(n, n, D, K)),
               'passes': passes.get(name)}
        p = passes.get(name) or {}
        if D > 16 and 'kernel_ms_per_call' in p:
            tiles = -(-n // 128)
            segs = tiles                                   # every row block meets every column tile once, whatever the segmentation
            flop_tile = 2.0 * 128 * 128 * (-(-D // 16) * 16)
            for which, count in (('radii', 2 * tiles * segs), ('cross', tiles * tiles)):
                rate = count * flop_tile / (p['kernel_ms_per_call'][which] * 1e-3)
                res['mfma_f64_tflops_' + which] = round(rate * 1e-12, 2)
                res['mfma_f64_frac_' + which] = round(rate / PEAK_F64_MATRIX, 4)
        if not a.no_baseline:
            free = torch.cuda.mem_get_info()[0]
            need = 3 * 8 * n * n + 2 * n * n + 2 * 8 * n * D    # three fp64 matrices, two boolean ones, the fp64 copies of the inputs
            if need <= 0.5 * free:
                baseline(torch, x, y, K)
                torch.cuda.synchronize()
                bt = []
                for _ in range(max(1, a.repeats - 1)):
                    ms, fig = timed(torch, lambda: baseline(torch, x, y, K))
                    bt.append(ms)
                res['baseline_ms_median'] = round(statistics.median(bt), 3)
                res['baseline_figures'] = [float(v) for v in fig.cpu()]
                res['baseline_over_ours'] = round(res['baseline_ms_median'] / res['ms_median'], 2)
                torch.cuda.empty_cache()
            else:
                res['baseline_skipped'] = 'three n x n fp64 matrices need %d bytes, %d free' % (need, free)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
