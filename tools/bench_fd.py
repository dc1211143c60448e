#!/usr/bin/env python3
"""Time per Frechet-distance call (dlpm_amd.metrics.fd_device, both inputs on the device) at (N, F) = (10 000, 2048), (50 000, 2048)
and (10 000, 3072), each set against a second one of the same shape; run by hand on the MI355X.

Per size, one JSON line with
  * ms per call: every size is warmed up, then REPEATS rounds visit the sizes in alternation, every call timed with device events
    around the whole call (it ends in host synchronisations of its own: one per Jacobi sweep); median and range;
  * the breakdown of ONE further call by the library's own event brackets (dlpm_prof_enable): the statistics of the two sets
    (fd_stats), the eigen-solve of sigma1 (fd_jacobi_1), the two F x F x F products with the scaling between them (fd_gemm), the
    eigen-solve of K (fd_jacobi_2), in ms and as shares, with the sweep counts and the number of Jacobi launches (rounds x sweeps);
  * the executed fp64-MFMA rate of the covariance pass and of the two products, from the FLOP the algorithm needs
    (2 n F (F + 128) / 2 per set for the upper-triangle tiles, 2 F^3 per product) over the bracketed time, as a fraction of the fp64
    matrix peak -- a bracket holds the small kernels around the tile kernel too, so this is a lower bound of the kernel's own rate;
  * at (10 000, 2048) the reference's recipe on the host of the same machine: np.cov of both sets and calculate_frechet_distance
    (scipy's fractional_matrix_power) as tests/test_fd_cpu.py restates it, wall clock, and its figure beside the device's; and the
    oracle's figure (no covariance formed) with the distance of both from it.
Reported, not gated.
Usage: python tools/bench_fd.py [--repeats 3] [--only NAME] [--no-host]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SIZES = [('feat_10000x2048', 10000, 2048), ('feat_50000x2048', 50000, 2048), ('flat_10000x3072', 10000, 3072)]
HOST_REFERENCE_AT = 'feat_10000x2048'
PEAK_F64_MATRIX = 78.6e12                  # AMD's published fp64 matrix peak of the MI355X, FLOP/s
SCOPES = ('fd_stats', 'fd_jacobi_1', 'fd_gemm', 'fd_jacobi_2')


def sets(torch, n, F):
    """Correlated features with a decaying spectrum, as a feature net's are: z A with a fixed random A, column scales 1 / (1 + d / 64)."""
    g = torch.Generator(device='cuda').manual_seed(n + F)
    A = torch.randn(F, F, device='cuda', generator=g) / F ** 0.5
    s = 1.0 / (1.0 + torch.arange(F, device='cuda') / 64.0)
    real = (torch.randn(n, F, device='cuda', generator=g) * s) @ A
    fake = (torch.randn(n, F, device='cuda', generator=g) * s * 1.05) @ A + 0.02
    return real.contiguous(), fake.contiguous()


def qr_oracle(np, x, y):
    """The figure of the oracle np_fd (tests/test_fd_cpu.py) by a cheaper route for n > F: with A = Q_a R_a and B = Q_b R_b the
    singular values of A B^T are those of the F x F matrix R_a R_b^T.  No covariance is formed."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    A = (x - x.mean(axis=0)) / np.sqrt(len(x) - 1)
    B = (y - y.mean(axis=0)) / np.sqrt(len(y) - 1)
    sv = np.linalg.svd(np.linalg.qr(A, mode='r') @ np.linalg.qr(B, mode='r').T, compute_uv=False)
    dm, t1, t2 = float(((x.mean(axis=0) - y.mean(axis=0)) ** 2).sum()), float((A * A).sum()), float((B * B).sum())
    return dm + t1 + t2 - 2 * float(sv.sum()), t1 + t2, float(sv[-1] / sv[0])


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def breakdown(torch, L, metrics, x, y):
    """ms per scope of one call, from the library's event brackets."""
    L.dlpm_prof_enable(1)
    try:
        out = metrics.fd_device(x, y)
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 16)
        assert L.dlpm_prof_report(buf, len(buf)) == 0
    finally:
        L.dlpm_prof_enable(0)
    ms = {k: 0.0 for k in SCOPES}
    for line in buf.value.decode().splitlines():
        name, launches, t = line.split()[:3]
        if name in ms:
            ms[name] += float(t)
    return ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--only', default=None)
    ap.add_argument('--no-host', action='store_true')
    a = ap.parse_args()
    sizes = [s for s in SIZES if a.only in (None, s[0])]
    import numpy as np
    import torch
    from dlpm_amd import _lib, metrics
    assert torch.cuda.is_available(), 'bench_fd.py needs the MI355X'
    L = _lib.lib()
    data, skipped = {}, {}
    for name, n, F in sizes:
        need = L.dlpm_fd_workspace_bytes(n, n, F) + 2 * 4 * n * F
        free = torch.cuda.mem_get_info()[0]
        if need > 0.5 * free:
            skipped[name] = 'workspace + inputs %d bytes, %d free' % (need, free)
            continue
        data[name] = sets(torch, n, F)
    outs, times = {}, {name: [] for name in data}
    for name, (x, y) in data.items():                     # warm-up
        outs[name] = metrics.fd_device(x, y)
        print('warmed up %s' % name, file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for name, (x, y) in data.items():
            ms, outs[name] = timed(torch, lambda: metrics.fd_device(x, y))
            times[name].append(ms)
            print('%s: %.1f ms' % (name, ms), file=sys.stderr, flush=True)
    for name, n, F in sizes:
        if name in skipped:
            print(json.dumps({'config': name, 'skipped': skipped[name]}), flush=True)
            continue
        x, y = data[name]
        scopes, out2 = breakdown(torch, L, metrics, x, y)
        o = outs[name].cpu().numpy()
        assert np.array_equal(o, out2.cpu().numpy(), equal_nan=True), 'the profiled call gave other bits'
        total = sum(scopes.values())
        rounds = F - 1 + (F & 1)
        res = {'config': name, 'n': n, 'F': F, 'fd': float(o[0]), 'terms': [float(v) for v in o[1:5]], 'status': int(o[5]),
               'sweeps': [int(o[6]), int(o[7])], 'jacobi_launches': [rounds * int(o[6]), rounds * int(o[7])],
               'ms_median': round(statistics.median(times[name]), 2), 'ms_min': round(min(times[name]), 2),
               'ms_max': round(max(times[name]), 2), 'workspace_bytes': int(L.dlpm_fd_workspace_bytes(n, n, F)),
               'scope_ms': {k: round(v, 3) for k, v in scopes.items()},
               'scope_share': {k: round(v / total, 4) for k, v in scopes.items()} if total else {}}
        T = -(-F // 128)
        cov_flop = 2 * (2.0 * n * (T * (T + 1) // 2) * 128 * 128)              # both sets, upper-triangle tiles
        gemm_flop = 2 * (2.0 * (T * 128) ** 2 * F)
        for key, flop, scope in (('cov', cov_flop, 'fd_stats'), ('gemm', gemm_flop, 'fd_gemm')):
            if scopes[scope] > 0:
                rate = flop / (scopes[scope] * 1e-3)
                res['mfma_f64_tflops_' + key] = round(rate * 1e-12, 2)
                res['mfma_f64_frac_' + key] = round(rate / PEAK_F64_MATRIX, 4)
        us = scopes['fd_jacobi_1'] * 1e3 / max(1, rounds * int(o[6]))
        res['jacobi_1_us_per_round'] = round(us, 2)
        res['jacobi_2_us_per_round'] = round(scopes['fd_jacobi_2'] * 1e3 / max(1, rounds * int(o[7])), 2)
        if name == HOST_REFERENCE_AT and not a.no_host:
            from test_fd_cpu import np_stats, reference_recipe
            xh, yh = x.cpu().numpy(), y.cpu().numpy()
            print('the reference recipe on the host ...', file=sys.stderr, flush=True)
            t0 = time.perf_counter()
            s1, s2 = np_stats(xh), np_stats(yh)
            t1 = time.perf_counter()
            ref = reference_recipe(*s1, *s2)
            t2 = time.perf_counter()
            res['host_np_cov_s'] = round(t1 - t0, 2)
            res['host_frechet_s'] = round(t2 - t1, 2)
            res['host_fd'] = ref
            res['host_over_ours'] = round((t2 - t0) * 1e3 / res['ms_median'], 2)
            res['host_threads'] = os.cpu_count() if 'OMP_NUM_THREADS' not in os.environ else int(os.environ['OMP_NUM_THREADS'])
            print('the oracle on the host ...', file=sys.stderr, flush=True)
            oracle, scale, ratio = qr_oracle(np, xh, yh)
            res['oracle_fd'] = oracle
            res['ours_minus_oracle'] = res['fd'] - oracle
            res['host_minus_oracle'] = ref - oracle
            res['model_floor'] = 64 * F * 2.0 ** -53 * scale            # 64 F EPS (tr sigma1 + tr sigma2), tests/test_fd_cpu.py bound_of
            res['smallest_over_largest_singular_value'] = ratio
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
