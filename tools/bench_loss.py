#!/usr/bin/env python3
"""Time per held-out-loss call (GenerativeLevyProcess.training_losses_dlpm, check_finite=False, Philox draws, mean estimator) beside
the bare forward of the same net at the same batch: CIFAR-10 UNet B = 1024, MNIST UNet B = 256, toy MLP B = 15000, synthetic weights.
Device events around `--calls` back-to-back calls on the call's own stream, after warm-up, the two variants alternating over
`--rounds` rounds in one process (clocks and thermals hit both alike); the median round is reported.  `--kernels` adds one pass under
the library's per-launch timing (dlpm_prof_*: HIP events around every launch) and prints, for the three loss kernels, the time per
launch and the algorithmic bytes moved / time against the HBM peak of 8 TB/s.  The forward is not changed by the loss path; the
sha256 over the forward's sources is printed so that a reader can compare it with any other revision.
Run under `rocprofv3 --kernel-trace --stats -- python tools/bench_loss.py --only mnist --rounds 1` for the profiler's own kernel times.
`--method lim` times LIM's objective instead (training_losses_lim, Philox draws, coefficients in fp64 in the kernel); with --kernels
its elements kernel is reported as lim_loss_elements beside the shared loss_terms / loss_reduce.
Usage: python tools/bench_loss.py [--rounds 5] [--calls 20] [--warmup 3] [--only cifar10|mnist|2d_data] [--kernels] [--method dlpm|lim]"""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
import torch
import dlpm_amd
from dlpm_amd import _lib

WORKLOADS = [('cifar10', 1024), ('mnist', 256), ('2d_data', 15000)]
T, ALPHA, HBM_PEAK = 1000, 1.7, 8.0e12


def forward_sources_digest():
    csrc = os.path.join(ROOT, 'dlpm_amd', 'csrc')
    h = hashlib.sha256()
    for fn in sorted(os.listdir(csrc)):
        if fn not in ('loss.hip', 'lim_loss.hip'):
            h.update(fn.encode())
            h.update(open(os.path.join(csrc, fn), 'rb').read())
    return h.hexdigest()


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', default=None)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--method', default='dlpm', choices=['dlpm', 'lim'])
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_loss.py needs the MI355X'
    digest = forward_sources_digest()
    for config, B in WORKLOADS:
        if a.only and a.only != config:
            continue
        p = dlpm_amd.load_config(config)
        p['device'] = 'cuda'
        torch.manual_seed(0)
        net = dlpm_amd.rerandomize_(dlpm_amd.init_model_by_parameter(p), 1)
        shape = [B] + dlpm_amd.config.sample_shape(p)
        x = (0.5 * torch.randn(shape, generator=torch.Generator().manual_seed(1))).to('cuda')
        t = torch.rand(B, generator=torch.Generator().manual_seed(2)).to('cuda')
        meth = dlpm_amd.GenerativeLevyProcess(ALPHA, 'cuda', T, rescale_timesteps=True, seed=1, LIM=a.method == 'lim')
        out = {}

        def forward():
            with torch.inference_mode():
                out['eps'] = net(x, t)

        def loss():
            if a.method == 'lim':
                out['loss'] = meth.training_losses_lim(net, x, clamp_eps=20, check_finite=False)
            else:
                out['loss'] = meth.training_losses_dlpm(net, x, clamp_a=20, check_finite=False)
        timed(forward, a.warmup)
        timed(loss, a.warmup)
        ms = {'forward': [], 'loss': []}
        for r in range(a.rounds):
            for tag, fn in ([('forward', forward), ('loss', loss)] if r % 2 == 0 else [('loss', loss), ('forward', forward)]):
                ms[tag].append(timed(fn, a.calls))
        med = {k: statistics.median(v) for k, v in ms.items()}
        D = x[0].numel()
        res = {'workload': '%s_b%d_T%d' % (config, B, T), 'method': a.method, 'elements': B * D, 'ms_forward': round(med['forward'], 4),
               'ms_loss_call': round(med['loss'], 4), 'ms_beyond_forward': round(med['loss'] - med['forward'], 4),
               'overhead_pct': round(100 * (med['loss'] / med['forward'] - 1), 3), 'loss': float(out['loss']),
               'rounds': a.rounds, 'calls_per_round': a.calls, 'all_ms': {k: [round(v, 4) for v in vs] for k, vs in ms.items()},
               'forward_sources_sha256': digest}
        if a.kernels:
            L = _lib.lib()
            _lib.check(L.dlpm_prof_enable(1))
            for _ in range(a.calls):
                loss()
            buf = (b' ' * (1 << 16))
            import ctypes as C
            cbuf = C.create_string_buffer(buf)
            _lib.check(L.dlpm_prof_report(cbuf, len(buf)))
            _lib.check(L.dlpm_prof_enable(0))
            kernels = {}
            for line in cbuf.value.decode().splitlines():
                f = line.split()
                if len(f) >= 5 and f[0].startswith(('loss_', 'lim_loss_')):
                    n, total_ms, nbytes = int(f[1]), float(f[2]), float(f[4])
                    us = 1e3 * total_ms / n
                    kernels[f[0]] = {'launches': n, 'us_per_launch': round(us, 2), 'bytes_per_launch': nbytes / n,
                                     'GB_per_s': round(nbytes / n / (us * 1e-6) / 1e9, 1),
                                     'pct_of_hbm_peak': round(100 * nbytes / n / (us * 1e-6) / HBM_PEAK, 2)}
            res['kernels'] = kernels
        print(json.dumps(res), flush=True)
        meth.close()
        del net, meth
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
