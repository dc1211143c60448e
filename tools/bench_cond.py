#!/usr/bin/env python3
"""Cost of class conditioning per reverse step: the unconditional and the class-conditional (K = 10, labels i % K) variant of the same
net, synthetic weights, T = 1000, alpha = 1.7, Philox noise, one captured graph per step -- measured alternately in one process, so
clocks and thermals hit both alike.  Workloads: the CIFAR net at B = 1024 and the MNIST net at B = 256 (developer tool; bench.py
measures only the unconditional workloads).  Prints one JSON line per workload with the median ms/step of each variant.
Usage: python tools/bench_cond.py [--rounds 7] [--steps 40] [--warmup 10] [--only cifar10|mnist]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch
import dlpm_amd
from dlpm_amd import _lib

WORKLOADS = [('cifar10', 1024), ('mnist', 256)]
K, T, ALPHA = 10, 1000, 1.7


def sampler(config, B, cond):
    p = dlpm_amd.load_config(config)
    p['device'] = 'cuda'
    if cond:
        p['model']['class_cond'] = True
        p['data']['num_classes'] = K
    torch.manual_seed(0)
    net = dlpm_amd.rerandomize_(dlpm_amd.init_model_by_parameter(p), 1)
    net.declare_batch(B)
    hw = p['data']['image_size']
    shape = [B, p['data']['channels'], hw, hw]
    meth = dlpm_amd.GenerativeLevyProcess(ALPHA, 'cuda', T, rescale_timesteps=True, seed=1)
    L, st = _lib.lib(), _lib.stream_ptr()
    h = meth._native_sampler(net, shape, 0, 0.0, 20.0, 200.0, 0)
    if cond:
        y = (torch.arange(B, device='cuda') % K).to(torch.int64)
        _lib.check(L.dlpm_sampler_set_labels(h, y.data_ptr(), st))
    _lib.check(L.dlpm_sampler_begin(h, st))
    return dict(net=net, meth=meth, h=h, shape=shape)


def timed(s, n):
    L, st = _lib.lib(), _lib.stream_ptr()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _lib.check(L.dlpm_sampler_steps(s['h'], n, st))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--only', default=None)
    a = ap.parse_args()
    assert a.warmup + a.rounds * a.steps <= T - 1, 'more steps than one trajectory has'
    for config, B in WORKLOADS:
        if a.only and a.only != config:
            continue
        unc, cond = sampler(config, B, False), sampler(config, B, True)
        timed(unc, a.warmup)
        timed(cond, a.warmup)
        ms = {'unconditional': [], 'conditional': []}
        for r in range(a.rounds):
            order = [('unconditional', unc), ('conditional', cond)] if r % 2 == 0 else [('conditional', cond), ('unconditional', unc)]
            for tag, s in order:
                ms[tag].append(timed(s, a.steps))
        L, st = _lib.lib(), _lib.stream_ptr()
        finite = True
        for s in (unc, cond):
            x = torch.empty(s['shape'], device='cuda')
            _lib.check(L.dlpm_sampler_copy_state(s['h'], x.data_ptr(), st))
            finite &= bool(torch.isfinite(x).all())
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({'workload': '%s_unet_b%d_T%d' % (config, B, T), 'num_classes': K,
                          'ms_per_step_unconditional': round(med['unconditional'], 4),
                          'ms_per_step_conditional': round(med['conditional'], 4),
                          'overhead_pct': round(100 * (med['conditional'] / med['unconditional'] - 1), 3),
                          'rounds': a.rounds, 'steps_per_round': a.steps, 'samples_finite': finite,
                          'all_ms': {k: [round(v, 4) for v in vs] for k, vs in ms.items()}}), flush=True)
        for s in (unc, cond):
            s['meth'].close()
        del unc, cond
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
