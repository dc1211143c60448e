#!/usr/bin/env python3
"""ms per reverse step of the 28x28 MNIST UNet (dlpm_amd/configs/mnist28.yml, synthetic weights) at B = 256, T = 1000, alpha = 1.7,
Philox noise and one captured graph per step: the sampling loop GenerationManager runs (developer tool; bench.py measures only the
shipped workloads).  Usage: python tools/bench_mnist28.py [--batch 256] [--steps 100] [--warmup 10]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch
import dlpm_amd
from dlpm_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=256)
ap.add_argument('--steps', type=int, default=100)
ap.add_argument('--warmup', type=int, default=10)
a = ap.parse_args()
p = dlpm_amd.load_config('mnist28')
p['device'] = 'cuda'
torch.manual_seed(0)
net = dlpm_amd.rerandomize_(dlpm_amd.init_model_by_parameter(p), 1)
net.declare_batch(a.batch)
T, alpha = 1000, 1.7
meth = dlpm_amd.GenerativeLevyProcess(alpha, 'cuda', T, rescale_timesteps=True, seed=1)
L, st = _lib.lib(), _lib.stream_ptr()
h = meth._native_sampler(net, [a.batch, 1, 28, 28], 0, 0.0, 20.0, 200.0, 0)
_lib.check(L.dlpm_sampler_begin(h, st))
_lib.check(L.dlpm_sampler_steps(h, a.warmup, st))
torch.cuda.synchronize()
t0 = time.perf_counter()
_lib.check(L.dlpm_sampler_steps(h, a.steps, st))
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) * 1e3 / a.steps
x = torch.empty(a.batch, 1, 28, 28, device='cuda')
_lib.check(L.dlpm_sampler_copy_state(h, x.data_ptr(), st))
assert bool(torch.isfinite(x).all())
print('{"workload": "mnist28_unet_b%d_T1000", "ms_per_step": %.4f, "steps": %d}' % (a.batch, ms, a.steps))
meth.close()
