"""Steps per second of the toy net's training step on one GPU, against a torch-eager autograd mirror on the same GPU.

    python tools/bench_train.py [--steps 200] [--warmup 50] [--rounds 3]

The workload is the shipped 2d_data config: batches [1024, 1, 2], lploss = 2, mean estimator, AdamW at lr = 0.005, with and
without one EMA shadow (mu = 0.9).  `device` is dlpm_amd.MLPTrainer.step -- loss elements (Philox draws), forward, terms, estimator,
loss gradient, backward, AdamW + EMA, parameter import.  `torch` is the same architecture as torch.nn.functional calls with autograd,
torch.optim.AdamW and the reference's EMA update (bem/utils_ema.py) on ONE fixed batch of loss elements made beforehand: it draws
nothing per step, which favours it.  Both are timed with device events around `--steps` steps after `--warmup`, alternating, `--rounds`
times; the figures are medians.  `enqueue` is the host time to issue those steps (no synchronisation inside): where it equals the
device time, the step is bound by launches, not by the kernels.  One JSON line per variant, then a summary."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dlpm_amd  # noqa: E402


def forward(sd, x, t, nblocks):
    def block(pre, h, temb):
        y = F.layer_norm(F.linear(h, sd[pre + 'mlp_1.1.weight'], sd[pre + 'mlp_1.1.bias']), [64], sd[pre + 'group_norm1.weight'],
                         sd[pre + 'group_norm1.bias'])
        y = F.silu(y) + F.silu(F.linear(temb, sd[pre + 't_proj.1.weight'], sd[pre + 't_proj.1.bias']))
        y = F.layer_norm(F.linear(y, sd[pre + 'mlp_2.1.weight'], sd[pre + 'mlp_2.1.bias']), [64], sd[pre + 'group_norm2.weight'],
                         sd[pre + 'group_norm2.bias'])
        return F.silu(y + h)
    temb = F.silu(F.linear(t.reshape(-1, 1, 1), sd['time_emb.weight'], sd['time_emb.bias']))
    temb = F.silu(F.linear(temb, sd['time_mlp.2.weight'], sd['time_mlp.2.bias']))
    h = F.silu(F.layer_norm(F.linear(x, sd['linear_in.weight'], sd['linear_in.bias']), [64], sd['group_norm_in.weight'],
                            sd['group_norm_in.bias']))
    for i in range(nblocks):
        h = block('midblocks.%d.' % i, h, temb)
    h = block('outblocks_mean.0.', h, temb)
    return F.linear(h, sd['outblocks_mean.1.weight'], sd['outblocks_mean.1.bias'])


class TorchMirror:
    def __init__(self, net, batch, lr, ema):
        self.params = {n: p.detach().clone().cuda().requires_grad_(True) for n, p in net.named_parameters()}
        first = {id(p): n for n, p in net.named_parameters()}
        self.sd = {k: self.params[first[id(v)]] for k, v in net.state_dict(keep_vars=True).items()}
        self.nblocks = net.nblocks
        self.opt = torch.optim.AdamW(list(self.params.values()), lr=lr)
        self.shadow = {n: p.detach().clone() for n, p in self.params.items()} if ema else None
        self.x, self.t, self.eps = batch

    def step(self):
        out = forward(self.sd, self.x, self.t, self.nblocks)
        d = (out - self.eps).reshape(out.shape[0], -1)
        loss = torch.sqrt((d * d).mean(1)).mean()
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        if self.shadow is not None:
            for n, p in self.params.items():
                self.shadow[n] = (1. - 0.9) * p.detach() + 0.9 * self.shadow[n]


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    enqueue = time.perf_counter() - t0
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, 1e3 * enqueue / steps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args(argv)
    assert a.steps >= 200, 'time at least 200 steps'
    p = dlpm_amd.load_config('2d_data')
    p['device'] = 'cuda'
    B = p['training']['batch_size']
    data = dlpm_amd.get_dataset(p, 'cuda', 0)[0]
    runners = {}
    for ema in (False, True):
        torch.manual_seed(0)
        net = dlpm_amd.MLPModel(p)
        method = dlpm_amd.init_method_by_parameter(p, rng='philox', seed=0)
        tr = dlpm_amd.MLPTrainer(net, method, lr=p['optim']['lr'], ema_rates=[0.9] if ema else None)
        batches = [data[i * B:(i + 1) * B] for i in range(8)]
        state = {'i': 0}

        def dev_step(tr=tr, batches=batches, state=state):
            tr.step(batches[state['i'] % 8])
            state['i'] += 1
        r = method._loss_terms(net, batches[0], 2, 1, 1, None, None, None, keep=True)
        mirror = TorchMirror(net, (r['x_in'].clone(), r['tvec'].clone(), r['eps_t'].clone()), p['optim']['lr'], ema)
        runners[('device', ema)] = dev_step
        runners[('torch', ema)] = mirror.step
    for fn in runners.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runners}
    for _ in range(a.rounds):
        for k, fn in runners.items():                       # alternating: device, torch, device + EMA, torch + EMA
            times[k].append(timed(fn, a.steps))
    out = {}
    for (who, ema), v in times.items():
        ms, enq = statistics.median(x[0] for x in v), statistics.median(x[1] for x in v)
        out[(who, ema)] = ms
        print(json.dumps({'path': who, 'ema': ema, 'batch': B, 'steps': a.steps, 'rounds': a.rounds, 'ms_per_step': round(ms, 4),
                          'steps_per_s': round(1e3 / ms, 1), 'enqueue_ms_per_step': round(enq, 4),
                          'all_ms_per_step': [round(x[0], 4) for x in v]}))
    for ema in (False, True):
        print('%s: device %.1f steps/s, torch eager %.1f steps/s' % ('with one EMA' if ema else 'no EMA', 1e3 / out[('device', ema)],
                                                                     1e3 / out[('torch', ema)]))
    return out


if __name__ == '__main__':
    main()
