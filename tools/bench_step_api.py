#!/usr/bin/env python3
"""What the step-level API costs per reverse step: the MNIST net at [256,1,32,32], T = 1000, alpha = 1.7, synthetic
weights, Philox noise.  Four ways to take the same steps, measured in one process in a balanced order (see main) so that clocks and
thermals hit all alike; each timed window is `--steps` steps between two device synchronisations (host clock), the median of
`--rounds` windows is reported:

  a  loop          what p_sample_loop runs: ONE dlpm_sampler_steps call for the whole window
  b  loop_progress what p_sample_loop(progress=True) has always run: one dlpm_sampler_steps(h, 1) per step -- the baseline
  c  progressive   the native p_sample_loop_progressive generator: (b) plus one device copy of B D 4 bytes and a dict per step
  d  hand_loop     p_sample called in a Python loop: the net's forward and dlpm_update_f32 launched from Python, no graph

and dlpm_anterior_f32 alone at [1024,3072] (DLPM moments, isotropic): device events around `--launches` launches, algorithmic bytes
(read x and eps, write mean: 12 B/element) over time against the 8 TB/s HBM peak, the way tools/bench_update.py reports the update
kernel.  Prints one JSON line with the date and the board's clock and power while the windows ran (bench.py's BoardSampler).
Usage: python tools/bench_step_api.py [--rounds 8] [--steps 50] [--warmup 10] [--launches 200]"""
import argparse
import ctypes as C
import datetime
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
import torch
import dlpm_amd
from dlpm_amd import _lib
from bench import BoardSampler

B, T, ALPHA = 256, 1000, 1.7


def method():
    m = dlpm_amd.GenerativeLevyProcess(ALPHA, 'cuda', T, rescale_timesteps=True, seed=1)
    m.dlpm.gen_a.setParams(clamp_a=20.0)
    m.dlpm.gen_eps.setParams(clamp_eps=200.0)
    return m


class Loop:
    """(a) / (b): the sampler p_sample_loop drives, stepped `chunk` steps per call."""

    def __init__(self, net, shape, chunk):
        self.m, self.chunk, self.net = method(), chunk, net        # the net is kept: its samplers are destroyed with it
        self.h = self.m._native_sampler(net, shape, 0, 0.0, 20.0, 200.0, 1)
        _lib.check(_lib.lib().dlpm_sampler_begin(self.h, _lib.stream_ptr()))

    def steps(self, n):
        L, st = _lib.lib(), _lib.stream_ptr()
        for _ in range(n // self.chunk if self.chunk else 1):
            _lib.check(L.dlpm_sampler_steps(self.h, self.chunk or n, st))


class Progressive:
    """(c): the generator, one next() per step."""

    def __init__(self, net, shape):
        self.m, self.net = method(), net
        self.gen = self.m.p_sample_loop_progressive(net, shape)
        self.x = next(self.gen)['sample']

    def steps(self, n):
        for _ in range(n):
            self.x = next(self.gen)['sample']


class HandLoop:
    """(d): p_sample in a Python loop, from the x_T a progressive generator yields."""

    def __init__(self, net, shape):
        self.m, self.net, self.i = method(), net, T - 1
        self.x = next(self.m.p_sample_loop_progressive(net, shape))['sample']
        self.ts = torch.arange(T, device='cuda').view(T, 1).expand(T, shape[0])

    def steps(self, n):
        for _ in range(n):
            self.x = self.m.p_sample(self.net, self.x, self.ts[self.i])['sample']
            self.i -= 1


def timed(v, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v.steps(n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def anterior_alone(launches):
    Bk, D, Tk = 1024, 3072, 1000
    d = dlpm_amd.process.DLPM(ALPHA, 'cuda', Tk)
    d.sample_A([Bk, D], Tk, seed=1)
    d.compute_Sigmas()
    x, e = (torch.randn(Bk, D, device='cuda') for _ in range(2))
    mean, var = torch.empty_like(x), torch.empty(Bk, device='cuda')
    t = torch.tensor([500], dtype=torch.int32, device='cuda')
    a = _lib.AnteriorArgs()
    a.x_dev, a.eps_dev, a.t_dev, a.g_dev, a.bs_dev = x.data_ptr(), e.data_ptr(), t.data_ptr(), d.gammas.data_ptr(), d.barsigmas.data_ptr()
    a.Sigmas_dev, a.mean_dev, a.var_dev = d._Sigmas.data_ptr(), mean.data_ptr(), var.data_ptr()
    a.B, a.D, a.T, a.mode, a.alpha = Bk, D, Tk, _lib.ANT_DLPM, ALPHA
    L, st = _lib.lib(), _lib.stream_ptr()
    for _ in range(10):
        _lib.check(L.dlpm_anterior_f32(C.byref(a), st))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        _lib.check(L.dlpm_anterior_f32(C.byref(a), st))
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / launches
    by = 12 * Bk * D
    return dict(shape=[Bk, D], us_per_launch=round(us, 2), algorithmic_bytes=by, gb_per_s=round(by / us / 1e3, 1),
                pct_of_8tb_s_hbm_peak=round(by / us / 1e3 / 80, 1), launches=launches, finite=bool(torch.isfinite(mean).all()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--launches', type=int, default=200)
    a = ap.parse_args()
    assert a.warmup + a.rounds * a.steps <= T - 1, 'more steps than one trajectory has'
    p = dlpm_amd.load_config('mnist')
    p['device'] = 'cuda'
    hw = p['data']['image_size']
    shape = [B, p['data']['channels'], hw, hw]

    def net():
        # a net of its own per loop (the same weights): samplers that share one net share its plan, workspace and time table, and
        # what one of them binds there the others pay for
        torch.manual_seed(0)
        n = dlpm_amd.rerandomize_(dlpm_amd.init_model_by_parameter(p), 1)
        n.declare_batch(B)
        return n
    variants = [('loop', Loop(net(), shape, 0)), ('loop_progress', Loop(net(), shape, 1)), ('progressive', Progressive(net(), shape)),
                ('hand_loop', HandLoop(net(), shape))]
    for _, v in variants:
        timed(v, a.warmup)
    board = BoardSampler().start()
    ms = {k: [] for k, _ in variants}
    w0 = time.perf_counter()
    # a 4 x 4 Latin square in which every variant follows every other one once: neither a position in the round nor a fixed
    # predecessor (whose clocks and cache contents a window inherits) can pass for a difference between two variants
    square = [(0, 1, 2, 3), (1, 3, 0, 2), (2, 0, 3, 1), (3, 2, 1, 0)]
    for r in range(a.rounds):
        order = [variants[i] for i in square[r % 4]]
        for tag, v in order:
            ms[tag].append(timed(v, a.steps))
    w1 = time.perf_counter()
    board.stop()
    L = _lib.lib()
    assert all(L.dlpm_sampler_t(v.h) == T - 1 - a.warmup - a.rounds * a.steps for _, v in variants[:2]), 'a loop left its trajectory'
    med = {k: statistics.median(v) for k, v in ms.items()}
    finite = all(bool(torch.isfinite(v.x).all()) for _, v in variants[2:])
    alone = anterior_alone(a.launches)
    tele = board.window(w0, w1)
    print(json.dumps({'workload': 'mnist_unet_b%d_T%d' % (B, T), 'date': datetime.date.today().isoformat(),
                      'ms_per_step': {k: round(v, 4) for k, v in med.items()},
                      'progressive_minus_loop_progress_ms': round(med['progressive'] - med['loop_progress'], 4),
                      'copy_bytes_per_yield': 4 * B * shape[1] * hw * hw,
                      'rounds': a.rounds, 'steps_per_round': a.steps, 'warmup_steps': a.warmup, 'samples_finite': finite,
                      'all_ms': {k: [round(v, 4) for v in vs] for k, vs in ms.items()},
                      'anterior_alone': alone, 'board_power_w': tele['board_power_w'], 'sclk_mhz': tele['sclk_mhz'],
                      'board_samples': tele['samples']}), flush=True)
    for _, v in variants:
        v.m.close()


if __name__ == '__main__':
    main()
