#!/usr/bin/env python3
"""Attention kernel alone at the launch shapes of the BASELINE configs and of the geometries only the general kernel takes
(developer tool): ms per launch through dlpm_attention_f32 (the dispatch), TFLOP/s, GB/s, and ms per launch of the general kernel
(dlpm_attention_general_f32) with its ratio to the dispatch at the same shape (1.00 where the dispatch already runs it).
Launches of the two are interleaved over rounds in one process; the median of the rounds is printed."""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch
from dlpm_amd import _lib

L = _lib.lib()
SHAPES = [('cifar H8', 1024, 64, 256, 4), ('cifar H4', 1024, 16, 256, 4), ('celeba64 H16', 256, 256, 256, 4),
          ('celeba64 H8', 256, 64, 256, 4), ('mnist H16', 256, 256, 64, 4), ('mnist H8', 256, 64, 64, 4),
          # shapes the whole-head kernel does not take
          ('mnist28 H14', 256, 196, 64, 4), ('mnist28 H7', 256, 49, 64, 4), ('32x32 attn', 256, 1024, 32, 4),
          ('mnist28 H28', 256, 784, 32, 4), ('5-level 2x2', 256, 4, 64, 4), ('1 head ch 256', 256, 64, 256, 1)]


def timed(fn, qkv, out, B, T, C, heads, reps):
    st = _lib.stream_ptr()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        _lib.check(fn(qkv.data_ptr(), out.data_ptr(), B, T, C, heads, st))
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


ROUNDS = int(os.environ.get('ROUNDS', '5'))
print('%-14s %4s %4s %3s %2s  %9s %8s %7s  %9s %6s' % ('shape', 'B', 'T', 'C', 'h', 'ms', 'TFLOP/s', 'GB/s', 'general', 'ratio'))
for name, B, T, C, heads in SHAPES:
    qkv = torch.randn(B, T, 3 * C, device='cuda')
    out = torch.empty(B, T, C, device='cuda')
    fns = (L.dlpm_attention_f32, L.dlpm_attention_general_f32)
    for fn in fns:
        timed(fn, qkv, out, B, T, C, heads, 3)
    reps = max(5, min(50, int(2e10 / (4.0 * B * T * T * C + 1))))
    res = ([], [])
    for _ in range(ROUNDS):
        for i, fn in enumerate(fns):
            res[i].append(timed(fn, qkv, out, B, T, C, heads, reps))
    ms, msg = statistics.median(res[0]), statistics.median(res[1])
    fl = 4.0 * B * T * T * C
    by = 16.0 * B * T * C
    print('%-14s %4d %4d %3d %2d  %9.4f %8.1f %7.0f  %9.4f %6.2f' % (name, B, T, C, heads, ms, fl / ms / 1e9, by / ms / 1e6, msg, msg / ms))
