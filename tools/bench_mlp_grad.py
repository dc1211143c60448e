"""Gradients of the toy net at any width (dlpm_amd/csrc/mlp_general_grad.hip through the autograd bridge of dlpm_amd/mlp.py) on one
GPU against a torch-eager fp32 chain with autograd on the same GPU.

    python tools/bench_mlp_grad.py [--rounds 3] [--window 0.25] [--out FILE.jsonl]

nunits in {128, 256, 512, 1024}, nblocks = 4, TE = 32, F = 2 at B in {1024, 32000}; microseconds per call of
  bridge     model(x, t) with differentiable=True, then (out * dout).sum().backward(): the forward launch, the three steps of
             dlpm_mlp_grad_backward_f32 and autograd's bookkeeping (the .grad accumulation over 60 views included);
  backward   dlpm_mlp_grad_backward_f32 alone on a preallocated workspace (row pass, weight pass, slot sum);
  eager      the same container's torch modules in eager fp32 (rocBLAS GEMMs and elementwise kernels) with torch.autograd:
             forward, the same scalar, backward;
the three alternating in one process.  FLOP of the algorithm, padding and the recomputed forward not counted: the forward's
2 (TE + TE^2 + F nunits + (nblocks + 1) (2 nunits^2 + TE nunits) + nunits F) per row, twice that again for the backward (dX and dW
of every Linear), so 3 x for the bridge and the eager chain and 2 x for the backward alone -- over the time, against the 157.3
TFLOP/s fp32 peak.  Every figure is the median of `--rounds` windows of at least `--window` seconds of device time (device events,
after a warm-up of the same shape).  One JSON line per point, then one with the date and the board's clock and power while the
windows ran."""
import argparse
import datetime
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import dlpm_amd  # noqa: E402
from dlpm_amd import _lib  # noqa: E402
from bench import BoardSampler  # noqa: E402
from bench_mlp_general import PEAK_TFLOPS, flop_per_row, measure  # noqa: E402
import mlp_general_refs as G  # noqa: E402
import mlp_grad_refs as R  # noqa: E402


def make_net(nunits, differentiable):
    torch.manual_seed(1)
    return G.perturb_norms_(dlpm_amd.MLPModel(G.config(2, 4, 32, nunits), differentiable=differentiable), 1).cuda()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of device time per timed window')
    ap.add_argument('--units', type=int, nargs='*', default=[128, 256, 512, 1024])
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_mlp_grad.py measures on the GPU; none is visible')
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)
    L = _lib.lib()
    board = BoardSampler().start()
    w0 = time.perf_counter()
    g = torch.Generator().manual_seed(5)
    for nunits in a.units:
        net, twin = make_net(nunits, True), make_net(nunits, False)
        h = net.native_handle()
        P = L.dlpm_mlp_grad_param_floats(h)
        for B in (1024, 32000):
            x, t = (2 * torch.randn(B, 1, 2, generator=g)).cuda(), torch.rand(B, generator=g).cuda()
            dout = torch.randn(B, 1, 2, generator=g).cuda()
            need = L.dlpm_mlp_grad_workspace_bytes(h, B)
            ws = torch.empty((need + 7) // 8, dtype=torch.float64, device='cuda')
            flat = torch.empty(P, device='cuda')

            def bridge():
                net.zero_grad(set_to_none=True)
                (net(x, t) * dout).sum().backward()

            def backward():
                _lib.check(L.dlpm_mlp_grad_backward_f32(h, x.data_ptr(), t.data_ptr(), dout.data_ptr(), B, flat.data_ptr(), None,
                                                        ws.data_ptr(), need, _lib.stream_ptr()))

            def eager():
                twin.zero_grad(set_to_none=True)
                (R.module_forward(twin, x, t) * dout).sum().backward()
            bridge()
            eager()
            got = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
            want = torch.cat([p.grad.reshape(-1) for p in twin.parameters()])
            diff = float((got - want).norm() / want.norm())
            med, allus, counts = measure({'bridge': bridge, 'backward': backward, 'eager': eager}, a.rounds, a.window)
            fwd = flop_per_row(net) * B
            tf = {k: (3 if k != 'backward' else 2) * fwd / (med[k] * 1e-3) / 1e12 for k in med}
            emit({'what': 'grad', 'nunits': nunits, 'nblocks': 4, 'TE': 32, 'B': B, 'params': P, 'workspace_mb': round(need / 2 ** 20, 1),
                  'bridge_us': round(med['bridge'] * 1e3, 2), 'backward_us': round(med['backward'] * 1e3, 2),
                  'eager_us': round(med['eager'] * 1e3, 2), 'eager_over_bridge': round(med['eager'] / med['bridge'], 3),
                  'forward_gflop': round(fwd / 1e9, 3), 'bridge_tflops': round(tf['bridge'], 2), 'backward_tflops': round(tf['backward'], 2),
                  'eager_tflops': round(tf['eager'], 2), 'backward_share_of_fp32_peak': round(tf['backward'] / PEAK_TFLOPS, 4),
                  'rel_l2_bridge_vs_eager': diff, 'calls_per_window': counts, 'all_us': allus})
            del ws
    tele = board.window(w0, time.perf_counter())
    board.stop()
    emit({'what': 'board', 'date': datetime.datetime.utcnow().strftime('%Y-%m-%d %H:%M UTC'), 'gpu': torch.cuda.get_device_name(0),
          'board_power_w': tele['board_power_w'], 'sclk_mhz': tele['sclk_mhz']})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
