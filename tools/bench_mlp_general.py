"""The general toy-net forward (dlpm_amd/csrc/mlp_general.hip) on one GPU against a torch-eager mirror on the same GPU.

    python tools/bench_mlp_general.py [--rounds 3] [--window 0.25] [--out FILE.jsonl]

1. forward   nunits in {128, 256, 512, 1024}, nblocks = 4, TE = 32, F = 2 at B in {1024, 32000}: microseconds per call of
             dlpm_mlp_forward (one launch) and of the functional mirror of tests/mlp_general_refs.py in torch eager (rocBLAS GEMMs and
             elementwise kernels), the two alternating in one process; the algorithm's FLOP -- 2 (TE + TE^2 + F nunits +
             (nblocks + 1) (2 nunits^2 + TE nunits) + nunits F) per row, padding not counted -- over the time against the 157.3 TFLOP/s
             fp32 peak; the tile height M the launcher takes at that B and the LDS bytes of a workgroup.
2. shipped   the shipped 64-unit net on the general kernel against the lane kernel at B in {512, 32000}.
3. sample    a whole sample() call of the 256-unit net, [32000, 1, 2], T = 100 (the per-step graph path), in ms per step.
Every figure is the median of `--rounds` windows of at least `--window` seconds of device time (device events, after a warm-up of
the same shape).  One JSON line per point, then one with the date and the board's clock and power while the windows ran."""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dlpm_amd  # noqa: E402
from dlpm_amd import _lib  # noqa: E402
from bench import BoardSampler  # noqa: E402
import mlp_general_refs as R  # noqa: E402

PEAK_TFLOPS = 157.3


def flop_per_row(net):
    nu, te, f, nb = net.nunits, net.time_emb_size, net.nfeatures, net.nblocks + 1
    return 2 * (te + te * te + f * nu + nb * (2 * nu * nu + te * nu) + nu * f)


def chosen_tile(tallest, B):
    """The tile height a call of B rows takes (mlp_general_forward: 32 rows where they fit and make GEN_FILL_TILES tiles)."""
    return 16 if tallest == 32 and -(-B // 32) < 256 else tallest


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n          # ms per call


def measure(fns, rounds, seconds):
    """{name: median ms per call}, the callables alternating in every round."""
    counts = {}
    for k, fn in fns.items():
        window(fn, 3)
        counts[k] = max(10, int(seconds * 1e3 / max(window(fn, 5), 1e-3)))
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(window(fn, counts[k]))
    return {k: statistics.median(v) for k, v in ms.items()}, {k: [round(x * 1e3, 2) for x in v] for k, v in ms.items()}, counts


def eager_mirror(net, x, t):
    sd = {k: v.detach().float().cuda() for k, v in net.state_dict().items()}
    import torch.nn.functional as F

    def norm(pre, v):
        return F.layer_norm(v, [v.shape[-1]], sd[pre + '.weight'], sd[pre + '.bias']) if net.group_norm else v

    def block(pre, h, temb):
        y = F.silu(norm(pre + 'group_norm1', F.linear(h, sd[pre + 'mlp_1.1.weight'], sd[pre + 'mlp_1.1.bias'])))
        y = y + F.silu(F.linear(temb, sd[pre + 't_proj.1.weight'], sd[pre + 't_proj.1.bias']))
        y = norm(pre + 'group_norm2', F.linear(y, sd[pre + 'mlp_2.1.weight'], sd[pre + 'mlp_2.1.bias']))
        return F.silu(y + h if net.skip_connection else y)

    def run():
        temb = F.silu(F.linear(t.reshape(-1, 1, 1), sd['time_emb.weight'], sd['time_emb.bias']))
        temb = F.silu(F.linear(temb, sd['time_mlp.2.weight'], sd['time_mlp.2.bias']))
        h = F.silu(norm('group_norm_in', F.linear(x, sd['linear_in.weight'], sd['linear_in.bias'])))
        for i in range(net.nblocks):
            h = block('midblocks.%d.' % i, h, temb)
        h = block('outblocks_mean.0.', h, temb)
        return F.linear(h, sd['outblocks_mean.1.weight'], sd['outblocks_mean.1.bias'])
    return run


def make_net(nunits, nblocks=4, te=32, kernel='auto'):
    torch.manual_seed(1)
    return R.perturb_norms_(dlpm_amd.MLPModel(R.config(2, nblocks, te, nunits), kernel=kernel), 1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of device time per timed window')
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_mlp_general.py measures on the GPU; none is visible')
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)
    L = _lib.lib()
    board = BoardSampler().start()
    w0 = time.perf_counter()
    g = torch.Generator().manual_seed(5)
    with torch.inference_mode():
        for nunits in (128, 256, 512, 1024):
            net = make_net(nunits)
            h = net.native_handle()
            for B in (1024, 32000):
                x, t = (2 * torch.randn(B, 1, 2, generator=g)).cuda(), torch.rand(B, generator=g).cuda()
                mirror = eager_mirror(net, x, t)
                err = float((net(x, t) - mirror()).abs().max())
                med, allus, counts = measure({'kernel': lambda: net(x, t), 'eager': mirror}, a.rounds, a.window)
                fl = flop_per_row(net) * B
                tallest = L.dlpm_mlp_tile_rows(h)
                rows = chosen_tile(tallest, B)
                emit({'what': 'forward', 'nunits': nunits, 'nblocks': 4, 'TE': 32, 'B': B, 'tile_rows': rows,
                      'lds_bytes': L.dlpm_mlp_lds_bytes(h) * rows // tallest, 'kernel_us': round(med['kernel'] * 1e3, 2), 'eager_us': round(med['eager'] * 1e3, 2),
                      'eager_over_kernel': round(med['eager'] / med['kernel'], 3), 'gflop': round(fl / 1e9, 3),
                      'kernel_tflops': round(fl / (med['kernel'] * 1e-3) / 1e12, 2), 'eager_tflops': round(fl / (med['eager'] * 1e-3) / 1e12, 2),
                      'kernel_share_of_fp32_peak': round(fl / (med['kernel'] * 1e-3) / 1e12 / PEAK_TFLOPS, 4),
                      'max_abs_diff_kernel_eager': err, 'calls_per_window': counts, 'all_us': allus})
        general, lane = make_net(64, kernel='general'), make_net(64)
        for B in (512, 32000):
            x, t = (2 * torch.randn(B, 1, 2, generator=g)).cuda(), torch.rand(B, generator=g).cuda()
            err = float((general(x, t) - lane(x, t)).abs().max())
            med, allus, counts = measure({'general': lambda: general(x, t), 'lane': lambda: lane(x, t)}, a.rounds, a.window)
            emit({'what': 'shipped', 'B': B, 'general_us': round(med['general'] * 1e3, 2), 'lane_us': round(med['lane'] * 1e3, 2),
                  'lane_over_general': round(med['lane'] / med['general'], 3),
                  'tile_rows': chosen_tile(L.dlpm_mlp_tile_rows(general.native_handle()), B),
                  'max_abs_diff': err, 'calls_per_window': counts, 'all_us': allus})
        net, T, B = make_net(256), 100, 32000
        meth = dlpm_amd.GenerativeLevyProcess(1.7, 'cuda', T, rescale_timesteps=True, seed=3)
        meth.sample({'default': net}, [B, 1, 2], T)
        torch.cuda.synchronize()
        ms = []
        for _ in range(max(3, a.rounds)):
            t0 = time.perf_counter()
            out = meth.sample({'default': net}, [B, 1, 2], T)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        emit({'what': 'sample', 'nunits': 256, 'shape': [B, 1, 2], 'T': T, 'ms_per_call': round(statistics.median(ms), 3),
              'ms_per_step': round(statistics.median(ms) / T, 4), 'all_ms_per_call': [round(v, 3) for v in ms],
              'finite': bool(torch.isfinite(out).all())})
        meth.close()
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
