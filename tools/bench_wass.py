#!/usr/bin/env python3
"""Time per Wasserstein call (dlpm_amd.metrics.wass_device, both inputs on the device): the toy workload, [50 000, 2] against itself
with 250 bins (launch-latency bound: a few hundred KB), and [8192, 3072] against a second set with 250 bins and with numpy's 'auto'
rule -- streaming passes of 4 B per value: range + histogram for fixed bins, range + 4 radix-select passes + histogram for 'auto'.
All configurations run in ONE process: each is warmed up, then REPEATS rounds visit them in alternation, every call timed with
device events; median and range per configuration.  One further call under the library's per-launch timing (dlpm_prof_*) gives the
time of each streaming stage, from it the bytes/s per pass, and for the large shape the ratio to the 3.91 TB/s that the fused
update kernel (k_update, 574.6 MB in 0.1468 ms) reaches in this project's records.  One JSON line per configuration; reported, not
gated.
Usage: python tools/bench_wass.py [--repeats 7]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

K_UPDATE_BYTES_PER_S = 574.6e6 / 0.1468e-3          # the project's own record of a streaming kernel
PASSES = {'wass_range': 1, 'wass_select': 4, 'wass_hist': 1}


def main():
    import torch
    from dlpm_amd import _lib, metrics
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_wass.py needs the MI355X'
    g = torch.Generator(device='cuda').manual_seed(1)
    toy = torch.randn(50000, 2, device='cuda', generator=g)
    big1, big2 = torch.rand(8192, 3072, device='cuda', generator=g), torch.rand(8192, 3072, device='cuda', generator=g) ** 1.1
    configs = [('toy_50000x2_self_bins250', toy, toy, 250), ('img_8192x3072_bins250', big1, big2, 250),
               ('img_8192x3072_auto', big1, big2, 'auto')]
    times = {name: [] for name, *_ in configs}
    outs = {}
    for name, x, y, bins in configs:                    # warm-up of every configuration
        outs[name] = metrics.wass_device(x, y, bins=bins)
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for name, x, y, bins in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            outs[name] = metrics.wass_device(x, y, bins=bins)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    L = _lib.lib()
    for name, x, y, bins in configs:
        _lib.check(L.dlpm_prof_enable(1))
        metrics.wass_device(x, y, bins=bins)
        buf = C.create_string_buffer(1 << 16)
        _lib.check(L.dlpm_prof_report(buf, len(buf)))
        _lib.check(L.dlpm_prof_enable(0))
        nbytes = 4.0 * (x.numel() + y.numel())
        stages = {}
        for line in buf.value.decode().splitlines():
            f = line.split()
            if len(f) >= 3 and f[0] in PASSES:
                ms = float(f[2]) / int(f[1])
                stages[f[0]] = {'ms': round(ms, 4), 'passes': PASSES[f[0]],
                                'bytes_per_s_per_pass': round(nbytes * PASSES[f[0]] / (ms * 1e-3), 0)}
        o = outs[name].cpu().numpy()
        res = {'config': name, 'bins': int(o[1]), 'wass': float(o[0]), 'status': int(o[11]), 'ms_median': round(statistics.median(times[name]), 4),
               'ms_min': round(min(times[name]), 4), 'ms_max': round(max(times[name]), 4), 'bytes_per_pass': nbytes, 'stages': stages}
        if name.startswith('img'):
            for k, v in stages.items():
                v['ratio_to_k_update'] = round(v['bytes_per_s_per_pass'] / K_UPDATE_BYTES_PER_S, 4)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
