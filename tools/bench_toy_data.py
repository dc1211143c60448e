#!/usr/bin/env python3
"""Wall time of dlpm_amd.get_dataset (train + test, each [nsamples, 1, 2], drawn on the device) for the shipped 2-D config at its own
nsamples = 32000, and for the other three kinds with the same description; run by hand on the MI355X.

Per kind one JSON line with the median and range of REPEATS calls, each bracketed by device synchronisations (host wall clock: the
call is a handful of small launches, so this is launch latency and allocation, not bandwidth), after one warm-up call.
--host-reference times instead, without a GPU, the reference's own host generator for the config (its sample_grid_gmm, train + test),
imported by path from the checkout that DLPM_REFERENCE names, on the machine the tool runs on.  Reported, not gated.
Usage: python tools/bench_toy_data.py [--repeats 7] [--nsamples N] [--host-reference]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)


def reference_host_ms(d, repeats):
    """The reference's own sample_grid_gmm for the same description, train + test, timed through its module loaded by path."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('ref_distributions', os.path.join(os.environ['DLPM_REFERENCE'], 'bem', 'datasets',
                                                                                    'Distributions.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    side = int(round(d['n_mixture'] ** 0.5))
    out = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        for _split in range(2):
            ref.sample_grid_gmm(d['nsamples'], n=side, std=d['std'], weights=d['weights'])
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]                                        # the first call pays sklearn's imports


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--nsamples', type=int, default=None)
    ap.add_argument('--host-reference', action='store_true')
    a = ap.parse_args()
    import torch
    import dlpm_amd
    p = dlpm_amd.load_config('2d_data')
    if a.nsamples:
        p['data']['nsamples'] = a.nsamples
    if a.host_reference:
        ms = reference_host_ms(p['data'], a.repeats)
        print(json.dumps(dict(kind='gmm_grid', nsamples=p['data']['nsamples'], reference_host_ms_median=round(statistics.median(ms), 3),
                              reference_host_ms_range=[round(min(ms), 3), round(max(ms), 3)], torch_threads=torch.get_num_threads())))
        return

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for kind in ('gmm_grid', 'gmm_2', 'swiss_roll', 'sas_grid'):
        q = dict(p, data=dict(p['data'], dataset=kind, weights=p['data']['weights'] if kind.endswith('grid') else None))
        call = lambda: dlpm_amd.get_dataset(q, 'cuda', 0)
        call()
        ms = [timed(call) for _ in range(a.repeats)]
        line = dict(kind=kind, nsamples=q['data']['nsamples'], device_ms_median=round(statistics.median(ms), 3),
                    device_ms_range=[round(min(ms), 3), round(max(ms), 3)], device=torch.cuda.get_device_name(0))
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
