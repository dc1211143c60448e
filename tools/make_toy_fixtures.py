#!/usr/bin/env python
"""Generate fixture family F23 (tests/golden/f23_toy_*.npz) by IMPORTING the reference's bem/datasets/Distributions.py.

    DLPM_REFERENCE=<checkout of the reference> python tools/make_toy_fixtures.py

Needs the reference checkout, sklearn and scipy.  Nothing of the reference is copied: its module is loaded by path and called.

For each kind (gmm_2, gmm_grid, swiss_roll, sas_grid; the shipped config's n = 3, std = 0.1, theta = 3, weights, data_alpha = 1.7,
isotropic) and N in {64, 257, 1000}: numpy and torch are seeded, the reference is called once with both switches off (`raw`), and
again under the same seeds with
    norm         normalize=True
    bt99, bt100  between_minus_1_1=True, quantile_cutoff 0.99 / 1.0
    norm_bt99    normalize=True, between_minus_1_1=True, quantile_cutoff 0.99
Both calls consume the generators identically (the tool asserts that a second call with both switches off repeats the first bit for
bit), so each output is the reference's post-processing of `raw`, row for row, final shuffle included.  A setting under which the
reference itself raises is not recorded, and `<tag>_raises` says so: its two sign asserts, and swiss_roll's clamp, which hands a numpy
array to torch.quantile.  swiss_roll always normalises, so its `raw` is a replay of make_swiss_roll's three draws under the same seed;
the tool asserts that the replay, normalised in numpy, reproduces the reference's output exactly.
Also recorded: sas_grid's boundaries int(cumsum([0, w]) N) for the config's weights at N in {1, 2, 3, 64, 257, 1000, 32000}, and the
CDF of the reference's own gen_sas law (sqrt(a) z, one coordinate) at data_alpha in {1.7, 1.0, 2.0} on a 41-point grid, from one
4 000 000-point host draw each (binomial sampling error at most 0.5 / sqrt(4e6) = 2.5e-4 per point in standard deviation; the tests
allow 1e-3).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
REF = os.environ.get('DLPM_REFERENCE')
if not REF:
    sys.exit('set DLPM_REFERENCE to a checkout of the reference')
spec = importlib.util.spec_from_file_location('ref_distributions', os.path.join(REF, 'bem', 'datasets', 'Distributions.py'))
D = importlib.util.module_from_spec(spec)
spec.loader.exec_module(D)

WEIGHTS = np.array([0.01, 0.1, 0.3, 0.2, 0.02, 0.15, 0.02, 0.15, 0.05])
SIZES = (64, 257, 1000)
BOUND_SIZES = (1, 2, 3, 64, 257, 1000, 32000)
SETTINGS = {'norm': dict(normalize=True), 'bt99': dict(between_minus_1_1=True, quantile_cutoff=0.99),
            'bt100': dict(between_minus_1_1=True, quantile_cutoff=1.0),
            'norm_bt99': dict(normalize=True, between_minus_1_1=True, quantile_cutoff=0.99)}
KINDS = {'gmm_2': (D.sample_2_gmm, dict(std=0.1, theta=3.0)),
         'gmm_grid': (D.sample_grid_gmm, dict(n=3, std=0.1, weights=WEIGHTS)),
         'swiss_roll': (D.gen_swiss_roll, dict(std=0.1)),
         'sas_grid': (D.sample_grid_sas, dict(alpha=1.7, n=3, std=0.1, weights=WEIGHTS, isotropic=True))}
CDF_GRID = np.linspace(-8.0, 8.0, 41)


def call(fn, N, seed, **kw):
    np.random.seed(seed)
    torch.manual_seed(seed)
    return fn(N, **kw).numpy().copy()


def swiss_raw(N, seed, std):
    """make_swiss_roll's three draws on the global numpy generator, columns 0 and 2, in fp64."""
    np.random.seed(seed)
    t = 1.5 * np.pi * (1 + 2 * np.random.uniform(size=N))
    np.random.uniform(size=N)
    x = np.vstack((t * np.cos(t), np.zeros(N), t * np.sin(t)))
    x += std * np.random.standard_normal(size=(3, N))
    return np.ascontiguousarray(x.T[:, [0, 2]])


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    total = 0
    for ki, (kind, (fn, kw)) in enumerate(KINDS.items()):
        out = {}
        for N in SIZES:
            seed = 2300 + 10 * ki + SIZES.index(N)
            if kind == 'swiss_roll':
                raw64 = swiss_raw(N, seed, kw['std'])
                ref = call(fn, N, seed, **kw)
                replay = torch.tensor((raw64 - raw64.mean()) / raw64.std(), dtype=torch.float32).numpy()
                assert np.array_equal(replay, ref), 'the replay of make_swiss_roll does not reproduce the reference'
                out['raw64_%d' % N] = raw64
                out['raw_%d' % N] = raw64.astype(np.float32)
                out['norm_%d' % N] = ref
                settings = {k: v for k, v in SETTINGS.items() if k != 'norm'}
            else:
                raw = call(fn, N, seed, **kw)
                assert np.array_equal(raw, call(fn, N, seed, **kw)), 'two seeded calls differ'
                out['raw_%d' % N] = raw
                settings = SETTINGS
            for tag, extra in settings.items():
                try:
                    out['%s_%d' % (tag, N)] = call(fn, N, seed, **dict(kw, **extra))
                    out['%s_%d_raises' % (tag, N)] = np.array(0)
                except (AssertionError, TypeError) as e:
                    out['%s_%d_raises' % (tag, N)] = np.array(1)
                    print('%s N=%d %s: the reference raises %s' % (kind, N, tag, type(e).__name__))
        path = os.path.join(GOLDEN, 'f23_toy_%s.npz' % kind)
        np.savez_compressed(path, **out)
        total += os.path.getsize(path)
    extra = {'weights': WEIGHTS, 'bound_sizes': np.array(BOUND_SIZES), 'cdf_grid': CDF_GRID}
    for N in BOUND_SIZES:                                   # Distributions.py:212-218, evaluated by the expressions it uses
        idx = np.cumsum(np.concatenate((np.array([0.0]), WEIGHTS))) * N
        extra['bounds_%d' % N] = np.array([int(v) for v in idx], dtype=np.int64)
    for alpha in (1.7, 1.0, 2.0):
        np.random.seed(int(alpha * 10))
        torch.manual_seed(int(alpha * 10))
        x = np.sort(D.gen_sas(alpha, size=(4000000, 1), isotropic=True).numpy()[:, 0].astype(np.float64))
        extra['cdf_%s' % str(alpha).replace('.', 'p')] = np.searchsorted(x, CDF_GRID, side='right') / len(x)
    path = os.path.join(GOLDEN, 'f23_toy_tables.npz')
    np.savez_compressed(path, **extra)
    total += os.path.getsize(path)
    print('F23: %d bytes' % total)
    assert total < 300 * 1024


if __name__ == '__main__':
    main()
