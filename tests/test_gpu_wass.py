"""The device Wasserstein figure on the MI355X against `np_wass` (tests/test_wass_cpu.py): np.histogram's integer counts bin for bin,
the value within a derived rounding bound of the exact rational figure, numpy's 'auto' bin rule with its exact order statistics,
numpy's refusals, reproducibility, graph capture, the drop-in, and EvaluationManager.evaluate_wass / evaluate_metrics_2d / the CLI end
to end.  Every test prints the figures it measured before it asserts."""
import functools
import math

import numpy as np
import pytest
import torch

from dlpm_amd import metrics
from metric_helpers import managers, real_toy, toy
from test_wass_cpu import AUTO_CASES, auto_ratio, np_wass, sets, value_bound

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def ints17():
    g = np.random.default_rng(21)
    a, b = g.integers(-8, 9, (50, 2)).astype(np.float32), g.integers(-8, 9, (41, 2)).astype(np.float32)
    a[0, 0], b[0, 0], a[1, 1] = -8.0, 8.0, 8.0              # both ends present: the maximum falls in the closed last bin
    return a, b


def offset_base():
    """37 x 3 against 64 x 3 values; the first set starts one float into its buffer (a base pointer that is not 16-byte aligned)."""
    a, b = sets(22, 37, 64, 3)
    buf = torch.zeros(1 + a.size, dtype=torch.float32)
    buf[1:] = torch.from_numpy(a).reshape(-1)
    x = buf.to(DEV)[1:].view(37, 3)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    return (x, torch.from_numpy(b)), (a, b)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> ((first, second) as given to the device, (first, second) as numpy, bins, range)"""
    if name == 'all_equal_auto' or name == 'all_equal_10':
        a, b = np.full((7, 3), 1.25, np.float32), np.full((5, 3), 1.25, np.float32)
        return None, (a, b), 'auto' if name.endswith('auto') else 10, None
    if name == 'offset_37x3_64x3':
        dev, host = offset_base()
        return dev, host, 20, None
    if name == 'integers_on_edges':
        return None, ints17(), 16, None
    if name == 'narrow_range':
        return None, sets(23, 90, 70, 2), 24, (-0.5, 0.75)
    if name in ('lds_16384', 'global_16385'):
        return None, sets(24, 5000, 5000, 2), int(name.split('_')[1]), None
    if name == 'reference_call_600':
        a, b = sets(25, 600, 600, 2)
        return None, (a.reshape(600, 1, 2), b.reshape(600, 1, 2)), 250, None
    if name == 'many_workgroups':
        return None, sets(26, 64, 48, 3072), 250, None
    raise KeyError(name)


COUNT_CASES = ['all_equal_auto', 'all_equal_10', 'offset_37x3_64x3', 'integers_on_edges', 'narrow_range', 'lds_16384', 'global_16385',
               'reference_call_600', 'many_workgroups']


@functools.lru_cache(maxsize=None)
def oracle(name):
    _, host, bins, rng = case(name)
    return np_wass(host[0], host[1], bins, rng)


def check_counts_and_value(tag, got, parts, want, wp):
    err = abs(got - want)
    print('\n%s: bins %d (numpy %d)  lo %r hi %r (numpy %r %r)  counts differ in %d + %d bins  wass %.17g  exact %.17g  |diff| %.3g  '
          'bound %.3g' % (tag, parts['bins'], wp['bins'], parts['lo'], parts['hi'], wp['lo'], wp['hi'],
                          int((parts['hist_first'] != wp['hist_first']).sum()) if parts['bins'] == wp['bins'] else -1,
                          int((parts['hist_second'] != wp['hist_second']).sum()) if parts['bins'] == wp['bins'] else -1, got, want, err,
                          value_bound(wp)))
    assert parts['bins'] == wp['bins'] and parts['lo'] == wp['lo'] and parts['hi'] == wp['hi']
    assert parts['hist_first'].dtype == np.int32 and parts['hist_first'].shape == (wp['bins'],)
    assert np.array_equal(parts['hist_first'], wp['hist_first']) and np.array_equal(parts['hist_second'], wp['hist_second'])
    assert err <= value_bound(wp)


@pytest.mark.parametrize('name', COUNT_CASES)
def test_counts_equal_numpy_and_value_is_within_the_rounding_bound(name):
    dev, host, bins, rng = case(name)
    first, second = dev if dev is not None else (torch.from_numpy(host[0]), torch.from_numpy(host[1]))
    got, parts = metrics.wass(first, second, bins=bins, range=rng, return_parts=True)
    want, wp = oracle(name)
    check_counts_and_value(name, got, parts, want, wp)
    if name.startswith('all_equal'):
        assert got == 0.0 and (parts['lo'], parts['hi']) == (0.75, 1.75)
    if name == 'narrow_range':
        assert wp['hist_first'].sum() < host[0].size and wp['hist_second'].sum() < host[1].size     # values were dropped
    if name == 'integers_on_edges':
        assert wp['hist_first'][-1] >= 2 and parts['width'] == 1.0


def test_one_value_per_set_through_the_drop_in():
    data = torch.tensor([[[0.25]], [[9.0]]])
    gen = torch.tensor([[[-1.5]], [[7.0]]])
    got = metrics.compute_wasserstein_distance(data, gen)
    again, parts = metrics.wass(gen[:-1], data[:-1], return_parts=True)
    want, wp = np_wass(gen[:-1].numpy(), data[:-1].numpy())
    check_counts_and_value('one value per set', got, parts, want, wp)
    assert got == again and parts['hist_first'].sum() == 1 and parts['hist_second'].sum() == 1


@pytest.mark.parametrize('name', sorted(AUTO_CASES))
def test_auto_rule_order_statistics_quartiles_and_bins(name):
    first, second = AUTO_CASES[name]()
    ratio, _ = auto_ratio(first, second)
    assert abs(ratio - round(ratio)) >= 1e-3                  # the precondition, from numpy alone (also a CPU test)
    pooled = np.concatenate([first.ravel(), second.ravel()])
    m = pooled.size
    ranks = [int(math.floor((m - 1) * 0.75)), int(math.floor((m - 1) * 0.75)) + 1, int(math.floor((m - 1) * 0.25)),
             int(math.floor((m - 1) * 0.25)) + 1]
    want_os = np.partition(pooled, ranks)[ranks]
    q75, q25 = np.percentile(pooled, [75, 25])
    got, parts = metrics.wass(torch.from_numpy(first), torch.from_numpy(second), return_parts=True)
    want, wp = np_wass(first, second)
    ulp = [float(np.spacing(np.float32(abs(q)))) for q in (q25, q75)]
    print('\n%s: order statistics %s (numpy %s)  q25 %r (numpy %r)  q75 %r (numpy %r)  ratio %.6f  width %r' % (
        name, parts['order_stats'], want_os, parts['q25'], q25, parts['q75'], q75, ratio, parts['width']))
    assert parts['order_stats'].dtype == np.float32
    assert np.array_equal(parts['order_stats'].view(np.uint32), want_os.view(np.uint32))
    assert abs(parts['q25'] - q25) <= ulp[0] and abs(parts['q75'] - q75) <= ulp[1]
    check_counts_and_value(name, got, parts, want, wp)


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')])
def test_non_finite_input_raises_as_numpy(bad):
    a, b = sets(27, 40, 40, 2)
    b[17, 1] = bad
    x, y = torch.from_numpy(a), torch.from_numpy(b)
    outs = {bins: metrics.wass_device(x, y, bins=bins).cpu().numpy() for bins in (16, 'auto')}
    for name, r in (('range to inf', (0.0, float('inf'))), ('inverted range', (1.0, -1.0))):
        outs[name] = metrics.wass_device(x, x, bins=16, range=r).cpu().numpy()
    print('\nvalue %r: ' % bad + '  '.join('%s -> wass %r status %d' % (k, float(o[0]), int(o[11])) for k, o in outs.items()))
    with pytest.raises(ValueError, match='not finite'):
        np.histogram_bin_edges(np.concatenate([a.ravel(), b.ravel()]), bins=16)
    for bins in (16, 'auto'):
        assert math.isnan(float(outs[bins][0])) and int(outs[bins][11]) == 1 and int(outs[bins][1]) == 0
        with pytest.raises(ValueError, match='not finite'):
            metrics.wass(x, y, bins=bins)
    assert int(outs['range to inf'][11]) == 2 and int(outs['inverted range'][11]) == 3
    with pytest.raises(ValueError, match='not finite'):
        metrics.wass(x, x, range=(0.0, float('inf')))
    with pytest.raises(ValueError, match='max must be larger'):
        metrics.wass(x, x, range=(1.0, -1.0))
    # inside an explicit range a non-finite value is dropped, as np.histogram drops it
    got, parts = metrics.wass(torch.from_numpy(a), torch.from_numpy(b), bins=12, range=(-1.0, 1.0), return_parts=True)
    want, wp = np_wass(a, b, 12, (-1.0, 1.0))
    check_counts_and_value('non-finite value outside the range', got, parts, want, wp)


@pytest.mark.parametrize('bins', [250, 'auto', 16385])
def test_same_bits_twice_and_under_graph_replay(bins):
    a, b = sets(28, 700, 640, 2)
    x, y = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    eager = metrics.wass_device(x, y, bins=bins, max_bins=1 << 15)            # also the warm-up
    again = metrics.wass_device(x, y, bins=bins, max_bins=1 << 15)
    host = metrics.wass_device(torch.from_numpy(a), y, bins=bins, max_bins=1 << 15)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = metrics.wass_device(x, y, bins=bins, max_bins=1 << 15)
    captured.zero_()
    g.replay()
    torch.cuda.synchronize()
    print('\nbins %r: %s' % (bins, eager.cpu().numpy()))
    assert eager.shape == (12,) and eager.dtype == torch.float64 and float(eager[11]) == 0 and float(eager[0]) > 0
    for other in (again, host, captured):
        assert torch.equal(eager.view(torch.int64), other.view(torch.int64))
    assert float(eager[0]) == metrics.wass(a, b, bins=bins)


def test_drop_in_leaves_the_last_sample_out():
    a, b = sets(29, 120, 120, 2)
    data, gen = torch.from_numpy(a).reshape(120, 1, 2), torch.from_numpy(b).reshape(120, 1, 2)
    got = metrics.compute_wasserstein_distance(data, gen)
    print('\ndrop-in %r  wass(gen[:-1], data[:-1]) %r  wass(gen, data) %r' % (got, metrics.wass(gen[:-1], data[:-1]), metrics.wass(gen, data)))
    assert got == metrics.wass(gen[:-1], data[:-1]) and got != metrics.wass(gen, data)
    assert metrics.compute_wasserstein_distance(data, gen, bins=40, _range=(-1.0, 1.0)) == metrics.wass(gen[:-1], data[:-1], bins=40,
                                                                                                     range=(-1.0, 1.0))
    assert metrics.compute_wasserstein_distance(data, gen, num_samples=50) == metrics.wass(gen[:50], data[:50])


# ---------------------------------------------------------------- end to end
def test_evaluate_wass_does_not_depend_on_the_chunking():
    net, N, real = toy(), 512, real_toy(512)
    values = []
    for bs in (200, 512):
        method, gm, ev = managers()
        values.append(ev.evaluate_wass({'default': net}, real, N, bs))
        assert ev.evals['wass'] == [values[-1]] and ev.evals['mmd'] == [] and method.calls == 1
    method, gm, ev = managers()
    auto = ev.evaluate_wass({'default': net}, real, 300, 200)                # below 512 samples: numpy's 'auto'
    print('\nevaluate_wass: %r %r  (300 samples, auto bins: %r)' % (values[0], values[1], auto))
    assert values[0] == values[1] and isinstance(values[0], float) and values[0] > 0 and auto > 0 and auto != values[0]


def test_evaluate_metrics_2d_is_the_three_figures_of_one_generation():
    net, N, real = toy(), 512, real_toy(512)
    method, gm, ev = managers()
    res = ev.evaluate_metrics_2d({'default': net}, real, N, 200)
    keys = {'wass', 'mmd', 'precision', 'recall', 'density', 'coverage', 'fid', 'f_1_pr', 'f_1_dc', 'fig'}
    assert set(res) == keys | {'samples'} and method.calls == 1
    samples = res['samples']
    assert samples.shape == (N, 1, 2) and all(ev.evals[k] == [res[k]] for k in keys)
    assert res['density'] == res['coverage'] == res['fid'] == res['f_1_dc'] == 0.0 and res['fig'] is None
    _, _, other = managers()
    mmd = other.evaluate_mmd({}, real, N, 200, samples=samples)
    prd = other.evaluate_prd({}, real, N, 200, samples=samples)
    want, wp = np_wass(samples.cpu().numpy()[:-1], real[:N].numpy()[:-1], 250)
    print('\nevaluate_metrics_2d: %s  mmd alone %r  prd alone %s  np_wass %.17g  |diff| %.3g  bound %.3g' % (
        {k: res[k] for k in sorted(keys)}, mmd, prd, want, abs(res['wass'] - want), value_bound(wp)))
    assert res['mmd'] == mmd and {k: res[k] for k in prd} == prd
    assert abs(res['wass'] - want) <= value_bound(wp)
    # and the same figures as the single-metric methods generating for themselves
    method, gm, ev = managers()
    assert ev.evaluate_wass({'default': net}, real, N, 512) == res['wass']


def test_cli_eval_wass_equals_the_api(tmp_path, capsys):
    from dlpm_amd import cli
    real = torch.randn(600, 1, 2, generator=torch.Generator().manual_seed(42)).numpy()
    path, out = str(tmp_path / 'real.npy'), str(tmp_path / 'gen.npy')
    np.save(path, real)
    base = ['--config', '2d_data', '--synthetic_weights', '1', '--set_seed', '3', '--reverse_steps', '10', '--generate', '512']
    got = cli.main(base + ['--eval_wass', path, '--batch_size', '200', '--out', out])
    printed = capsys.readouterr().out.strip().splitlines()[-1].split()
    samples = np.load(out)
    api = metrics.compute_wasserstein_distance(torch.from_numpy(real[:512]), torch.from_numpy(samples), bins=250)
    every = cli.main(base + ['--eval_wass', path, '--eval_mmd', path, '--eval_prd', path, '--batch_size', '512'])
    lines = capsys.readouterr().out.strip().splitlines()
    few = cli.main(base + ['--eval_wass', path, '--wass_bins', '40'])
    capsys.readouterr()
    api_few = metrics.compute_wasserstein_distance(torch.from_numpy(real[:512]), torch.from_numpy(samples), bins=40)
    with capsys.disabled():
        print('\ncli --eval_wass %r (printed %s)  api %r  with --eval_mmd --eval_prd %s  --wass_bins 40: %r  api %r' % (
            got, printed, api, every, few, api_few))
    assert printed[0] == 'wass' and printed[2:] == 'over 512 generated vs 512 real samples'.split()
    assert float(printed[1]) == pytest.approx(got, rel=1e-8) and math.isfinite(got)
    assert samples.shape == (512, 1, 2) and got == api
    assert [l.split()[0] for l in lines[-3:]] == ['mmd', 'prd', 'wass']
    assert every['wass'] == got and every['mmd'] == metrics.mmd(samples, real[:512]) and set(every) == {'wass', 'mmd', 'precision', 'recall',
                                                                                                        'f_1_pr'}
    assert few == api_few and few != got
    with pytest.raises(SystemExit):
        cli.main(base + ['--eval_wass', path, '--gen_data_path', str(tmp_path / 'png')])
