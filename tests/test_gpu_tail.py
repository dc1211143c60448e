"""The tail figures on the MI355X against the host mirror of tests/tail_refs.py: k, both thresholds and every quantile are EQUAL to
the mirror's bit for bit (the quantiles are two rounded fp64 operations on the two order statistics they interpolate, so equal
quantiles at many levels are equal order statistics; at N = 2 K + 1, xi = 0.5 and K a power of two they ARE the order statistics),
msle and the Hill indices inside the derived bound of tail_refs; ties at a clamp, constant sets, sets that span many workgroups, every
D, K and xi; the statuses; the same bits on a second call, with the sets swapped and under graph replay; and the Python,
EvaluationManager and command-line layers.  Every test prints the figures it measured before it asserts."""
import functools
import math

import numpy as np
import pytest
import torch

import dlpm_amd
from dlpm_amd import metrics
from metric_helpers import managers, real_toy, toy
import tail_refs as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def device_call(x, y, xi, K, marginal):
    """(out [8], quantiles [2, K]) of dlpm_tail_f32 as numpy arrays."""
    out, q = metrics._tail_run(torch.as_tensor(x), torch.as_tensor(y), xi, K, marginal, True)
    return out.cpu().numpy(), q.cpu().numpy()


def heavy(seed, n, D):
    g = np.random.default_rng(seed)
    return (g.standard_t(1.5, (n, D)) * 0.7).astype(np.float32)


def assert_equals_mirror(got, m, label=''):
    out, q = got
    print('\n%s device msle %.17g hill %.17g %.17g k %d %d thresholds %.9g %.9g status %d | mirror msle %.17g hill %.17g %.17g' % (
        label, out[0], out[1], out[2], out[3], out[5], out[4], out[6], out[7], m['msle'], m['hill'][0], m['hill'][1]))
    assert int(out[7]) == m['status']
    assert [int(out[3]), int(out[5])] == m['k'] and out[3] == m['k'][0] and out[5] == m['k'][1]
    if m['status'] == 1:
        assert np.isnan(out[[0, 1, 2, 4, 6]]).all() and np.isnan(q).all()
        return
    for which in (0, 1):
        assert np.float64(out[4 + 2 * which]).tobytes() == np.float64(m['threshold'][which]).tobytes()
    assert q.dtype == np.float64 and q.tobytes() == m['quantiles'].tobytes()
    if math.isnan(m['msle']):
        assert math.isnan(out[0])
    else:
        err, bound = abs(out[0] - m['msle']), R.msle_bound(m)
        print('  msle error %.3g bound %.3g' % (err, bound))
        assert err <= bound
    for which in (0, 1):
        h = m['hill'][which]
        if math.isnan(h) or math.isinf(h):
            assert (math.isnan(out[1 + which]) and math.isnan(h)) or out[1 + which] == h
        else:
            rel, bound = abs(out[1 + which] - h) / h, R.hill_rel_bound(m, which)
            print('  hill %d relative error %.3g bound %.3g' % (which, rel, bound))
            assert rel <= bound


@functools.lru_cache(maxsize=None)
def sets(name):
    if name == 'two_three':
        return heavy(1, 2, 2), heavy(2, 3, 2)
    if name == '257_255':
        return heavy(3, 257, 2), heavy(4, 255, 2)
    if name == 'clamped':
        x, y = heavy(5, 1000, 2), np.clip(heavy(6, 777, 2), -6.0, 6.0)
        y[100:130] = 6.0                                    # 30 rows exactly on the clamp: ties at the top of both marginals
        return x, y
    if name == 'many_workgroups':
        return heavy(7, 100003, 2), heavy(8, 65537, 2)
    if name.startswith('d'):
        D = int(name[1:])
        return heavy(9 + D, 513, D), heavy(40 + D, 513, D)
    raise KeyError(name)


CASES = [('two_three', 0.5, 1), ('257_255', 0.95, 100), ('257_255', 0.5, 255), ('clamped', 0.95, 100), ('clamped', 0.97, 777),
         ('many_workgroups', 0.95, 100), ('many_workgroups', 0.5, 4096),
         ('d1', 0.5, 256), ('d2', 0.5, 256), ('d3', 0.5, 256), ('d17', 0.5, 256), ('d3', 0.95, 513),
         ('d2', 0.95, 1), ('d2', 0.95, 4096), ('d2', 0.999, 100), ('d17', 0.999, 4096)]


@pytest.mark.parametrize('marginal', R.MARGINALS)
@pytest.mark.parametrize('name,xi,K', CASES)
def test_case_equals_the_mirror(name, xi, K, marginal):
    x, y = sets(name)
    m = R.mirror(x, y, xi, K, marginal)
    assert m['status'] == 0
    assert_equals_mirror(device_call(x, y, xi, K, marginal), m, '%s xi %g K %d %s:' % (name, xi, K, marginal))


@pytest.mark.parametrize('D', [1, 2, 3, 17])
def test_quantiles_at_integer_ranks_are_the_order_statistics(D):
    """N = 513 = 2 K + 1 at xi = 0.5, K = 256: u_j (N - 1) = 256 + j exactly, so quantile j IS s[256 + j]."""
    x, y = sets('d%d' % D)
    _, q = device_call(x, y, 0.5, 256, 'norm')
    for which, a in enumerate((x, y)):
        s = np.sort(R.marginal_values(a, 'norm'))
        assert q[which].tobytes() == s[256:512].astype(np.float64).tobytes()
    if D == 1:
        _, qa = device_call(x, y, 0.5, 256, 'abs')
        assert qa.tobytes() == q.tobytes()


def test_ties_at_the_clamp_reach_the_top():
    """The 30 clamped rows of the second set are its 30 largest norms: the top quantiles sit on the clamp's norm and are equal."""
    x, y = sets('clamped')
    out, q = device_call(x, y, 0.97, 777, 'norm')
    top = np.float64(np.float32(math.sqrt(72.0)))
    # r0 = floor(0.97 * 776) = 752 lies inside the 30 tied ranks 747 .. 776: the tail is wholly on the clamp, the index +inf
    assert (q[1][-5:] == top).all() and out[7] == 0 and out[2] == math.inf and out[6] == top
    out, _ = device_call(x, y, 0.95, 100, 'norm')            # r0 = 737 lies below the ties: a finite index
    assert out[7] == 0 and math.isfinite(out[2]) and out[6] < top
    out, _ = device_call(x, y[100:130], 0.5, 4, 'norm')      # a set that is nothing but the clamp
    assert out[2] == math.inf and out[6] == top and out[7] == 0


def test_constant_sets():
    a, b = np.full((9, 3), 0.25, np.float32), np.full((5, 3), 0.25, np.float32)
    for marginal in R.MARGINALS:
        got = device_call(a, b, 0.5, 3, marginal)
        assert got[0][0] == 0.0 and got[0][1] == math.inf and got[0][2] == math.inf and got[0][7] == 0
        assert_equals_mirror(got, R.mirror(a, b, 0.5, 3, marginal), 'constant %s:' % marginal)


def test_heavy_tailed_device_draws():
    """Two independent draws of the package's own alpha-stable grid: exact against the mirror, and the figures tell them from a
    Gaussian cloud of the same scale."""
    kw = dict(alpha=1.5, n=3, std=0.1, isotropic=True)
    x = dlpm_amd.datasets.sample_grid_sas(20000, seed=1, **kw).cpu().numpy()
    y = dlpm_amd.datasets.sample_grid_sas(20000, seed=2, **kw).cpu().numpy()
    m = R.mirror(x, y, 0.95, 100, 'norm')
    got = device_call(x, y, 0.95, 100, 'norm')
    assert_equals_mirror(got, m, 'sas alpha 1.5:')
    gauss = np.random.default_rng(3).standard_normal((20000, 2)).astype(np.float32)
    far = device_call(x, gauss, 0.95, 100, 'norm')[0]
    print('  msle between two draws %.4g, against a Gaussian cloud %.4g; Hill %.3f %.3f, Gaussian %.3f' % (
        got[0][0], far[0], got[0][1], got[0][2], far[2]))
    # qualitative only: a Gaussian norm has a Rayleigh tail, whose Hill estimate at the 95 % point is near 2 ln 20 = 6, far above any
    # alpha < 2; two draws of one law differ by sampling noise, a heavy and a light tail by the growth of the quantiles themselves
    assert got[0][1] < far[2] and got[0][2] < far[2]
    assert got[0][0] < far[0]


@pytest.mark.parametrize('bad', [math.nan, math.inf, -math.inf])
def test_non_finite_input_is_status_1(bad):
    x, y = (a.copy() for a in sets('257_255'))
    for which in (0, 1):
        a, b = x.copy(), y.copy()
        (a, b)[which][200, 1] = bad
        for marginal in R.MARGINALS:
            got = device_call(a, b, 0.95, 10, marginal)
            assert_equals_mirror(got, R.mirror(a, b, 0.95, 10, marginal))
            assert got[0][7] == 1
            with pytest.raises(ValueError, match='non-finite'):
                metrics.tail(a, b, marginal=marginal)
    assert_equals_mirror(device_call(x, y, 0.95, 10, 'norm'), R.mirror(x, y, 0.95, 10, 'norm'))       # and the next call is fine


def test_zero_up_to_the_96th_percentile_is_status_2():
    x = np.abs(heavy(11, 400, 2)) + np.float32(0.01)
    z = x.copy()
    flat = z.reshape(-1)
    flat[:int(0.97 * flat.size)] = 0.0
    m = R.mirror(x, z, 0.95, 50, 'abs')
    got = device_call(x, z, 0.95, 50, 'abs')
    assert_equals_mirror(got, m, 'zeros:')
    assert got[0][7] == 2 and math.isnan(got[0][0]) and math.isnan(got[0][2]) and math.isfinite(got[0][1]) and got[0][6] == 0.0
    res = metrics.tail(x, z, marginal='abs', levels=50)                                # NaN, not an exception
    assert math.isnan(res['msle']) and math.isnan(res['tail_index_second']) and res['tail_index_first'] == got[0][1]
    # zeros below the threshold only: the quantiles at the first levels are positive, every figure is given
    z2 = x.copy()
    z2.reshape(-1)[:int(0.5 * flat.size)] = 0.0
    got2 = device_call(x, z2, 0.95, 50, 'abs')
    assert_equals_mirror(got2, R.mirror(x, z2, 0.95, 50, 'abs'))
    assert got2[0][7] == 0


def test_same_bits_twice_swapped_and_under_graph_replay():
    a, b = sets('clamped')
    x, y = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    for marginal in R.MARGINALS:
        first = metrics._tail_run(x, y, 0.95, 100, marginal, True)                     # also the warm-up
        again = metrics._tail_run(x, y, 0.95, 100, marginal, True)
        host = metrics._tail_run(torch.from_numpy(a), y, 0.95, 100, marginal, True)
        swapped = metrics._tail_run(y, x, 0.95, 100, marginal, True)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            captured = metrics._tail_run(x, y, 0.95, 100, marginal, True)
        captured[0].zero_()
        captured[1].zero_()
        g.replay()
        torch.cuda.synchronize()
        o = first[0].cpu().numpy()
        print('\n%s: %s' % (marginal, o))
        assert o[7] == 0 and o[0] > 0
        for other in (again, host, captured):
            assert torch.equal(first[0].view(torch.int64), other[0].view(torch.int64))
            assert torch.equal(first[1].view(torch.int64), other[1].view(torch.int64))
        s = swapped[0].cpu().numpy()
        assert s[[0, 2, 1, 5, 6, 3, 4, 7]].tobytes() == o.tobytes()
        assert torch.equal(swapped[1].flip(0).contiguous().view(torch.int64), first[1].view(torch.int64))
        assert torch.equal(metrics.tail_device(x, y, 0.95, 100, marginal).view(torch.int64), first[0].view(torch.int64))


def test_python_layer():
    a, b = sets('257_255')
    out, q = device_call(a, b, 0.9, 20, 'norm')
    res = metrics.tail(a, b, xi=0.9, levels=20, return_parts=True)
    assert set(res) == {'msle', 'tail_index_first', 'tail_index_second', 'k', 'thresholds', 'quantiles'}
    assert (res['msle'], res['tail_index_first'], res['tail_index_second']) == (out[0], out[1], out[2])
    assert res['k'] == (int(out[3]), int(out[5])) and res['thresholds'] == (out[4], out[6]) and (res['quantiles'] == q).all()
    assert set(metrics.tail(a, b, xi=0.9, levels=20)) == {'msle', 'tail_index_first', 'tail_index_second'}
    assert metrics.msle(a, b, xi=0.9, levels=20) == out[0]
    assert metrics.hill_index(a, xi=0.9) == out[1] and metrics.hill_index(torch.from_numpy(b).to(DEV), xi=0.9) == out[2]
    assert metrics.tail(a.reshape(257, 1, 2), torch.from_numpy(b).to(DEV), xi=0.9, levels=20)['msle'] == out[0]     # rows are flattened
    assert metrics.hill_index(a, xi=0.9, marginal='abs') == device_call(a, a, 0.9, 1, 'abs')[0][1]


def test_evaluate_tail_does_not_depend_on_the_chunking():
    net, N = toy(), 1000
    real = real_toy(N)
    results = []
    for bs in (256, 1000):
        method, gm, ev = managers()
        assert not {'msle', 'tail_index_real', 'tail_index_gen'} & set(ev.evals)
        res = ev.evaluate_tail({'default': net}, real, N, bs, xi=0.9)
        assert set(res) == {'msle', 'tail_index_real', 'tail_index_gen'} and method.calls == 1
        assert all(ev.evals[k] == [res[k]] for k in res)
        results.append(res)
    method, gm, ev = managers()
    with method.dataset_stream():
        samples = gm.generate({'default': net}, N, to_host=False, declare_batch=False)
    given = ev.evaluate_tail({}, real, N, 7, xi=0.9, samples=samples)
    direct = metrics.tail(real[:N], samples, xi=0.9)
    print('\nevaluate_tail %s  from samples= %s' % (results, given))
    assert results[0] == results[1] == given and method.calls == 1
    assert given == {'msle': direct['msle'], 'tail_index_real': direct['tail_index_first'], 'tail_index_gen': direct['tail_index_second']}
    assert math.isfinite(given['msle']) and all(v > 0 for v in given.values())       # an index may be +inf: the samples are clamped
    again = ev.evaluate_tail({}, real, N, 7, xi=0.9, marginal='abs', samples=samples)
    assert ev.evals['msle'] == [given['msle'], again['msle']] and again != given
    assert ev.evals['wass'] == [] and ev.evals['mmd'] == []


def test_cli_eval_tail(tmp_path, capsys, monkeypatch):
    from dlpm_amd import cli
    base = ['--config', '2d_data', '--synthetic_weights', '1', '--set_seed', '3', '--reverse_steps', '10', '--generate', '512',
            '--batch_size', '512']
    out = str(tmp_path / 'gen.npy')
    got = cli.main(base + ['--eval_tail', 'dataset', '--out', out])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    words = line.split()
    print('\n' + line)
    assert words[:2] == ['tail', 'msle'] and words[3:5] == ['index', 'real'] and words[6] == 'generated' and words[8] == 'xi'
    assert words[9:] == '0.95 over 512 generated vs 512 real samples'.split()
    assert set(got) == {'msle', 'tail_index_real', 'tail_index_gen'}
    assert [float(words[2]), float(words[5]), float(words[7])] == pytest.approx([got['msle'], got['tail_index_real'], got['tail_index_gen']],
                                                                                rel=1e-8)
    samples = np.load(out)
    real = str(tmp_path / 'real.npy')
    np.save(real, real_toy(512).numpy())
    from_file = cli.main(base + ['--eval_tail', real, '--tail_xi', '0.9', '--tail_levels', '50', '--tail_marginal', 'abs'])
    assert capsys.readouterr().out.strip().splitlines()[-1].split()[8:10] == ['xi', '0.9']
    want = metrics.tail(real_toy(512)[:512], samples, xi=0.9, levels=50, marginal='abs')
    assert from_file == {'msle': want['msle'], 'tail_index_real': want['tail_index_first'], 'tail_index_gen': want['tail_index_second']}
    calls = []
    generate = dlpm_amd.EvaluationManager._generate_flat
    monkeypatch.setattr(dlpm_amd.EvaluationManager, '_generate_flat', lambda self, *a: calls.append(1) or generate(self, *a))
    both = cli.main(base + ['--eval_tail', 'dataset', '--eval_w1', 'dataset'])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(calls) == 1 and [l.split()[0] for l in lines[-2:]] == ['w1', 'tail']
    assert both['tail'] == got and math.isfinite(both['w1']) and set(both) == {'w1', 'tail'}
