"""The exact W1 on the MI355X against the host mirror of tests/w1_refs.py: the permutation, the final prices, the round and phase
counts, the scale exponent and the integer cost are EQUAL to the mirror's bit for bit on every case of the table (every tile edge of
the cost kernels, every D-path, both grounds), W within the fp64 summation of the mirror's and inside the two-sided bound against the
optimum of tests/golden/f26_w1.npz; ties and degenerate sets; the same bits on a second call and under every tail_threshold; offset base
pointers; the round cap; non-finite input; and the Python, EvaluationManager and command-line layers."""
import math

import numpy as np
import pytest
import torch

import dlpm_amd
from dlpm_amd import metrics
from metric_helpers import managers
import w1_refs as R

pytestmark = pytest.mark.gpu


def device_call(x, y, ground, **kw):
    """(out [8], perm, prices) of metrics.w1_device as numpy arrays."""
    out, perm, prices = metrics.w1_device(torch.as_tensor(x), torch.as_tensor(y), ground, **kw)
    return out.cpu().numpy(), perm.cpu().numpy(), prices.cpu().numpy()


def assert_inside_the_bound(w, w_opt, m, n):
    """The two-sided bound against an exactly summed optimum.  Every cost of the assignment is within 2^-e / 2 of q 2^-e, so the
    exact mean of its costs lies in [W_opt, W_opt + 2^-e].  The device adds the n terms, each <= cmax, in fp64 in a fixed order:
    each of the n - 1 additions rounds a partial sum <= n cmax by at most 2^-53 relative, the division by n rounds once more, so
    |W - exact| <= (n - 1) 2^-53 cmax + 2^-53 cmax = n 2^-53 cmax.  Below: a feasible assignment is never under the optimum, only
    its rounded sum may be, by at most that.  Above: 2^-e + n 2^-52 cmax (w1_refs.w_bound), as for the mirror."""
    assert -n * 2.0 ** -53 * m['cmax'] <= w - w_opt <= R.w_bound(m['e'], n, m['cmax'])


def assert_equals_mirror(got, m, n):
    out, perm, prices = got
    assert int(out[6]) == 0
    assert (int(out[3]), int(out[4]), int(out[2])) == (m['rounds'], m['phases'], m['e'])
    assert out[5] == m['cmax']
    assert perm.dtype == np.int32 and (perm == m['perm']).all()
    assert prices.dtype == np.int64 and (prices == m['prices']).all()
    assert int(out[1]) == m['integer_cost']
    assert abs(out[0] - m['w']) <= n * 2.0 ** -52 * m['cmax']


@pytest.mark.parametrize('name,ground', R.PAIRS)
def test_table_case_equals_the_mirror_bit_for_bit(name, ground):
    m, f = R.mirror(name, ground), R.fixture()
    n = R.CASES[name][0]
    got = device_call(m['x'], m['y'], ground)
    print('\n%s %s: W %.17g mirror %.17g optimum %.17g  rounds %d (%d in the one-workgroup kernel) phases %d e %d' % (
        name, ground, got[0][0], m['w'], float(f['%s.%s.w_opt' % (name, ground)]), got[0][3], got[0][7], got[0][4], got[0][2]))
    assert_equals_mirror(got, m, n)
    assert int(got[0][1]) == int(f['%s.%s.q_opt' % (name, ground)])
    assert_inside_the_bound(got[0][0], float(f['%s.%s.w_opt' % (name, ground)]), m, n)


def clipped_cauchy(n, D, seed):
    g = np.random.default_rng(seed)
    return np.clip(g.standard_cauchy((n, D)), -50.0, 50.0).astype(np.float32)


def degenerate_sets():
    g = np.random.default_rng(77)
    lattice = np.array([[a, b] for a in range(4) for b in range(4)], np.float32)
    dup = g.standard_normal((24, 2)).astype(np.float32)
    dup[8:16] = dup[:8]                                  # duplicated rows in one set ...
    dup_y = g.standard_normal((24, 2)).astype(np.float32)
    dup_y[12:] = dup_y[:12]                              # ... and in the other
    return {'lattice': (lattice, (lattice[g.permutation(16)] + np.float32(1.0)).astype(np.float32)),
            'duplicates': (dup, dup_y),
            'cauchy_vs_gauss': (clipped_cauchy(96, 2, 78), g.standard_normal((96, 2)).astype(np.float32))}


@pytest.mark.parametrize('kind', ['lattice', 'duplicates', 'cauchy_vs_gauss'])
@pytest.mark.parametrize('ground', R.GROUNDS)
def test_ties_and_duplicates_equal_the_mirror(kind, ground):
    x, y = degenerate_sets()[kind]
    m = R.mirror_of(x, y, ground)
    n = len(x)
    assert m['rounds'] <= R.MAX_TABLE_ROUNDS
    got = device_call(x, y, ground)
    assert_equals_mirror(got, m, n)
    terms, _ = R.scipy_optimum(m['c'])
    assert int(got[0][1]) == int(R.scipy_optimum(m['q'])[0].sum())
    assert_inside_the_bound(got[0][0], math.fsum(terms.tolist()) / n, m, n)


@pytest.mark.parametrize('ground', R.GROUNDS)
def test_all_points_equal(ground):
    n = 33
    x = np.full((n, 3), 0.75, np.float32)
    out, perm, prices = device_call(x, x, ground)
    assert (out[0], out[1], out[2], out[3], out[4], out[5], out[6]) == (0.0, 0.0, 0.0, float(n), 1.0, 0.0, 0.0)
    assert sorted(perm.tolist()) == list(range(n))
    assert_equals_mirror((out, perm, prices), R.mirror_of(x, x, ground), n)


@pytest.mark.parametrize('ground', R.GROUNDS)
def test_permuted_copy_gives_zero_and_the_inverse_permutation(ground):
    g = np.random.default_rng(3)
    n = 100
    x = g.standard_normal((n, 2)).astype(np.float32)
    assert len(np.unique(x, axis=0)) == n
    s = g.permutation(n)
    y = x[s].copy()                                      # y[k] = x[s[k]]: row i of x sits at row inverse(s)[i] of y
    value, parts = metrics.w1(x, y, ground=ground, return_parts=True)
    assert value == 0.0 and parts['integer_cost'] == 0
    assert (parts['perm'] == np.argsort(s)).all()


def test_same_bits_on_a_second_call_and_under_every_tail_threshold():
    name, ground = 'n65_d3', 'l1_mean'
    m = R.mirror(name, ground)
    n = 65
    first = device_call(m['x'], m['y'], ground)
    runs = {'again': device_call(m['x'], m['y'], ground), 'never': device_call(m['x'], m['y'], ground, tail_threshold=0),
            'always': device_call(m['x'], m['y'], ground, tail_threshold=n), 'four': device_call(m['x'], m['y'], ground, tail_threshold=4)}
    assert_equals_mirror(first, m, n)
    for key, got in runs.items():
        assert got[0][:7].tobytes() == first[0][:7].tobytes(), key
        assert (got[1] == first[1]).all() and (got[2] == first[2]).all(), key
    assert runs['never'][0][7] == 0 and runs['always'][0][7] == first[0][3] and 0 < runs['four'][0][7] < first[0][3]
    assert first[0][7] == runs['again'][0][7]


@pytest.mark.parametrize('name', ['n17_d3', 'n65_d17'])
def test_base_pointers_offset_by_one_float(name):
    m = R.mirror(name, 'euclidean')
    n, D, _ = R.CASES[name]
    bx, by = torch.zeros(n * D + 1, device='cuda'), torch.zeros(n * D + 1, device='cuda')
    bx[1:] = torch.from_numpy(m['x']).reshape(-1).cuda()
    by[1:] = torch.from_numpy(m['y']).reshape(-1).cuda()
    x, y = bx[1:].view(n, D), by[1:].view(n, D)
    assert x.data_ptr() % 8 == 4 and x.is_contiguous()
    out, perm, prices = metrics.w1_device(x, y, 'euclidean')
    assert_equals_mirror((out.cpu().numpy(), perm.cpu().numpy(), prices.cpu().numpy()), m, n)


def test_round_cap_is_status_2_and_the_next_call_is_correct(monkeypatch):
    m = R.mirror('n64_d2', 'l1_mean')
    assert m['rounds'] > 1
    out, perm, prices = device_call(m['x'], m['y'], 'l1_mean', max_rounds=1)
    assert int(out[6]) == 2 and math.isnan(out[0]) and int(out[3]) == 1
    exact = device_call(m['x'], m['y'], 'l1_mean', max_rounds=m['rounds'])          # exactly enough rounds is not the cap
    assert_equals_mirror(exact, m, 64)
    short = device_call(m['x'], m['y'], 'l1_mean', max_rounds=m['rounds'] - 1)
    assert int(short[0][6]) == 2 and math.isnan(short[0][0])
    monkeypatch.setattr(metrics, 'w1_default_max_rounds', lambda n: 1)
    with pytest.raises(RuntimeError, match='max_rounds = 1'):
        metrics.w1(m['x'], m['y'])
    monkeypatch.undo()
    assert metrics.w1(m['x'], m['y']) == exact[0][0]                               # the caching allocator hands the same workspace back


def test_non_finite_input_is_status_1():
    m = R.mirror('n17_d2', 'l1_mean')
    for which, bad in ((0, np.nan), (1, np.inf), (1, np.nan)):
        x, y = m['x'].copy(), m['y'].copy()
        (x, y)[which][5, 1] = bad
        out, _, _ = device_call(x, y, 'l1_mean')
        assert int(out[6]) == 1 and math.isnan(out[0])
        with pytest.raises(ValueError, match='non-finite'):
            metrics.w1(x, y)
    assert_equals_mirror(device_call(m['x'], m['y'], 'l1_mean'), m, 17)


def test_return_parts_and_host_or_device_inputs():
    m = R.mirror('n63_d16', 'euclidean')
    value, parts = metrics.w1(m['x'], m['y'], ground='euclidean', return_parts=True)
    assert set(parts) == {'perm', 'prices', 'rounds', 'phases', 'scale_exponent', 'cmax', 'integer_cost'}
    assert (parts['rounds'], parts['phases'], parts['scale_exponent'], parts['cmax'], parts['integer_cost']) == (
        m['rounds'], m['phases'], m['e'], m['cmax'], m['integer_cost'])
    assert (parts['perm'] == m['perm']).all() and (parts['prices'] == m['prices']).all()
    assert metrics.w1(torch.from_numpy(m['x']).cuda(), torch.from_numpy(m['y']), ground='euclidean') == value
    assert metrics.w1(m['x'].reshape(63, 4, 4), m['y'].reshape(63, 2, 8), ground='euclidean') == value      # rows are flattened


def test_compute_w1_distance_cuts_both_sets():
    m = R.mirror('n65_d2', 'l1_mean')
    x, y = m['x'], m['y']
    assert metrics.compute_w1_distance(x, y) == metrics.w1(x, y)
    assert metrics.compute_w1_distance(x, y[:40]) == metrics.w1(x[:40], y[:40]) == metrics.compute_w1_distance(x, y, num_samples=40)
    assert metrics.compute_w1_distance(x[:17], y) == metrics.w1(x[:17], y[:17])
    want = R.mirror_of(x[:40], y[:40], 'l1_mean')['w']
    assert abs(metrics.compute_w1_distance(x, y, num_samples=40) - want) <= 40 * 2.0 ** -52 * m['cmax']


def test_evaluate_w1_with_given_samples_fills_its_key():
    m = R.mirror('n64_d2', 'l1_mean')
    _, _, ev = managers()
    assert 'w1' not in ev.evals
    real, samples = m['x'].reshape(64, 1, 2), m['y'].reshape(64, 1, 2)
    value = ev.evaluate_w1({}, real, 64, 16, samples=samples)
    assert isinstance(value, float) and value == metrics.w1(m['x'], m['y']) and ev.evals['w1'] == [value]
    other = ev.evaluate_w1({}, real, 64, 16, ground='euclidean', samples=samples)
    assert ev.evals['w1'] == [value, other] and other == metrics.w1(m['x'], m['y'], ground='euclidean') and other > value
    assert ev.evals['wass'] == [] and ev.evals['mmd'] == []
    ev.reset(keep_evals=True)
    assert ev.evals['w1'] == [value, other]
    ev.reset()
    assert 'w1' not in ev.evals


def test_cli_eval_w1_writes_a_finite_figure(tmp_path, capsys):
    from dlpm_amd import cli
    real = torch.randn(80, 1, 2, generator=torch.Generator().manual_seed(42)).numpy()
    path, out = str(tmp_path / 'real.npy'), str(tmp_path / 'gen.npy')
    np.save(path, real)
    base = ['--config', '2d_data', '--synthetic_weights', '1', '--set_seed', '3', '--reverse_steps', '10', '--generate', '64',
            '--batch_size', '64']
    got = cli.main(base + ['--eval_w1', path, '--out', out])
    printed = capsys.readouterr().out.strip().splitlines()[-1].split()
    samples = np.load(out)
    assert printed[0] == 'w1' and printed[2:] == 'ground l1_mean over 64 generated vs 64 real samples'.split()
    assert math.isfinite(got) and got > 0 and float(printed[1]) == pytest.approx(got, rel=1e-8)
    assert got == metrics.compute_w1_distance(torch.from_numpy(real[:64]), torch.from_numpy(samples))
    eu = cli.main(base + ['--eval_w1', path, '--w1_ground', 'euclidean'])
    assert math.isfinite(eu) and eu == metrics.w1(real[:64], samples, ground='euclidean')
    own = cli.main(base + ['--eval_w1', 'dataset'])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert math.isfinite(own) and own > 0 and line.startswith('w1 ')
