"""Device Frechet distance on the MI355X against the oracle `np_fd` (tests/test_fd_cpu.py) inside the error model `bound_of`, on the
fixture family f21 and around the tile edges; the statistics against np.mean / np.cov; the closed forms (Hadamard, fake = real,
y = x + c); permutations, repeated calls, a NaN in the input; the reference-named functions; and the ways in (EvaluationManager with
samples, generated samples, a features callable, precomputed statistics, the command line).  Every test prints the measured error
beside its bound."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dlpm_amd import _lib, metrics
from metric_helpers import managers, real_toy, toy
from test_fd_cpu import ALL_NAMES, EPS, HAD_A, HAD_B, HAD_C, HAD_NAME, bound_of, fixture, np_fd, np_stats, ref_fd

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model_of(x, y):
    """(oracle dict, bound) of a pair of sets that is no fixture case: the reference recipe's own distance from the oracle enters the
    bound where the recipe gives a finite real number (on a singular product it may not; the floor and the null term then stand alone,
    which asks more, not less)."""
    o = np_fd(x, y)
    try:
        ref_dev = abs(ref_fd(x, y) - o['fd'])
    except Exception:
        ref_dev = 0.0
    if not math.isfinite(ref_dev):
        ref_dev = 0.0
    F = int(np.prod(np.shape(x)[1:]))
    return o, bound_of(F, ref_dev, o['tr1'] + o['tr2'], o['z'], o['tr1'], o['tr2'])


def check_stats(tag, x, mu, sigma):
    """mu, sigma (device tensors) against np.mean / np.cov in fp64: an n-term fp64 sum of products bounded by max |x - mu|^2 per entry
    (for mu, the smaller of that and its first power, the n-term sum of the values themselves)."""
    n = len(x)
    want_mu, want_sigma = np_stats(x)
    x64 = np.asarray(x, np.float64).reshape(n, -1)
    m = np.abs(x64 - want_mu).max()
    tol = 4 * (n + 8) * EPS * m * m
    tol_mu = 4 * (n + 8) * EPS * min(m * m, np.abs(x64).max()) if m > 0 else 0.0
    err_mu = np.abs(mu.cpu().numpy() - want_mu).max()
    err_sigma = np.abs(sigma.cpu().numpy() - want_sigma).max()
    print('%s: mu error %.3g (%.3g)  sigma error %.3g (%.3g)' % (tag, err_mu, tol_mu, err_sigma, tol))
    assert mu.dtype == torch.float64 and sigma.dtype == torch.float64 and mu.is_cuda and sigma.is_cuda
    assert tuple(sigma.shape) == (x64.shape[1],) * 2 and torch.equal(sigma, sigma.T.contiguous())      # exactly symmetric
    assert err_mu <= tol_mu and err_sigma <= tol


def check_against(tag, x, y, want, bound, oracle=None):
    value, parts = metrics.fd(x, y, return_parts=True)
    err = abs(value - want)
    print('\n%s: fd %.17g  want %.17g  error %.3g  bound %.3g  sweeps %s' % (tag, value, want, err, bound, parts['sweeps']))
    assert isinstance(value, float) and err <= bound
    assert 1 <= parts['sweeps'][0] <= 60 and 1 <= parts['sweeps'][1] <= 60
    if oracle is not None:
        for key, name in (('mean_term', 'mean_term'), ('tr1', 'tr_sigma1'), ('tr2', 'tr_sigma2'), ('tr_sqrt', 'tr_sqrt')):
            assert abs(parts[name] - oracle[key]) <= bound, key
    return value, parts


# ---------------------------------------------------------------- 1, 2: the fixture family
@pytest.mark.parametrize('name', ALL_NAMES)
def test_fixture_case_within_the_error_model_and_statistics_within_fp64(name):
    f = fixture(name)
    value, parts = check_against(name, f['real'], f['fake'], f['fd'], f['bound'], oracle=f)
    check_stats(name + ' real', f['real'], parts['mu1'], parts['sigma1'])
    check_stats(name + ' fake', f['fake'], parts['mu2'], parts['sigma2'])
    assert (parts['n1'], parts['n2']) == (f['n1'], f['n2'])


def test_hadamard_closed_form_and_an_already_diagonal_matrix_takes_no_rotation():
    f = fixture(HAD_NAME)
    F = f['F']
    want = F * (64 / 63) * (HAD_A - HAD_B) ** 2 + F * HAD_C ** 2
    value, parts = check_against('hadamard closed form', f['real'], f['fake'], want, f['bound'])
    assert parts['sweeps'][0] <= 2
    assert torch.equal(parts['sigma1'], torch.eye(F, dtype=torch.float64, device=DEV) * (HAD_A ** 2 * 64 / 63))
    assert abs(parts['mean_term'] - F * HAD_C ** 2) <= f['bound']


# ---------------------------------------------------------------- 3: sizes around the edges
@pytest.fixture(scope='module')
def edge_pool():
    rs = np.random.RandomState(77)
    s = 0.5 + np.arange(65) / 65
    x = (rs.standard_normal((130, 65)) * s).astype(np.float32)
    y = (rs.standard_normal((130, 65)) * 1.2 * s + 0.1).astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@pytest.mark.parametrize('n,F', [(130, F) for F in (15, 16, 17, 63, 64, 65)] + [(n, 17) for n in (2, 3, 127, 128, 129)])
def test_sizes_around_the_edges(edge_pool, n, F):
    x, y = (np.ascontiguousarray(a[:n, :F]) for a in edge_pool)
    o, bound = model_of(x, y)
    value, parts = check_against('edge n = %d, F = %d (z = %d)' % (n, F, o['z']), x, y, o['fd'], bound, oracle=o)
    check_stats('edge real', x, parts['mu1'], parts['sigma1'])


@pytest.mark.parametrize('F', [20, 130])
def test_a_covariance_cut_into_two_row_chunks(F):
    """n1 = 600 and n2 = 520 rows are cut into 304 + 296 and 272 + 248 (the chunk rule: no chunk under 256 rows, a multiple of 16 per
    chunk), so every tile adds two partials, each with a ragged last chunk and a ragged last K step; F = 130 has three triangle
    tiles, so the partials are indexed by chunk x tile."""
    rs = np.random.RandomState(600 + F)
    s = 0.5 + np.arange(F) / F
    x = (rs.standard_normal((600, F)) * s).astype(np.float32)
    y = (rs.standard_normal((520, F)) * 1.2 * s + 0.1).astype(np.float32)
    o, bound = model_of(x, y)
    value, parts = check_against('two chunks, F = %d' % F, x, y, o['fd'], bound, oracle=o)
    check_stats('two chunks real', x, parts['mu1'], parts['sigma1'])
    check_stats('two chunks fake', y, parts['mu2'], parts['sigma2'])


# ---------------------------------------------------------------- 4, 5: closed forms
def test_fake_equal_to_real_is_zero_within_the_bound_and_not_clamped():
    x = fixture('gauss300x260x64')['real']
    o, bound = model_of(x, x)
    value, parts = check_against('fake = real', x, x, 0.0, bound)
    assert abs(o['fd']) <= bound                                  # the oracle itself: the reference, too, may go slightly negative
    assert torch.equal(parts['sigma1'], parts['sigma2']) and parts['mean_term'] == 0.0


@pytest.mark.parametrize('n,F', [(150, 12), (260, 70)])
def test_a_shift_adds_its_squared_length(n, F):
    """x on a 2^-10 grid, so that x + c is exact in float32: the covariances are equal in exact arithmetic and fd = F c^2."""
    rs = np.random.RandomState(5 + F)
    x = (np.round(rs.standard_normal((n, F)) * 1024) / 1024).astype(np.float32)
    c = 0.25
    y = x + np.float32(c)
    assert np.array_equal(y.astype(np.float64), x.astype(np.float64) + c)
    _, bound = model_of(x, y)
    check_against('y = x + %g' % c, x, y, c * c * F, bound)


# ---------------------------------------------------------------- 6, 7: permutations, repeated calls
def test_row_permutations_stay_within_the_bound():
    """Not bit-identical: the column sums and the rank-n update add the rows in index order."""
    f = fixture('gauss300x260x64')
    rs = np.random.RandomState(7)
    pr, pf = rs.permutation(f['n1']), rs.permutation(f['n2'])
    for tag, real, fake in (('fake permuted', f['real'], f['fake'][pf]), ('real permuted', f['real'][pr], f['fake'])):
        check_against(tag, np.ascontiguousarray(real), np.ascontiguousarray(fake), f['fd'], f['bound'])


@pytest.mark.parametrize('name', ['gauss129x131x17', 'gauss300x260x129', 'gauss40x50x64'])
def test_two_calls_give_the_same_bits(name):
    f = fixture(name)
    x, y = torch.from_numpy(f['real']).to(DEV), torch.from_numpy(f['fake']).to(DEV)
    a, b = metrics.fd_device(x, y), metrics.fd_device(x, y)
    assert a.dtype == torch.float64 and a.shape == (8,) and float(a[5]) == 0
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    va, pa = metrics.fd(x, y, return_parts=True)
    vb, pb = metrics.fd(x, y, return_parts=True)
    assert va == vb == float(a[0]) and pa['sweeps'] == pb['sweeps'] == (int(a[6]), int(a[7]))
    for key in ('mu1', 'sigma1', 'mu2', 'sigma2'):
        assert torch.equal(pa[key].view(torch.int64), pb[key].view(torch.int64))


# ---------------------------------------------------------------- 8: a NaN in the input
def test_nan_raises_value_error_and_leaves_evals_untouched():
    f = fixture('gauss129x131x17')
    fake = f['fake'].copy()
    fake[17, 1] = float('nan')
    o = metrics.fd_device(f['real'], fake).cpu().numpy()
    print('\nNaN in fake[17, 1]: out %s' % o)
    assert int(o[5]) == 1 and all(math.isnan(v) for v in o[:5])
    for kw in ({}, {'return_parts': True}):
        with pytest.raises(ValueError, match='non-finite'):
            metrics.fd(f['real'], fake, **kw)
    with pytest.raises(ValueError, match='non-finite'):
        metrics.feature_statistics(fake)
    real = f['real'].copy()
    real[3, 0] = float('inf')
    assert int(metrics.fd_device(real, f['fake'])[5]) == 1
    s = np.eye(3)
    s[1, 1] = float('nan')
    with pytest.raises(ValueError, match='non-finite'):
        metrics.calculate_frechet_distance(np.zeros(3), s, np.zeros(3), np.eye(3))
    _, _, ev = managers()
    with pytest.raises(ValueError, match='non-finite'):
        ev.evaluate_fid({}, f['real'][:100], 100, 64, samples=fake[:100])
    assert ev.evals['fid'] == []
    assert abs(metrics.fd(f['real'], f['fake']) - f['fd']) <= f['bound']            # the process goes on, and a clean call is correct


# ---------------------------------------------------------------- 9, 10: the reference's names
def test_frechet_distance_of_device_statistics_equals_fd_bit_for_bit():
    for name in ('gauss129x131x17', 'gauss300x260x129'):
        f = fixture(name)
        a, b = torch.from_numpy(f['real']).to(DEV), f['fake']
        assert metrics.calculate_frechet_distance(*metrics.feature_statistics(a), *metrics.feature_statistics(b)) == metrics.fd(a, b)
        assert metrics.calculate_frechet_distance(*metrics.feature_statistics(a), *metrics.feature_statistics(b), eps=1e-3) == metrics.fd(a, b)


@pytest.mark.parametrize('name', ['gauss200x173x2', 'gauss300x260x64', 'gauss140x140x1', 'const300x260x48'])
def test_frechet_distance_of_numpy_statistics_within_the_bound(name):
    f = fixture(name)
    (mu1, s1), (mu2, s2) = np_stats(f['real']), np_stats(f['fake'])
    value = metrics.calculate_frechet_distance(mu1, s1, mu2, s2)
    print('\nnp.cov statistics of %s: error %.3g  bound %.3g' % (name, abs(value - f['fd']), f['bound']))
    assert abs(value - f['fd']) <= f['bound']
    assert metrics.calculate_frechet_distance(torch.from_numpy(mu1), torch.from_numpy(s1).to(DEV), mu2, s2) == value


# ---------------------------------------------------------------- 11: end to end
def test_evaluate_fid_with_samples_generated_and_precomputed_statistics(tmp_path):
    net, N, real = toy(), 300, real_toy(300)
    results = []
    for bs in (128, 300):
        method, gm, ev = managers()
        results.append(ev.evaluate_fid({'default': net}, real, N, bs))
        assert method.calls == 1 and ev.evals['fid'] == [results[-1]]
        assert ev.evals['mmd'] == [] and ev.evals['precision'] == [] and ev.evals['wass'] == []
    method, gm, ev = managers()
    _, samples = ev.evaluate_mmd({'default': net}, real, N, 300, return_samples=True)
    _, _, other = managers()
    results.append(other.evaluate_fid({}, real, N, 64, samples=samples))
    print('\nevaluate_fid: %s' % results)
    assert results[0] == results[1] == results[2] and isinstance(results[0], float)          # no dependence on the chunking
    x, y = real[:N].numpy().reshape(N, -1), samples.cpu().numpy().reshape(N, -1)
    o, bound = model_of(x, y)
    assert abs(results[0] - o['fd']) <= bound and results[0] == metrics.fd(x, y)
    # precomputed statistics: a pair, and the reference's .npz layout
    mu, sigma = metrics.feature_statistics(real[:N])
    path = str(tmp_path / 'stats.npz')
    np.savez(path, mu=mu.cpu().numpy(), sigma=sigma.cpu().numpy())
    assert other.evaluate_fid({}, None, N, 64, real_stats=path, samples=samples) == results[0]
    assert other.evaluate_fid({}, None, N, 64, real_stats=(mu, sigma), samples=samples) == results[0]
    assert other.evals['fid'] == [results[0]] * 3


def test_evaluate_fid_with_a_features_callable():
    net, N, real = toy(), 200, real_toy(200)
    W = torch.randn(2, 24, generator=torch.Generator().manual_seed(5)).to(DEV)
    seen = []

    def features(x):
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape[1:]) == (1, 2)
        seen.append(x.shape[0])
        return x.reshape(x.shape[0], -1) @ W

    method, gm, ev = managers()
    _, samples = ev.evaluate_mmd({'default': net}, real, N, 200, return_samples=True)
    value = ev.evaluate_fid({}, real, N, 64, features=features, samples=samples)
    assert seen == [64, 64, 64, 8] * 2
    mapped = [torch.cat([t[i:i + 64].reshape(-1, 2).to(DEV) @ W for i in range(0, N, 64)]) for t in (real[:N], samples)]
    assert value == metrics.fd(mapped[0], mapped[1]) and ev.evals['fid'] == [value]
    # 24 features of rank 2: 22 null directions
    o, bound = model_of(mapped[0].cpu().numpy(), mapped[1].cpu().numpy())
    print('\nfeatures=: fd %.17g  oracle %.17g  error %.3g  bound %.3g  z %d' % (value, o['fd'], abs(value - o['fd']), bound, o['z']))
    assert o['z'] == 22 and abs(value - o['fd']) <= bound
    with pytest.raises(AssertionError, match=r'evaluate_fid: features must return float32 \[B, F\]'):
        ev.evaluate_fid({}, real, N, 64, features=lambda x: x.double().reshape(x.shape[0], -1), samples=samples)


def test_cli_eval_fid_prints_the_api_figure_and_saves_the_statistics(tmp_path):
    real = torch.randn(300, 1, 2, generator=torch.Generator().manual_seed(42)).numpy()
    path, out, stats = str(tmp_path / 'real.npy'), str(tmp_path / 'gen.npy'), str(tmp_path / 'stats.npz')
    np.save(path, real)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'dlpm_amd.cli', '--config', '2d_data', '--synthetic_weights', '1', '--set_seed', '3',
                        '--reverse_steps', '10', '--generate', '256', '--batch_size', '100', '--eval_fid', path, '--save_fid_stats', stats,
                        '--out', out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    words = r.stdout.strip().splitlines()[-1].split()
    print('\ncli: %s' % ' '.join(words))
    assert words[0] == 'fid' and words[2:] == 'over 256 generated vs 256 real samples'.split()
    samples = np.load(out)
    want = metrics.fd(real[:256], samples)
    assert samples.shape == (256, 1, 2) and float(words[1]) == pytest.approx(want, rel=1e-8)
    z = np.load(stats)
    mu, sigma = metrics.feature_statistics(real[:256])
    assert z['mu'].dtype == np.float64 and np.array_equal(z['mu'], mu.cpu().numpy()) and np.array_equal(z['sigma'], sigma.cpu().numpy())
    assert metrics.calculate_frechet_distance(z['mu'], z['sigma'], *metrics.feature_statistics(samples)) == want


# ---------------------------------------------------------------- the C entry points' refusals, with device pointers
def test_c_entry_point_refusals_leave_the_outputs_alone():
    L = _lib.lib()
    x, y = torch.randn(40, 3, device=DEV), torch.randn(30, 3, device=DEV)
    need = L.dlpm_fd_workspace_bytes(40, 30, 3)
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=DEV)
    out = torch.full((8,), -7.0, dtype=torch.float64, device=DEV)
    good = dict(x=x.data_ptr(), n1=40, y=y.data_ptr(), n2=30, F=3, ws=ws.data_ptr(), wsb=need, out=out.data_ptr())

    def call(**o):
        a = dict(good, **o)
        return L.dlpm_fd_f32(a['x'], a['n1'], a['y'], a['n2'], a['F'], a['ws'], a['wsb'], a['out'], _lib.stream_ptr())

    for over, code in [(dict(n1=1), -1), (dict(n2=0), -1), (dict(F=0), -1), (dict(F=4097), -1), (dict(x=None), -1), (dict(y=None), -1),
                       (dict(ws=None), -1), (dict(out=None), -1), (dict(ws=ws.data_ptr() + 8), -1), (dict(wsb=need - 1), -5), (dict(wsb=0), -5)]:
        assert call(**over) == code, over
    torch.cuda.synchronize()
    assert (out == -7.0).all()                                            # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert float(out[5]) == 0 and float(out[0]) == metrics.fd(x, y)
