"""Frechet distance from features without a GPU: the oracle `np_fd` (fp64, singular values of A B^T: no covariance is formed, so the
null-space noise of every covariance-based recipe is absent); the reference's recipe (np.cov + calculate_frechet_distance of
bem/evaluate/fid_score.py:118-171) restated in numpy / scipy; the fixture family tests/golden/f21_fd.npz (tools/make_fd_fixtures.py)
with the conditions its cases must meet; the error model the GPU tests hold the device to; and every refusal of the Python layer and
of the C entry points, all of which fire before the GPU is touched."""
import inspect
import os

import numpy as np
import pytest
import torch

import dlpm_amd
from dlpm_amd import _lib, metrics
from metric_helpers import buffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'f21_fd.npz')
EPS = 2.0 ** -53

# (n1, n2, F)
FULL_CASES = [(200, 173, 2), (129, 131, 17), (300, 260, 64), (300, 260, 129), (600, 500, 256), (140, 140, 1)]
NULL_GAUSS = (40, 50, 64)                # n < F
NULL_CONST = (300, 260, 48)              # five constant columns and one duplicated column
HADAMARD = (64, 64, 16)
HAD_A, HAD_B, HAD_C = 0.5, 0.75, 0.25
STORED_ROWS_MAX_F = 64                   # wider cases store their seed and recipe, not their rows (the committed-file limit)
KINDS = {'gauss': 0, 'const': 1, 'hadamard': 2}


def case_name(kind, n1, n2, F):
    return '%s%dx%dx%d' % (kind, n1, n2, F)


FULL_NAMES = [case_name('gauss', *c) for c in FULL_CASES]
NULL_NAMES = [case_name('gauss', *NULL_GAUSS), case_name('const', *NULL_CONST)]
HAD_NAME = case_name('hadamard', *HADAMARD)
ALL_NAMES = FULL_NAMES + NULL_NAMES + [HAD_NAME]


def seed_of(kind, n1, n2, F):
    return 2100 + 7 * F + n1 % 13 + KINDS[kind]


def rows_of(kind, seed, n1, n2, F):
    """The recipe of a case, float32.  gauss: real ~ N(0, s_d^2) with s_d = 0.5 + d / F, fake ~ 1.1 x that + 0.3 / sqrt(F) in every
    coordinate.  const: the same, then columns 0..4 constant (0.7 in real, 0.4 in fake) and column 9 a copy of column 8.  hadamard:
    the 64 rows of the Sylvester Hadamard matrix without its all-ones column, first F columns, real = a H, fake = b H + c."""
    if kind == 'hadamard':
        H = np.array([[1.0]])
        while H.shape[0] < 64:
            H = np.block([[H, H], [H, -H]])
        H = H[:, 1:1 + F]
        return (HAD_A * H).astype(np.float32), (HAD_B * H + HAD_C).astype(np.float32)
    rs = np.random.RandomState(seed)
    s = 0.5 + np.arange(F) / F
    real = (rs.standard_normal((n1, F)) * s).astype(np.float32)
    fake = (rs.standard_normal((n2, F)) * (1.1 * s) + 0.3 / np.sqrt(F)).astype(np.float32)
    if kind == 'const':
        real[:, :5], fake[:, :5] = 0.7, 0.4
        real[:, 9], fake[:, 9] = real[:, 8], fake[:, 8]
    return real, fake


def np_fd(x, y):
    """The oracle: dict(fd, mean_term, tr1, tr2, tr_sqrt, z).  With A = (x - mean) / sqrt(n1 - 1) and B likewise, the singular values of
    A B^T are the square roots of the eigenvalues of sigma1 sigma2; z = how many of the first F fall below 1e-10 of the largest
    (those that do not exist, n < F, included)."""
    x, y = np.asarray(x, np.float64).reshape(len(x), -1), np.asarray(y, np.float64).reshape(len(y), -1)
    F = x.shape[1]
    A = (x - x.mean(axis=0)) / np.sqrt(len(x) - 1)
    B = (y - y.mean(axis=0)) / np.sqrt(len(y) - 1)
    sv = np.linalg.svd(A @ B.T, compute_uv=False)
    first = sv[:F]
    z = int((first < 1e-10 * sv[0]).sum()) + max(0, F - len(first))
    dm = float(((x.mean(axis=0) - y.mean(axis=0)) ** 2).sum())
    t1, t2, ts = float((A * A).sum()), float((B * B).sum()), float(sv.sum())
    return dict(fd=dm + t1 + t2 - 2 * ts, mean_term=dm, tr1=t1, tr2=t2, tr_sqrt=ts, z=z)


def np_stats(x):
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    return x.mean(axis=0), np.atleast_2d(np.cov(x, rowvar=False))


def reference_recipe(mu1, sigma1, mu2, sigma2):
    """calculate_frechet_distance as fid_score.py:118-171 writes it: fractional_matrix_power of the product, the imaginary part
    stripped, |diff|^2 + tr sigma1 + tr sigma2 - 2 tr covmean.  (Its singular-product branch is restated too; no case here takes it.)"""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    diff = mu1 - mu2
    covmean = linalg.fractional_matrix_power(sigma1.dot(sigma2), 0.5)
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * 1e-6
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError('Imaginary component {}'.format(np.max(np.abs(covmean.imag))))
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))


def ref_fd(x, y):
    return reference_recipe(*np_stats(x), *np_stats(y))


def bound_of(F, ref_dev, scale, z, tr1, tr2):
    """The error model: the device is held to the reference's own distance from the oracle (x 8: it factorises in another order), with
    a floor of F eigenvalues of F EPS |.| error each over two solves, plus the square root of an fp64-zero eigenvalue of K
    (|K| <= tr sigma1 tr sigma2) once per null direction."""
    return max(8 * ref_dev, 64 * F * EPS * scale) + 2 * z * np.sqrt(F * EPS * tr1 * tr2)


_fixture = {}


def fixture(name):
    """Case `name` of f21_fd.npz as a dict; the rows of a wide case come from its stored seed and recipe; built once and shared."""
    if name not in _fixture:
        z = np.load(FIXTURE)
        n1, n2, F, seed, kind = (int(v) for v in z[name + '.meta'])
        kind = [k for k, v in KINDS.items() if v == kind][0]
        if name + '.real' in z.files:
            real, fake = z[name + '.real'], z[name + '.fake']
        else:
            real, fake = rows_of(kind, seed, n1, n2, F)
        for a in (real, fake):
            a.setflags(write=False)
        terms = z[name + '.terms']
        f = dict(real=real, fake=fake, n1=n1, n2=n2, F=F, seed=seed, kind=kind, fd=float(z[name + '.fd']), mean_term=float(terms[0]),
                 tr1=float(terms[1]), tr2=float(terms[2]), tr_sqrt=float(terms[3]), ref_fd=float(z[name + '.ref_fd']),
                 ref_dev=float(z[name + '.ref_dev']), scale=float(z[name + '.scale']), z=int(z[name + '.z']), digest=z[name + '.digest'],
                 recipe=str(z[name + '.recipe']))
        f['bound'] = bound_of(F, f['ref_dev'], f['scale'], f['z'], f['tr1'], f['tr2'])
        _fixture[name] = f
    return _fixture[name]


# ---------------------------------------------------------------- the fixture family
def test_fixture_holds_every_case_and_is_small():
    z = np.load(FIXTURE)
    assert sorted(str(n) for n in z['names']) == sorted(ALL_NAMES)
    assert os.path.getsize(FIXTURE) < 400 * 1024
    for name in ALL_NAMES:
        f = fixture(name)
        assert name == case_name(f['kind'], f['n1'], f['n2'], f['F'])
        assert (name + '.real' in z.files) == (f['F'] <= STORED_ROWS_MAX_F)
        assert f['seed'] == seed_of(f['kind'], f['n1'], f['n2'], f['F']) and f['kind'] in f['recipe']


@pytest.mark.parametrize('name', ALL_NAMES)
def test_fixture_rows_follow_their_recipe_and_the_oracle_agrees_with_the_reference_recipe(name):
    f = fixture(name)
    real, fake = rows_of(f['kind'], f['seed'], f['n1'], f['n2'], f['F'])
    assert np.array_equal(real, f['real']) and np.array_equal(fake, f['fake'])
    assert f['digest'].tolist() == [float(real.astype(np.float64).sum()), float(fake.astype(np.float64).sum())]
    o = np_fd(real, fake)
    ref = ref_fd(real, fake)
    scale = o['tr1'] + o['tr2']
    print('\n%s: fd %.17g  ref %.17g  ref_dev %.3g  stored %.3g  z %d  bound %.3g' % (name, o['fd'], ref, abs(ref - o['fd']), f['ref_dev'],
                                                                                 o['z'], f['bound']))
    # the stored figures are those of this machine's LAPACK to a few ulp of the terms; z is an integer and must be equal
    tiny = 64 * EPS * scale
    assert abs(o['fd'] - f['fd']) <= tiny and o['z'] == f['z'] and abs(scale - f['scale']) <= tiny
    for key in ('mean_term', 'tr1', 'tr2', 'tr_sqrt'):
        assert abs(o[key] - f[key]) <= tiny, key
    assert f['ref_dev'] == abs(f['ref_fd'] - f['fd'])
    if name in FULL_NAMES:
        floor = 64 * f['F'] * EPS * scale
        assert o['z'] == 0 and f['ref_dev'] <= floor and abs(ref - o['fd']) <= floor
    elif name in NULL_NAMES:
        assert o['z'] >= 5
        assert abs(ref - o['fd']) <= f['bound']            # the restated recipe sits inside the model as well
    assert abs(ref - f['ref_fd']) <= max(8 * f['ref_dev'], f['bound'])


def test_hadamard_closed_form():
    f = fixture(HAD_NAME)
    F = f['F']
    mu1, s1 = np_stats(f['real'])
    mu2, s2 = np_stats(f['fake'])
    assert np.array_equal(s1, HAD_A ** 2 * 64 / 63 * np.eye(F)) and np.array_equal(mu1, np.zeros(F))
    assert np.abs(s2 - HAD_B ** 2 * 64 / 63 * np.eye(F)).max() <= 4 * EPS and np.array_equal(mu2, np.full(F, HAD_C))
    want = F * (64 / 63) * (HAD_A - HAD_B) ** 2 + F * HAD_C ** 2
    assert abs(f['fd'] - want) <= f['bound'] and abs(np_fd(f['real'], f['fake'])['fd'] - want) <= f['bound']
    assert abs(f['ref_fd'] - want) <= f['bound'] and f['z'] == 0


def test_error_model_arithmetic():
    assert bound_of(64, 0.0, 10.0, 0, 5.0, 5.0) == 64 * 64 * EPS * 10.0
    assert bound_of(64, 1.0, 10.0, 0, 5.0, 5.0) == 8.0
    assert bound_of(4, 0.0, 1.0, 3, 2.0, 8.0) == 64 * 4 * EPS + 2 * 3 * np.sqrt(4 * EPS * 16.0)


# ---------------------------------------------------------------- exports, mirrors, signatures
def test_exports_and_mirrors():
    for name in ('fd', 'fd_device', 'feature_statistics', 'calculate_frechet_distance'):
        assert getattr(dlpm_amd, name) is getattr(metrics, name)
    assert metrics.MAX_FEATURES == 4096


def test_signatures_and_docstrings():
    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(metrics.calculate_frechet_distance) == [('mu1', E), ('sigma1', E), ('mu2', E), ('sigma2', E), ('eps', 1e-6)]
    assert sig(metrics.fd) == [('real', E), ('fake', E), ('return_parts', False)]
    assert sig(metrics.fd_device) == [('real', E), ('fake', E)]
    assert sig(metrics.feature_statistics) == [('features', E)]
    assert sig(dlpm_amd.EvaluationManager.evaluate_fid)[1:] == [
        ('models', E), ('real_data', E), ('data_to_generate', E), ('batch_size', E), ('class_labels', None), ('features', None),
        ('real_stats', None), ('samples', None), ('kwargs', E)]
    assert 'unused' in metrics.calculate_frechet_distance.__doc__
    assert 'graph' in metrics.fd_device.__doc__
    assert 'Inception pool3' in dlpm_amd.EvaluationManager.evaluate_fid.__doc__


# ---------------------------------------------------------------- refusals
def test_workspace_bytes_refusals_and_growth():
    L = _lib.lib()
    ws = L.dlpm_fd_workspace_bytes
    for args, word in [((1, 40, 2), 'at least 2 rows'), ((40, 1, 2), 'at least 2 rows'), ((0, 0, 2), 'at least 2 rows'), ((-5, 40, 2), 'at least 2'),
                       ((40, 40, 0), 'F must be'), ((40, 40, 4097), 'F must be'), ((40, 40, -1), 'F must be'), ((1 << 31, 40, 2), 'out of range')]:
        assert ws(*args) == -1, args
        assert word.encode() in L.dlpm_last_error(), (args, L.dlpm_last_error())
    assert ws(2, 2, 1) > 0 and ws(2, 2, 4096) > 0
    # five F x F fp64 matrices, 36 vectors of F, and the partial tiles of the covariance: one 128 KB tile per (chunk, tile), at most
    # 64 chunks of at least 256 rows and about 512 partial tiles in all
    F = 2048
    assert 5 * F * F * 8 <= ws(2, 2, F) <= 5 * F * F * 8 + 36 * F * 8 + 136 * 131072 + 16 * 256
    assert ws(50000, 50000, F) - ws(2, 2, F) == (512 // 136 - 1) * 136 * 131072
    assert ws(50000, 300, 64) == ws(300, 50000, 64) and ws(50000, 50000, 64) - ws(2, 2, 64) == 63 * 131072
    assert ws(511, 511, 64) == ws(2, 2, 64) < ws(512, 512, 64)


def test_c_entry_points_refuse_before_any_launch():
    """No GPU here: every one of these returns before a kernel is launched (the pointers are host addresses, never followed)."""
    L = _lib.lib()
    buf, base = buffers()
    P = [int(base) + 4096 * i for i in range(8)]
    need = L.dlpm_fd_workspace_bytes(40, 30, 3)
    assert 0 < need
    good = dict(x=P[0], n1=40, y=P[1], n2=30, F=3, ws=P[6], wsb=need, out=P[5], mu=P[2], sigma=P[3], status=P[4], mu2=P[1], sigma2=P[7])

    def call_fd(**o):
        a = dict(good, **o)
        return L.dlpm_fd_f32(a['x'], a['n1'], a['y'], a['n2'], a['F'], a['ws'], a['wsb'], a['out'], None)

    def call_stats(**o):
        a = dict(good, **o)
        return L.dlpm_fd_stats_f32(a['x'], a['n1'], a['F'], a['ws'], a['wsb'], a['mu'], a['sigma'], a['status'], None)

    def call_from(**o):
        a = dict(good, **o)
        return L.dlpm_fd_from_stats_f64(a['mu'], a['sigma'], a['mu2'], a['sigma2'], a['F'], a['ws'], a['wsb'], a['out'], None)

    shared = [(dict(F=0), 'F must be'), (dict(F=4097), 'F must be'), (dict(ws=None), 'null'), (dict(ws=P[6] + 8), 'misaligned')]
    cases = {
        call_fd: shared + [(dict(n1=1), 'at least 2'), (dict(n2=1), 'at least 2'), (dict(n1=0), 'at least 2'), (dict(n2=-4), 'at least 2'),
                           (dict(x=None), 'null'), (dict(y=None), 'null'), (dict(out=None), 'null'), (dict(x=P[0] + 2), 'misaligned'),
                           (dict(out=P[5] + 4), 'misaligned')],
        call_stats: shared + [(dict(n1=1), 'at least 2'), (dict(x=None), 'null'), (dict(mu=None), 'null'), (dict(sigma=None), 'null'),
                              (dict(status=None), 'null'), (dict(mu=P[2] + 4), 'misaligned'), (dict(status=P[4] + 2), 'misaligned')],
        call_from: shared + [(dict(mu=None), 'null'), (dict(sigma=None), 'null'), (dict(mu2=None), 'null'), (dict(sigma2=None), 'null'),
                             (dict(out=None), 'null'), (dict(sigma2=P[7] + 4), 'misaligned')],
    }
    for call, overs in cases.items():
        for over, word in overs:
            with pytest.raises(ValueError, match=word):
                _lib.check(call(**over))
        with pytest.raises(_lib.DlpmError, match='workspace'):
            _lib.check(call(wsb=7))
        assert call(wsb=7) == -5                                           # DLPM_ERR_NOMEM
    assert call_fd(wsb=need - 1) == -5
    assert call_stats(wsb=L.dlpm_fd_workspace_bytes(40, 40, 3) - 1) == -5
    assert call_from(wsb=L.dlpm_fd_workspace_bytes(2, 2, 3) - 1) == -5


def test_python_refusals_touch_no_device():
    x = torch.zeros(40, 2)
    for fn in (metrics.fd, metrics.fd_device):
        for bad, word in [((x.double(), x), 'float32'), ((x, x.to(torch.float16)), 'float32'), ((np.zeros((40, 2), np.int64), x), 'float32'),
                          ((x, torch.zeros(40, 3)), 'values'), ((torch.zeros(0, 2), x), 'at least one point'), ((x[:1], x), 'at least 2 rows'),
                          ((x, x[:1]), 'at least 2 rows'), ((torch.zeros(3, 4097), torch.zeros(3, 4097)), 'at most 4096'),
                          ((torch.zeros(3, 3, 64, 64), torch.zeros(3, 3, 64, 64)), 'features=')]:
            with pytest.raises(AssertionError, match=word):
                fn(*bad)
    with pytest.raises(AssertionError, match='at least 2 rows'):
        metrics.fd(x[:1], x, return_parts=True)
    for bad, word in [(x.double(), 'float32'), (x[:1], 'at least 2 rows'), (torch.zeros(3, 5000), 'at most 4096')]:
        with pytest.raises(AssertionError, match=word):
            metrics.feature_statistics(bad)
    mu, s = np.zeros(3), np.eye(3)
    for bad, word in [((mu.astype(np.float32), s, mu, s), 'float64'), ((mu, s, mu, s.astype(np.float32)), 'float64'),
                      ((mu, s, np.zeros(4), s), 'different lengths'), ((mu, s, mu, np.eye(4)), 'different dimensions'),
                      ((mu, np.eye(4), mu, np.eye(4)), r'sigma must be \[3, 3\]'), ((mu, np.zeros((3, 3, 1)), mu, np.zeros((3, 3, 1))), 'dimension'),
                      ((np.zeros(4097), np.zeros((4097, 4097)), np.zeros(4097), np.zeros((4097, 4097))), 'at most 4096')]:
        with pytest.raises(AssertionError, match=word):
            metrics.calculate_frechet_distance(*bad)


def test_evaluate_fid_refusals_leave_evals_untouched(tmp_path):
    ev = dlpm_amd.EvaluationManager(None, None, None, verbose=False)
    real = np.zeros((8, 1, 2), np.float32)
    gen = np.zeros((8, 1, 2), np.float32)
    with pytest.raises(AssertionError, match='float32'):
        ev.evaluate_fid({}, np.zeros((8, 1, 2)), 8, 4)
    with pytest.raises(AssertionError, match='real samples'):
        ev.evaluate_fid({}, real[:4], 8, 4)
    with pytest.raises(AssertionError, match='at least 2 samples'):
        ev.evaluate_fid({}, real, 1, 4)
    with pytest.raises(AssertionError, match='samples given'):
        ev.evaluate_fid({}, real, 8, 4, samples=gen[:7])
    with pytest.raises(AssertionError, match='callable'):
        ev.evaluate_fid({}, real, 8, 4, features='inception', samples=gen)
    with pytest.raises(AssertionError, match='float64 real_stats'):
        ev.evaluate_fid({}, None, 8, 4, real_stats=(np.zeros(2, np.float32), np.eye(2)), samples=gen)
    with pytest.raises(AssertionError, match='real_stats of shapes'):
        ev.evaluate_fid({}, None, 8, 4, real_stats=(np.zeros(2), np.eye(3)), samples=gen)
    with pytest.raises(AssertionError, match='real_stats of 3 features'):
        ev.evaluate_fid({}, None, 8, 4, real_stats=(np.zeros(3), np.eye(3)), samples=gen)
    path = str(tmp_path / 'stats.npz')
    np.savez(path, mu=np.zeros(3), sigma=np.eye(3))
    with pytest.raises(AssertionError, match='real_stats of 3 features'):
        ev.evaluate_fid({}, None, 8, 4, real_stats=path, samples=gen)
    with pytest.raises(AssertionError, match='at most 4096'):
        ev.evaluate_fid({}, np.zeros((4, 3, 64, 64), np.float32), 4, 4, samples=np.zeros((4, 3, 64, 64), np.float32))
    assert all(ev.evals[k] == [] for k in ('wass', 'mmd', 'precision', 'recall', 'density', 'coverage', 'fid', 'f_1_pr', 'f_1_dc', 'fig'))
