"""PRDC (precision, recall, density, coverage by k-nearest neighbours) without a GPU: `np_prdc`, the definition restated in numpy fp64
with direct differences; the `prdc` package's own recipe (sklearn pairwise_distances, argpartition, the four expressions as written)
that it is held to; the fixture family tests/golden/f20_prdc.npz (tools/make_prdc_fixtures.py) with the two conditions its cases must
meet; and every refusal of the Python layer and of the C entry points, all of which fire before the GPU is touched."""
import inspect
import os

import numpy as np
import pytest
import torch

import dlpm_amd
from dlpm_amd import _lib, metrics
from metric_helpers import buffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'f20_prdc.npz')

# (n1, n2, D, k): every one straddles a 128 tile edge or a segment edge somewhere
GAUSS_CASES = [(200, 173, 2, 5), (129, 131, 16, 3), (129, 131, 17, 5), (300, 260, 64, 5), (160, 150, 2048, 5), (140, 140, 8, 1),
               (140, 150, 24, 32)]
LATTICE_CASE = (150, 140, 2, 4)          # integer coordinates in 0..5: duplicates and exact ties everywhere
STORED_ROWS_MAX_D = 64                   # wider cases store their seed and recipe, not their rows (the committed-file limit)
MIN_GAP = 1e-9                           # condition (a)


def case_name(n1, n2, D, k, lattice=False):
    return '%s%dx%dx%dk%d' % ('lattice' if lattice else 'gauss', n1, n2, D, k)


ALL_NAMES = [case_name(*c) for c in GAUSS_CASES] + [case_name(*LATTICE_CASE, lattice=True)]


def gauss_rows(seed, n1, n2, D, scale, shift):
    """The recipe of a Gaussian case: real ~ N(0, 1), fake ~ N(shift / sqrt(D) in every coordinate, scale^2), float32."""
    rs = np.random.RandomState(seed)
    real = rs.standard_normal((n1, D)).astype(np.float32)
    fake = (rs.standard_normal((n2, D)) * scale + shift / np.sqrt(D)).astype(np.float32)
    return real, fake


def lattice_rows(seed, n1, n2, D):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 6, (n1, D)).astype(np.float32), rs.randint(0, 6, (n2, D)).astype(np.float32)


def sq_dists(a, b):
    """Squared Euclidean distances in fp64 by direct differences, summed in d order (exact on integer-valued inputs)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.zeros((a.shape[0], b.shape[0]))
    for d in range(a.shape[1]):
        df = a[:, d][:, None] - b[:, d][None, :]
        out += df * df
    return out


def figures_of(counts, n1, n2, k):
    return {'precision': int(counts[0]) / n2, 'recall': int(counts[1]) / n1, 'density': int(counts[2]) / (k * n2),
            'coverage': int(counts[3]) / n1}


def np_prdc(real, fake, k):
    """The definition: (counts int64 [4], figures, radii_real, radii_fake, (d2 real x fake, squared radii of real, of fake))."""
    real = np.asarray(real, np.float64).reshape(len(real), -1)
    fake = np.asarray(fake, np.float64).reshape(len(fake), -1)
    rg = sq_dists(real, fake)
    r2 = np.partition(sq_dists(real, real), k, axis=1)[:, k]            # the (k+1)-th smallest, itself included, with multiplicity
    g2 = np.partition(sq_dists(fake, fake), k, axis=1)[:, k]
    inside_r, inside_g = rg < r2[:, None], rg < g2[None, :]
    counts = np.array([inside_r.any(axis=0).sum(), inside_g.any(axis=1).sum(), inside_r.sum(), (rg.min(axis=1) < r2).sum()], np.int64)
    return counts, figures_of(counts, len(real), len(fake), k), np.sqrt(r2), np.sqrt(g2), (rg, r2, g2)


def centred_norms(real, fake):
    """|c|^2 of the rows of both sets, centred on the pooled mean, in fp64."""
    real, fake = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    m = np.concatenate([real, fake]).mean(axis=0)
    return ((real - m) ** 2).sum(axis=1), ((fake - m) ** 2).sum(axis=1)


def decision_gap(real, fake, parts):
    """min over all pairs of |d2(R_i, G_j) - r_i^2| and |d2 - g_j^2|, divided by |c_i|^2 + |c_j|^2."""
    rg, r2, g2 = parts
    cr, cg = centred_norms(real, fake)
    den = cr[:, None] + cg[None, :]
    return float(min((np.abs(rg - r2[:, None]) / den).min(), (np.abs(rg - g2[None, :]) / den).min()))


def package_recipe(real_features, fake_features, nearest_k):
    """compute_prdc of the `prdc` package as it is written (prdc/prdc.py), with its helpers inlined."""
    import sklearn.metrics

    def pairwise(x, y=None):
        return sklearn.metrics.pairwise_distances(x, x if y is None else y, metric='euclidean', n_jobs=1)

    def kth(unsorted, k, axis=-1):
        indices = np.argpartition(unsorted, k, axis=axis)[..., :k]
        return np.take_along_axis(unsorted, indices, axis=axis).max(axis=axis)

    def radii(x, k):
        return kth(pairwise(x), k=k + 1, axis=-1)

    real_r, fake_r = radii(real_features, nearest_k), radii(fake_features, nearest_k)
    dist = pairwise(real_features, fake_features)
    precision = (dist < np.expand_dims(real_r, axis=1)).any(axis=0).mean()
    recall = (dist < np.expand_dims(fake_r, axis=0)).any(axis=1).mean()
    density = (1. / float(nearest_k)) * (dist < np.expand_dims(real_r, axis=1)).sum(axis=0).mean()
    coverage = (dist.min(axis=1) < real_r).mean()
    return dict(precision=precision, recall=recall, density=density, coverage=coverage), real_r, fake_r


_fixture = {}


def fixture(name):
    """Case `name` of f20_prdc.npz: dict(real, fake, n1, n2, D, k, seed, scale, shift, counts, radii_real, radii_fake, gap).  The rows
    of a wide case come from its stored seed and recipe; every case is built once and shared."""
    if name not in _fixture:
        z = np.load(FIXTURE)
        n1, n2, D, k, seed = (int(v) for v in z[name + '.meta'])
        scale, shift = (float(v) for v in z[name + '.params'])
        if name + '.real' in z.files:
            real, fake = z[name + '.real'], z[name + '.fake']
        else:
            real, fake = gauss_rows(seed, n1, n2, D, scale, shift)
        for a in (real, fake):
            a.setflags(write=False)
        _fixture[name] = dict(real=real, fake=fake, n1=n1, n2=n2, D=D, k=k, seed=seed, scale=scale, shift=shift, counts=z[name + '.counts'],
                              radii_real=z[name + '.radii_real'], radii_fake=z[name + '.radii_fake'], gap=float(z[name + '.gap']),
                              digest=z[name + '.digest'], lattice=name.startswith('lattice'))
    return _fixture[name]


# ---------------------------------------------------------------- the restatement against the package's recipe
@pytest.mark.parametrize('seed,n1,n2,D,k', [(11, 90, 75, 3, 5), (12, 64, 80, 40, 3), (13, 120, 100, 300, 7)])
def test_np_prdc_equals_the_package_recipe(seed, n1, n2, D, k):
    real, fake = gauss_rows(seed, n1, n2, D, 1.03, 0.5)
    counts, fig, rr, rf, _ = np_prdc(real, fake, k)
    want, want_rr, want_rf = package_recipe(real.astype(np.float64), fake.astype(np.float64), k)
    for key in ('precision', 'recall', 'coverage'):
        assert fig[key] == float(want[key]), (key, fig[key], want[key])
    # the package writes density as (1 / k) * mean(column sums): the same integer, divided in another order (two roundings, not one)
    assert round(float(want['density']) * k * n2) == counts[2] and abs(fig['density'] - float(want['density'])) <= 4e-16 * fig['density']
    assert np.abs(rr / want_rr - 1).max() <= 1e-9 and np.abs(rf / want_rf - 1).max() <= 1e-9


def test_np_prdc_on_a_case_done_by_hand():
    # real: 0, 1, 2, 10 on a line, k = 1: radii 1, 1, 1, 8.  fake: 0.5, 2.9, 30: radii 2.4, 2.4, 27.1
    real = np.array([[0.], [1.], [2.], [10.]], np.float32)
    fake = np.array([[0.5], [2.9], [30.]], np.float32)
    counts, fig, rr, rf, _ = np_prdc(real, fake, 1)
    assert rr.tolist() == [1., 1., 1., 8.]
    assert np.allclose(rf, [2.4, 2.4, 27.1], rtol=1e-6)
    # inside real balls: 0.5 in balls of 0, 1 (and of 10? |10 - 0.5| = 9.5 no); 2.9 in ball of 2 (0.9) and of 10 (7.1); 30 in none
    # inside fake balls: 0 (0.5 < 2.4), 1, 2 (1.5 < 2.4), 10 (|10 - 30| = 20 < 27.1)
    # coverage: nearest fake of 0 is 0.5 < 1; of 1: 0.5 < 1; of 2: 0.9 < 1; of 10: 7.1 < 8
    assert counts.tolist() == [2, 4, 4, 4]
    assert fig == {'precision': 2 / 3, 'recall': 1.0, 'density': 4 / 3, 'coverage': 1.0}


def test_strict_comparison_and_multiplicity_on_a_lattice():
    real = np.array([[0, 0], [0, 0], [1, 0], [3, 0]], np.float32)       # a duplicate: the 2nd smallest of row 0 is 0
    fake = np.array([[0, 0], [1, 0], [2, 0]], np.float32)
    counts, fig, rr, rf, _ = np_prdc(real, fake, 1)
    assert rr.tolist() == [0., 0., 1., 2.] and rf.tolist() == [1., 1., 1.]
    # d < 0 never; ball of (1, 0) radius 1: strictly inside only the fake (1, 0); ball of (3, 0) radius 2: only (2, 0)
    # recall: both (0, 0) and (1, 0) lie at distance 0 from a fake point; (3, 0) is at exactly 1 from (2, 0), whose radius is 1: outside
    assert counts.tolist() == [2, 3, 2, 2]


# ---------------------------------------------------------------- the fixture family
def test_fixture_holds_every_case_and_is_small():
    z = np.load(FIXTURE)
    assert sorted(str(n) for n in z['names']) == sorted(ALL_NAMES)
    assert os.path.getsize(FIXTURE) < 400 * 1024
    for name in ALL_NAMES:
        f = fixture(name)
        assert (f['n1'], f['n2'], f['D'], f['k']) == ((LATTICE_CASE if f['lattice'] else GAUSS_CASES[ALL_NAMES.index(name)]))
        assert (name + '.real' in z.files) == (f['D'] <= STORED_ROWS_MAX_D)


@pytest.mark.parametrize('name', ALL_NAMES)
def test_fixture_rows_follow_their_recipe_and_results_follow_np_prdc(name):
    f = fixture(name)
    if f['lattice']:
        real, fake = lattice_rows(f['seed'], f['n1'], f['n2'], f['D'])
    else:
        real, fake = gauss_rows(f['seed'], f['n1'], f['n2'], f['D'], f['scale'], f['shift'])
    assert np.array_equal(real, f['real']) and np.array_equal(fake, f['fake'])
    assert f['digest'].tolist() == [float(real.astype(np.float64).sum()), float(fake.astype(np.float64).sum())]
    counts, fig, rr, rf, parts = np_prdc(f['real'], f['fake'], f['k'])
    assert np.array_equal(counts, f['counts'])
    assert np.array_equal(rr, f['radii_real']) and np.array_equal(rf, f['radii_fake'])
    # condition (b): at least three of the four figures lie in (0.05, 0.95)
    inside = [key for key, v in fig.items() if 0.05 < v < 0.95]
    assert len(inside) >= 3, fig
    if f['lattice']:
        assert (parts[0] == parts[1][:, None]).sum() > 100              # exact ties with the radius are everywhere
        assert (sq_dists(real, real) == 0).sum() > len(real)            # duplicates
    else:
        # condition (a): no decision of any pair is closer than 1e-9 of |c_i|^2 + |c_j|^2 -- no pair is excluded
        g = decision_gap(f['real'], f['fake'], parts)
        assert g == f['gap'] and g >= MIN_GAP, (g, f['gap'])


# ---------------------------------------------------------------- f_1 and evals
def test_f_1_arithmetic_and_both_zero_branches():
    assert metrics.f_1(0.5, 0.25) == 2 * 0.5 * 0.25 / 0.75
    assert metrics.f_1(0.0, 0.0) == 0.0 and metrics.f_1(0, 0) == 0.0
    assert metrics.f_1(0.0, 0.7) == 0.0 and metrics.f_1(1.0, 1.0) == 1.0
    assert metrics.f_1(1.25, 0.5) == 2 * 1.25 * 0.5 / 1.75                                    # density may pass 1


def test_evals_keys_are_the_reference_ones():
    ev = dlpm_amd.EvaluationManager(None, None, None, verbose=False)
    assert set(ev.evals) == {'losses', 'losses_batch', 'wass', 'mmd', 'precision', 'recall', 'density', 'coverage', 'f_1_pr', 'f_1_dc', 'fid',
                             'fig', 'grad_norm'}


# ---------------------------------------------------------------- exports and mirrors
def test_exports_and_mirrors():
    for name in ('prdc', 'prdc_device', 'compute_prdc'):
        assert getattr(dlpm_amd, name) is getattr(metrics, name)
    assert callable(dlpm_amd.EvaluationManager.evaluate_prdc)


def test_drop_in_signatures():
    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(metrics.compute_prdc) == [('real_features', E), ('fake_features', E), ('nearest_k', E)]
    assert sig(metrics.prdc)[:4] == [('real', E), ('fake', E), ('nearest_k', 5), ('return_parts', False)]
    assert sig(metrics.prdc_device) == [('real', E), ('fake', E), ('nearest_k', 5), ('return_radii', False)]
    assert sig(dlpm_amd.EvaluationManager.evaluate_prdc)[1:] == [
        ('models', E), ('real_data', E), ('data_to_generate', E), ('batch_size', E), ('class_labels', None), ('nearest_k', 5),
        ('features', None), ('samples', None), ('kwargs', E)]
    assert 'float32' in metrics.compute_prdc.__doc__ and 'ONCE' in metrics.compute_prdc.__doc__


# ---------------------------------------------------------------- refusals
def test_workspace_bytes_refusals_and_growth():
    L = _lib.lib()
    ws = L.dlpm_prdc_workspace_bytes
    for args, word in [((0, 40, 2, 5), 'bad shape'), ((40, 0, 2, 5), 'bad shape'), ((40, 40, 0, 5), 'bad shape'), ((40, 40, 2, 0), 'nearest_k'),
                       ((40, 40, 2, 33), 'nearest_k'), ((40, 5, 2, 5), 'nearest_k'), ((5, 40, 2, 5), 'nearest_k'), ((6, 6, 2, 6), 'nearest_k'),
                       ((1 << 23, 40, 2, 5), 'out of range')]:
        assert ws(*args) == -1, args
        assert word.encode() in L.dlpm_last_error(), (args, L.dlpm_last_error())
    assert ws(6, 6, 2, 5) > 0 and ws(33, 33, 2, 32) > 0
    # O((n1 + n2) (k + 1) segments): the survivors of the larger radii pass (segments x 2 halves x (k + 1) doubles per row; the rule
    # gives 1 segment at 128 rows and 7 at 10^4) and 32 bytes of radii, counts, flags and minima per row, in 256-byte regions
    assert ws(1000, 1000, 2, 5) < ws(1000, 1000, 2, 32)
    assert ws(128, 128, 2, 5) <= 128 * (1 * 2 * 6 * 8 + 32) + 16 * 256
    assert 10000 * 7 * 2 * 6 * 8 <= ws(10000, 10000, 2, 5) <= 10000 * (7 * 2 * 6 * 8 + 32) + 16 * 256
    # the Gram form adds the mean, its chunk sums and one norm per row: nothing n x n, nothing n x D
    assert ws(10000, 10000, 2048, 5) - ws(10000, 10000, 2, 5) <= 33 * 2048 * 8 + 20000 * 8 + 4 * 256


def test_c_entry_point_refuses_before_any_launch():
    """No GPU here: every one of these returns before a kernel is launched (the pointers are host addresses, never followed)."""
    L = _lib.lib()
    buf, base = buffers()
    P = [int(base) + 4096 * i for i in range(7)]
    need = L.dlpm_prdc_workspace_bytes(40, 30, 3, 5)
    assert 0 < need <= 4096 * 9
    good = dict(x=P[0], n1=40, y=P[1], n2=30, D=3, k=5, ws=P[6], wsb=need, rr=P[2], rf=P[3], counts=P[4], out=P[5])

    def call(**o):
        a = dict(good, **o)
        return L.dlpm_prdc_f32(a['x'], a['n1'], a['y'], a['n2'], a['D'], a['k'], a['ws'], a['wsb'], a['rr'], a['rf'], a['counts'], a['out'], None)

    for over, word in [(dict(n1=0), 'bad shape'), (dict(n2=0), 'bad shape'), (dict(D=0), 'bad shape'), (dict(n1=-3), 'bad shape'),
                       (dict(k=0), 'nearest_k'), (dict(k=33), 'nearest_k'), (dict(k=-1), 'nearest_k'), (dict(k=30), 'nearest_k'),
                       (dict(k=31), 'nearest_k'), (dict(n1=5), 'nearest_k'), (dict(n2=4), 'nearest_k'),
                       (dict(x=None), 'null'), (dict(y=None), 'null'), (dict(ws=None), 'null'), (dict(counts=None), 'null'),
                       (dict(out=None), 'null'), (dict(ws=P[6] + 8), 'misaligned'), (dict(x=P[0] + 2), 'misaligned'),
                       (dict(out=P[5] + 4), 'misaligned'), (dict(rr=P[2] + 4), 'misaligned')]:
        with pytest.raises(ValueError, match=word):
            _lib.check(call(**over))
    with pytest.raises(_lib.DlpmError, match='workspace'):
        _lib.check(call(wsb=7))
    assert call(wsb=7) == -5 and call(wsb=need - 1) == -5                  # DLPM_ERR_NOMEM


def test_python_refusals_touch_no_device():
    x = torch.zeros(40, 2)
    for fn in (metrics.prdc, metrics.prdc_device):
        for bad, word in [((x.double(), x), 'float32'), ((x, x.to(torch.float16)), 'float32'), ((np.zeros((40, 2), np.int64), x), 'float32'),
                          ((x, torch.zeros(40, 3)), 'values'), ((torch.zeros(0, 2), x), 'at least one point')]:
            with pytest.raises(AssertionError, match=word):
                fn(*bad)
        for k in (0, 33, -1, 2.5):
            with pytest.raises(AssertionError, match='nearest_k must be'):
                fn(x, x, nearest_k=k)
        for a, b, k in ((x, x[:5], 5), (x[:6], x, 6), (x[:33], x[:33], 32 + 1)):
            with pytest.raises(AssertionError, match='nearest_k'):
                fn(a, b, nearest_k=k)
        with pytest.raises(AssertionError, match='needs more than 5 points'):
            fn(x, x[:5], nearest_k=5)
    for bad, word in [((x.to(torch.float16), x), 'float32 or float64'), ((x, np.zeros((40, 2), np.int32)), 'float32 or float64'),
                      ((x.double(), torch.zeros(40, 3).double()), 'values')]:
        with pytest.raises(AssertionError, match=word):
            metrics.compute_prdc(*bad, nearest_k=5)
    with pytest.raises(AssertionError, match='nearest_k'):
        metrics.compute_prdc(x.double(), x.double()[:4], nearest_k=5)
    with pytest.raises(AssertionError, match='nearest_k must be'):
        metrics.compute_prdc(real_features=x, fake_features=x, nearest_k=40)


def test_evaluate_prdc_refusals_leave_evals_untouched():
    ev = dlpm_amd.EvaluationManager(None, None, None, verbose=False)
    real = np.zeros((8, 1, 2), np.float32)
    with pytest.raises(AssertionError, match='float32'):
        ev.evaluate_prdc({}, np.zeros((8, 1, 2)), 8, 4)
    with pytest.raises(AssertionError, match='real samples'):
        ev.evaluate_prdc({}, real[:4], 8, 4)
    with pytest.raises(AssertionError, match='positive'):
        ev.evaluate_prdc({}, real, 0, 4)
    with pytest.raises(AssertionError, match='samples given'):
        ev.evaluate_prdc({}, real, 8, 4, samples=np.zeros((7, 1, 2), np.float32))
    with pytest.raises(AssertionError, match='nearest_k'):
        ev.evaluate_prdc({}, real, 8, 4, nearest_k=8, samples=np.zeros((8, 1, 2), np.float32))
    with pytest.raises(AssertionError, match='callable'):
        ev.evaluate_prdc({}, real, 8, 4, nearest_k=3, features='inception', samples=np.zeros((8, 1, 2), np.float32))
    assert all(ev.evals[k] == [] for k in ('wass', 'mmd', 'precision', 'recall', 'density', 'coverage', 'fid', 'f_1_pr', 'f_1_dc', 'fig'))
