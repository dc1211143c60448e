"""PRD precision / recall without a GPU: the fp64 numpy restatement of the reference's _cluster_into_bins (after the fit), compute_prd
and prd_to_max_f_beta_pair held to the reference's own recorded results (fixture family F19), the fixtures themselves, and the
refusals of the C entry points, of the Python functions and of EvaluationManager.evaluate_prd -- all of which happen before anything
touches a device."""
import inspect

import numpy as np
import pytest
import torch

from conftest import golden
import dlpm_amd
from dlpm_amd import _lib, metrics
from metric_helpers import buffers

DIRECT = ['toy500_k20', 'toy3000_k100', 'heavy2000_k20', 'same400_k20', 'disjoint300_k20', 'k7_n64', 'd3', 'd16']   # D <= 16
TILED = ['d17', 'd48', 'd192']                                                                                   # D > 16
CASES = DIRECT + TILED
KEYS = {'x', 'y', 'centers64', 'labels', 'inertia', 'eval_bins', 'ref_bins', 'precision', 'recall', 'f_pair', 'min_margin', 'fb_calls',
        'ref_seconds', 'num_clusters', 'num_angles'}


def case(name):
    return golden('f19_prd_' + name)


def np_labels(x, y, centers):
    """fp64 argmin_k sum_d (p - c_k)^2 over p = [x; y] per run (lowest index on ties), and the minimum itself."""
    p = np.concatenate([np.asarray(x, np.float64).reshape(len(x), -1), np.asarray(y, np.float64).reshape(len(y), -1)])
    labels, dist = [], []
    for c in np.asarray(centers, np.float64):
        d2 = ((p[:, None, :] - c[None, :, :]) ** 2).sum(2)
        labels.append(d2.argmin(1))
        dist.append(d2.min(1))
    return np.stack(labels), np.stack(dist)


def np_bins(labels, n1, K):
    """prd_score.py:129-135 as counts: [R, K] for the eval points (the first n1) and for the ref points."""
    return (np.stack([np.bincount(l[:n1], minlength=K) for l in labels]), np.stack([np.bincount(l[n1:], minlength=K) for l in labels]))


def np_curve(eval_bins, ref_bins, n1, n2, num_angles, epsilon=1e-10):
    """prd_score.py:84-105 per run and :189-190 over the runs, on counts normalised by each set's own size.
    Returns (precision, recall, largest value before clipping)."""
    slopes = np.tan(np.linspace(epsilon, np.pi / 2 - epsilon, num=num_angles))
    ps, rs, raw = [], [], 0.0
    for e, r in zip(np.asarray(eval_bins, np.float64) / n1, np.asarray(ref_bins, np.float64) / n2):
        precision = np.minimum(r[None, :] * slopes[:, None], e[None, :]).sum(axis=1)
        recall = precision / slopes
        raw = max(raw, precision.max(), recall.max())
        ps.append(np.clip(precision, 0, 1))
        rs.append(np.clip(recall, 0, 1))
    return np.mean(ps, axis=0), np.mean(rs, axis=0), raw


def np_f_pair(precision, recall, beta=8):
    """prd_score.py:226-227, :260-262."""
    def f(b):
        return np.max((1 + b ** 2) * (precision * recall) / ((b ** 2 * precision) + recall + 1e-10))
    return np.array([f(beta), f(1 / beta)])


@pytest.mark.parametrize('name', CASES)
def test_restatement_equals_the_reference(name):
    f = case(name)
    n1, K, A = len(f['x']), int(f['num_clusters']), int(f['num_angles'])
    labels, dist = np_labels(f['x'], f['y'], f['centers64'])
    assert np.array_equal(labels, f['labels'])
    eb, rb = np_bins(labels, n1, K)
    assert np.array_equal(eb, f['eval_bins']) and np.array_equal(rb, f['ref_bins'])
    p, r, raw = np_curve(eb, rb, n1, len(f['y']), A)
    assert np.abs(p - f['precision']).max() <= 1e-12 and np.abs(r - f['recall']).max() <= 1e-12
    assert np.abs(np_f_pair(p, r) - f['f_pair']).max() <= 1e-12 and raw <= 1.001
    assert np.abs(np.array(metrics.prd_to_max_f_beta_pair(f['precision'], f['recall'])) - f['f_pair']).max() <= 1e-12
    assert np.abs(metrics.compute_f_beta(f['precision'], f['recall']) - f['f_pair']).max() <= 1e-12
    assert np.abs(dist.sum(1) - f['inertia']).max() <= 1e-9 * f['inertia'].max()


def test_fixtures_are_small_and_complete():
    for name in CASES:
        f = case(name)
        assert set(f.files) >= KEYS, name
        n, D = f['x'].shape
        R, K, A = f['centers64'].shape[0], int(f['num_clusters']), int(f['num_angles'])
        assert n <= 3000 and f['y'].shape == (n, D) and (D > 16) == (name in TILED)
        assert f['x'].dtype == np.float32 and f['y'].dtype == np.float32 and f['centers64'].dtype == np.float64
        assert f['centers64'].shape == (R, K, D) and f['labels'].shape == (R, 2 * n) and f['labels'].dtype == np.uint8
        assert f['eval_bins'].shape == (R, K) and f['ref_bins'].shape == (R, K) and f['inertia'].shape == (R,)
        assert (f['eval_bins'].sum(1) == n).all() and (f['ref_bins'].sum(1) == n).all()
        assert f['precision'].shape == (A,) and f['recall'].shape == (A,) and f['precision'].dtype == np.float64
        assert f['fb_calls'].shape == (8, 2) and f['f_pair'].shape == (2,)
        p = np.concatenate([f['x'], f['y']]).astype(np.float64)
        assert float(f['min_margin']) >= 1e-10 * (p ** 2).sum(1).max() and float(f['ref_seconds']) > 0
    assert case('k7_n64')['centers64'].shape[:2] == (3, 7) and int(case('k7_n64')['num_angles']) == 11
    heavy = np.concatenate([case('heavy2000_k20')['x'], case('heavy2000_k20')['y']])
    assert np.abs(heavy).max() == 6.0 and len(np.unique(heavy, axis=0)) < len(heavy)        # duplicates on the clamp boundary
    assert np.array_equal(case('same400_k20')['x'], case('same400_k20')['y'])


def test_workspace_bytes_refusals_and_growth():
    L = _lib.lib()
    ws = L.dlpm_prd_workspace_bytes
    for args, word in [((0, 4, 2, 2, 1, 1), 'bad shape'), ((4, 0, 2, 2, 1, 1), 'bad shape'), ((4, 4, 0, 2, 1, 1), 'bad shape'),
                       ((4, 4, 4097, 2, 1, 1), 'D must be'), ((300, 300, 2, 0, 1, 1), 'num_clusters'),
                       ((300, 300, 2, 257, 1, 1), 'num_clusters'), ((4, 4, 2, 9, 1, 1), 'num_clusters'), ((4, 4, 2, 2, 0, 1), 'num_runs'),
                       ((4, 4, 2, 2, 1, 0), 'n_init')]:
        assert ws(*args) == -1, args
        assert word.encode() in L.dlpm_last_error(), (args, L.dlpm_last_error())
    base = ws(500, 500, 2, 20, 4, 3)
    assert base > 0
    assert ws(500, 500, 2, 40, 4, 3) > base and ws(500, 500, 2, 20, 5, 3) > base and ws(500, 500, 2, 20, 4, 4) > base
    assert ws(500, 500, 192, 20, 4, 3) > base and ws(500, 500, 4096, 256, 1, 1) > 0
    big = ws(3000000, 3000000, 2, 20, 10, 10)                 # 100 instances x 6e6 points: labels and distances alone pass 2^31 bytes
    assert big >= 100 * 6000000 * 9 > 2 ** 31


def test_c_entry_points_refuse_before_any_launch():
    """No GPU here: every one of these returns before a kernel is launched (the pointers are host addresses, never followed)."""
    L = _lib.lib()
    buf, base = buffers()
    P = [base + 4096 * i for i in range(12)]
    need = L.dlpm_prd_workspace_bytes(8, 8, 2, 3, 2, 2)
    good = dict(x=P[0], n1=8, y=P[1], n2=8, D=2, K=3, R=2, n_init=2, max_iter=5, tol=1e-4, seed=1, first=0, ws=P[2], wsb=need, cen=P[3],
                lab=P[4], cnt=P[5], ine=P[6], it=P[7], conv=P[8], A=11, eps=1e-10, beta=8.0, out=P[9])

    def kmeans(**o):
        a = dict(good, **o)
        return L.dlpm_kmeans_f32(a['x'], a['n1'], a['y'], a['n2'], a['D'], a['K'], a['R'], a['n_init'], a['max_iter'], a['tol'], a['seed'],
                                 a['first'], a['ws'], a['wsb'], a['cen'], a['lab'], a['cnt'], a['ine'], a['it'], a['conv'], None)

    def hist(**o):
        a = dict(good, **o)
        return L.dlpm_prd_histograms_f32(a['x'], a['n1'], a['y'], a['n2'], a['D'], a['K'], a['R'], a['cen'], a['ws'], a['wsb'], a['lab'],
                                         a['cnt'], a['ine'], None)

    def curve(**o):
        a = dict(good, **o)
        return L.dlpm_prd_curve_f64(a['cnt'], a['n1'], a['n2'], a['K'], a['R'], a['A'], a['eps'], a['beta'], a['ws'], a['wsb'], a['out'], None)

    def prd(**o):
        a = dict(good, **o)
        return L.dlpm_prd_f32(a['x'], a['n1'], a['y'], a['n2'], a['D'], a['K'], a['R'], a['n_init'], a['max_iter'], a['tol'], a['seed'],
                              a['A'], a['eps'], a['beta'], a['ws'], a['wsb'], a['cen'], a['lab'], a['cnt'], a['out'], None)

    shape = [(dict(n1=0), 'bad shape'), (dict(n2=0), 'bad shape'), (dict(K=0), 'num_clusters'), (dict(K=257), 'num_clusters'),
             (dict(K=17), 'num_clusters'), (dict(R=0), 'num_runs')]
    width = [(dict(D=0), 'bad shape'), (dict(D=4097), 'D must be')]
    fit = [(dict(n_init=0), 'n_init'), (dict(max_iter=0), 'max_iter'), (dict(tol=-1.0), 'tol')]
    angles = [(dict(A=2), 'num_angles'), (dict(A=1000001), 'num_angles'), (dict(eps=0.0), 'epsilon'), (dict(eps=0.1), 'epsilon'),
              (dict(beta=0.0), 'beta'), (dict(beta=-8.0), 'beta')]

    def nulls(*names):
        return [({k: None}, 'null') for k in names]
    for fn, cases in [(kmeans, shape + width + fit + [(dict(first=-1), 'first_run')] +
                       nulls('x', 'y', 'ws', 'cen', 'lab', 'cnt', 'ine', 'it', 'conv')),
                      (hist, shape + width + nulls('x', 'y', 'cen', 'ws', 'lab', 'cnt', 'ine')),
                      (curve, shape + angles + nulls('cnt', 'ws', 'out')),
                      (prd, shape + width + fit + angles + nulls('x', 'y', 'ws', 'out'))]:
        for over, word in cases:
            with pytest.raises(ValueError, match=word):
                _lib.check(fn(**over))
        with pytest.raises(_lib.DlpmError, match='workspace'):
            _lib.check(fn(wsb=7))
        assert fn(wsb=7) == -5                  # DLPM_ERR_NOMEM
    for fn in (kmeans, prd):
        assert fn(wsb=need - 1) == -5


def test_python_refusals():
    x = torch.zeros(40, 2)
    for bad, word in [((x.double(), x), 'float32'), ((x, x.to(torch.float16)), 'float32'), ((x, torch.zeros(40, 3)), 'values'),
                      ((torch.zeros(0, 2), x), 'at least one point'), ((np.zeros((40, 2), np.int64), x), 'float32'),
                      ((torch.zeros(4, 4097), torch.zeros(4, 4097)), 'at most 4096')]:
        with pytest.raises(AssertionError, match=word):
            metrics.prd(*bad)
    for kw, word in [(dict(num_clusters=0), 'num_clusters'), (dict(num_clusters=257), 'num_clusters'), (dict(num_clusters=81), 'num_clusters'),
                     (dict(num_clusters=2.5), 'num_clusters'), (dict(num_runs=0), 'num_runs'), (dict(n_init=0), 'n_init'),
                     (dict(max_iter=0), 'max_iter'), (dict(centers=np.zeros((2, 20, 2), np.float32)), 'float64'),
                     (dict(centers=np.zeros((20, 2))), 'float64')]:
        with pytest.raises(AssertionError, match=word):
            metrics.prd(x, x, **kw)
    for kw, word in [(dict(num_angles=2), 'num_angles'), (dict(num_angles=10 ** 6 + 1), 'num_angles')]:
        with pytest.raises(ValueError, match=word):            # the reference raises ValueError on these (prd_score.py:78-81)
            metrics.prd(x, x, **kw)
    with pytest.raises(ValueError, match='beta'):
        metrics.prd_device(x, x, beta=0)
    with pytest.raises(ValueError, match='epsilon'):
        metrics.prd_device(x, x, epsilon=0.1)
    with pytest.raises(ValueError, match='not equal'):
        metrics.compute_prd_from_embedding(torch.zeros(64, 2), torch.zeros(80, 2))
    for args, kw, word in [((x.double(), 3), {}, 'float32'), ((x[:1], 1), {}, 'two points'), ((x, 41), {}, 'num_clusters'),
                           ((x, 3), dict(tol=-1), 'tol'), ((x, 3), dict(first_run=-1), 'first_run'), ((x, 3), dict(runs=0), 'num_runs')]:
        with pytest.raises(AssertionError, match=word):
            metrics.kmeans(*args, **kw)
    for bad in [(np.array([0.5, 1.5]), np.array([0.5, 0.5])), (np.array([0.5, 0.5]), np.array([-0.1, 0.5]))]:
        with pytest.raises(ValueError, match=r'\[0, 1\]'):
            metrics.prd_to_max_f_beta_pair(*bad)
    with pytest.raises(ValueError, match='beta'):
        metrics.prd_to_max_f_beta_pair(np.array([0.5]), np.array([0.5]), beta=0)


def test_drop_in_signatures():
    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(metrics.compute_prd_from_embedding) == [('eval_data', E), ('ref_data', E), ('num_clusters', 20), ('num_angles', 1001),
                                                       ('num_runs', 10), ('enforce_balance', True)]
    assert sig(metrics.compute_precision_recall_curve) == [('data', E), ('gen_samples', E), ('num_angles', 201), ('num_clusters', 20)]
    assert sig(metrics.prd_to_max_f_beta_pair) == [('precision', E), ('recall', E), ('beta', 8)]
    assert sig(metrics.compute_f_beta) == [('prec', E), ('rec', E)]
    assert sig(metrics.prd)[:10] == [('eval_data', E), ('ref_data', E), ('num_clusters', 20), ('num_angles', 1001), ('num_runs', 10),
                                     ('n_init', 10), ('max_iter', 100), ('seed', 0), ('centers', None), ('return_parts', False)]
    assert sig(metrics.kmeans)[:6] == [('points', E), ('K', E), ('n_init', 10), ('max_iter', 100), ('seed', 0), ('runs', 1)]
    assert sig(dlpm_amd.EvaluationManager.evaluate_prd)[1:10] == [
        ('models', E), ('real_data', E), ('data_to_generate', E), ('batch_size', E), ('class_labels', None), ('num_angles', 201),
        ('num_clusters', None), ('seed', 0), ('samples', None)]
    for name in ('kmeans', 'prd', 'compute_prd_from_embedding', 'compute_precision_recall_curve', 'prd_to_max_f_beta_pair',
                 'compute_f_beta'):
        assert getattr(dlpm_amd, name) is getattr(metrics, name)
    assert 'REAL' in metrics.compute_precision_recall_curve.__doc__


def test_evaluate_prd_refusals_leave_evals_untouched():
    ev = dlpm_amd.EvaluationManager(None, None, None, verbose=False)
    with pytest.raises(AssertionError, match='float32'):
        ev.evaluate_prd({}, np.zeros((8, 1, 2)), 8, 4)
    with pytest.raises(AssertionError, match='real samples'):
        ev.evaluate_prd({}, np.zeros((4, 1, 2), np.float32), 8, 4)
    with pytest.raises(AssertionError, match='positive'):
        ev.evaluate_prd({}, np.zeros((4, 1, 2), np.float32), 0, 4)
    with pytest.raises(AssertionError, match='samples given'):
        ev.evaluate_prd({}, np.zeros((8, 1, 2), np.float32), 8, 4, samples=np.zeros((7, 1, 2), np.float32))
    with pytest.raises(AssertionError, match='float32 samples'):
        ev.evaluate_prd({}, np.zeros((8, 1, 2), np.float32), 8, 4, samples=np.zeros((8, 1, 2)))
    with pytest.raises(AssertionError, match='values'):
        ev.evaluate_prd({}, np.zeros((8, 1, 2), np.float32), 8, 4, samples=np.zeros((8, 1, 3), np.float32))
    assert ev.evals['precision'] == [] and ev.evals['recall'] == [] and ev.evals['f_1_pr'] == []
