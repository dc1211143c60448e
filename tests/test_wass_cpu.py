"""The Wasserstein figure without a GPU: `np_wass`, a numpy restatement of pyemd.emd_samples whose value is taken from the integer
counts and the fp64 edges in exact rational arithmetic (the oracle of tests/test_gpu_wass.py), held to scipy's 1-D Wasserstein distance
and to the transport LP that pyemd solves; the exports and the C / Python mirrors; and the refusals of the C entry points, of the
Python functions and of EvaluationManager.evaluate_wass -- all of which happen before anything touches a device."""
import inspect
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import dlpm_amd
from dlpm_amd import _lib, metrics
from metric_helpers import buffers



def np_wass(first, second, bins='auto', range=None):
    """pyemd.emd_samples(first, second, bins=bins, range=range) restated.  Bin count and outer edges: np.histogram_bin_edges on the
    pooled fp32 values (numpy's own 'auto' arithmetic on fp32 data); counts: np.histogram of each set, converted to fp64, over
    np.linspace(lo, hi, bins + 1) in fp64; value: sum_i |C1_i / n1' - C2_i / n2'| (c_{i+1} - c_i) over cumulative counts C and bin
    centres c, as a Fraction.  Returns (float(value), parts) with parts = {'exact', 'bins', 'lo', 'hi', 'hist_first', 'hist_second',
    'edges'}."""
    a, b = np.asarray(first, np.float32).ravel(), np.asarray(second, np.float32).ravel()
    pooled = np.concatenate([a, b])
    e = np.histogram_bin_edges(pooled, bins=bins, range=range)
    nb = len(e) - 1
    if range is None:
        lo, hi = float(e[0]), float(e[-1])                 # the fp32 min / max (widened in fp32 when equal), exactly
    else:
        lo, hi = float(range[0]), float(range[1])
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5
    h1, edges = np.histogram(a.astype(np.float64), bins=nb, range=(lo, hi))
    h2, edges2 = np.histogram(b.astype(np.float64), bins=nb, range=(lo, hi))
    assert edges.dtype == np.float64 and np.array_equal(edges, edges2) and edges[0] == lo and edges[-1] == hi
    n1, n2 = int(h1.sum()), int(h2.sum())
    parts = {'bins': nb, 'lo': lo, 'hi': hi, 'hist_first': h1, 'hist_second': h2, 'edges': edges}
    if n1 == 0 or n2 == 0:
        parts['exact'] = None
        return float('nan'), parts
    E = [Fraction(float(v)) for v in edges]
    c1 = c2 = 0
    total = Fraction(0)
    for i in np.arange(nb - 1):
        c1 += int(h1[i])
        c2 += int(h2[i])
        d = abs(c1 * n2 - c2 * n1)
        if d:
            total += d * (E[i + 2] - E[i])
    total = total / (2 * n1 * n2)
    parts['exact'] = total
    return float(total), parts


def value_bound(parts):
    """|device - exact| allowed: every term carries at most two rounded quotients of magnitude <= 1 (and the rounded difference and
    product) times a spacing, summed over bins - 1 terms."""
    return 4 * parts['bins'] * 2.0 ** -53 * (parts['hi'] - parts['lo'])


def sets(seed, n1, n2, D, kind='gauss'):
    g = np.random.default_rng(seed)
    if kind == 'gauss':
        return g.standard_normal((n1, D)).astype(np.float32), (0.7 * g.standard_normal((n2, D)) + 0.4).astype(np.float32)
    return (g.standard_normal((n1, D)).astype(np.float32),
            np.clip(g.standard_cauchy((n2, D)), -20, 20).astype(np.float32))


def mostly_equal(seed, n, D):
    g = np.random.default_rng(seed)
    a, b = g.standard_normal((n, D)) + 1.5, g.standard_normal((n, D)) + 2.0
    return (np.where(g.random((n, D)) < 0.8, 1.5, a).astype(np.float32), np.where(g.random((n, D)) < 0.8, 1.5, b).astype(np.float32))


def zeros_and_duplicates():
    """80 pooled values whose quartile ranks (19, 20 and 59, 60) fall inside runs of duplicates; -0.0, +0.0 and two denormals sit at
    ranks 25..28, away from them (numpy's partition does not order -0.0 against +0.0, the device's key does)."""
    pooled = np.concatenate([np.full(15, -2.0), np.full(10, -0.75), [-0.0, 0.0, -1e-40, 1e-40], np.linspace(0.01, 0.4, 21),
                             np.full(20, 0.5), np.linspace(0.6, 3.0, 10)]).astype(np.float32)
    assert pooled.size == 80
    pooled = pooled[np.random.default_rng(3).permutation(80)]
    return pooled[:40].reshape(20, 2), pooled[40:].reshape(20, 2)


def tight_with_outliers():
    """602 values, nearly all within 0.01 of 0 and one at each of -5 and 5: the Freedman-Diaconis width is tiny against the range, so
    'auto' asks for several thousand bins -- more than there are values."""
    g = np.random.default_rng(31)
    a, b = (0.01 * g.standard_normal((150, 2))).astype(np.float32), (0.01 * g.standard_normal((151, 2)) + 0.002).astype(np.float32)
    a[7, 1], b[9, 0] = -5.0, 5.0
    return a, b


AUTO_CASES = {'gauss_cauchy_39x2': lambda: sets(11, 39, 39, 2, 'cauchy'), 'gauss_300x2': lambda: sets(12, 300, 300, 2),
              'iqr_zero': lambda: mostly_equal(13, 150, 2), 'zeros_duplicates': zeros_and_duplicates,
              'more_bins_than_values': tight_with_outliers}


def auto_ratio(first, second):
    """(hi - lo) / width of numpy's 'auto' rule, evaluated in fp64 from public numpy functions alone."""
    p = np.concatenate([np.ravel(first), np.ravel(second)]).astype(np.float64)
    q75, q25 = np.percentile(p, [75, 25])
    ptp = p.max() - p.min()
    fd, sturges = 2.0 * (q75 - q25) * p.size ** (-1.0 / 3.0), ptp / (np.log2(p.size) + 1.0)
    width = min(fd, sturges) if fd else sturges
    return ptp / width, q75 - q25


@pytest.mark.parametrize('name', sorted(AUTO_CASES))
def test_auto_cases_keep_the_ceiling_away_from_an_integer(name):
    """The precondition of the device's bin-count check: a condition on the inputs, so that the order of fp32 and fp64 evaluation
    cannot flip the ceiling."""
    first, second = AUTO_CASES[name]()
    ratio, iqr = auto_ratio(first, second)
    assert abs(ratio - round(ratio)) >= 1e-3, (name, ratio)
    assert (iqr == 0) == (name == 'iqr_zero')
    assert np_wass(first, second)[1]['bins'] == int(np.ceil(ratio))


def auto_rule_restated(p):
    """numpy 2's 'auto' rule on an fp32 array, operation by operation and dtype by dtype -- the very sequence k_wass_setup / auto_bins
    of wass.hip evaluate on the device: (bins, lo, hi, q75, q25)."""
    f32, f64 = np.float32, np.float64
    m = p.size
    mn, mx = p.min(), p.max()
    lo, hi = mn, mx
    if lo == hi:
        lo, hi = f32(lo - f32(0.5)), f32(hi + f32(0.5))            # np.float32 scalars: the widening runs in fp32
    s = np.sort(p)
    qs = []
    for q in (0.75, 0.25):                                          # [75, 25] / np.float32(100): an int64 array over an fp32 scalar, fp64
        vi = (m - 1) * q                                            # method='linear': get_virtual_index
        prev = math.floor(vi)
        nxt = prev + 1
        g = vi - prev
        if vi >= m - 1:
            prev = nxt = m - 1
        a, b = s[int(prev)], s[int(nxt)]
        d = f32(b - a)                                              # _lerp: b - a in fp32, the products in fp64
        r = f64(a) + f64(d) * g
        if g >= 0.5:
            r = f64(b) - f64(d) * (1.0 - g)
        qs.append(r)
    fd = 2.0 * (qs[0] - qs[1]) * float(m) ** (-1.0 / 3.0)
    sturges = f64(f32(mx - mn)) / (math.log2(m) + 1.0)              # _ptp in fp32 over an fp64
    width = min(fd, sturges) if fd else sturges
    bins = int(math.ceil(f64(f32(hi - lo)) / width)) if width else 1
    return bins, float(lo), float(hi), qs[0], qs[1]


def test_restated_auto_rule_equals_numpy_bit_for_bit():
    """What the device mirrors is what numpy does: bin count, outer edges and both quartiles on 1200 random fp32 sets."""
    g = np.random.default_rng(0)
    for t in np.arange(1200):
        n = int(g.integers(1, 400))
        kind = t % 4
        if kind == 0:
            p = g.standard_normal(n)
        elif kind == 1:
            p = np.clip(g.standard_cauchy(n), -20, 20)
        elif kind == 2:
            p = np.round(g.standard_normal(n) * 2)
        else:
            p = np.where(g.random(n) < 0.6, 1.5, g.standard_normal(n))
        p = p.astype(np.float32)
        e = np.histogram_bin_edges(p, 'auto')
        q75, q25 = np.percentile(p, [75, 25])
        assert auto_rule_restated(p) == (len(e) - 1, float(e[0]), float(e[-1]), q75, q25), (t, n)


CLOSED_FORM = [('gauss_cauchy_39x2', 'auto', None), ('gauss_300x2', 'auto', None), ('iqr_zero', 'auto', None), ('gauss_300x2', 250, None),
               ('gauss_300x2', 40, (-1.0, 1.5))]


@pytest.mark.parametrize('name,bins,rng', CLOSED_FORM)
def test_restatement_equals_scipy(name, bins, rng):
    from scipy.stats import wasserstein_distance
    first, second = AUTO_CASES[name]()
    value, p = np_wass(first, second, bins, rng)
    c = (p['edges'][:-1] + p['edges'][1:]) / 2
    want = wasserstein_distance(c, c, p['hist_first'], p['hist_second'])
    assert abs(value - want) <= 1e-12, (value, want)
    assert value > 0


@pytest.mark.parametrize('name,bins,rng', CLOSED_FORM[1:3] + CLOSED_FORM[4:] + [('gauss_cauchy_39x2', 60, None), ('zeros_duplicates', 'auto', None)])
def test_restatement_equals_the_transport_optimum(name, bins, rng):
    """The problem pyemd solves: min sum_ij f_ij |c_i - c_j| with both marginals as equality constraints."""
    from scipy.optimize import linprog
    first, second = AUTO_CASES[name]()
    value, p = np_wass(first, second, bins, rng)
    nb = p['bins']
    assert nb <= 60
    c = (p['edges'][:-1] + p['edges'][1:]) / 2
    w1, w2 = p['hist_first'] / p['hist_first'].sum(), p['hist_second'] / p['hist_second'].sum()
    cost = np.abs(c[:, None] - c[None, :]).ravel()
    A = np.zeros((2 * nb, nb * nb))
    for i in np.arange(nb):
        A[i, i * nb:(i + 1) * nb] = 1                      # row sums = first marginal
        A[nb + i, i::nb] = 1                               # column sums = second marginal
    res = linprog(cost, A_eq=A, b_eq=np.concatenate([w1, w2]), bounds=(0, None), method='highs')
    assert res.status == 0
    assert abs(res.fun - value) <= 1e-6 * value, (res.fun, value)


def test_one_bin_and_equal_sets_give_zero():
    x = np.full((5, 2), 1.25, np.float32)
    v, p = np_wass(x, x)
    assert v == 0.0 and p['bins'] == 1 and (p['lo'], p['hi']) == (0.75, 1.75)
    a, _ = sets(5, 30, 30, 2)
    assert np_wass(a, a, 17)[0] == 0.0


# ---------------------------------------------------------------- exports and mirrors
def test_exports_and_mirrors():
    for name in ('wass', 'wass_device', 'compute_wasserstein_distance'):
        assert getattr(dlpm_amd, name) is getattr(metrics, name)
    for hook in ('evaluate_wass', 'evaluate_metrics_2d'):
        assert callable(getattr(dlpm_amd.EvaluationManager, hook))


def test_drop_in_signatures():
    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(metrics.compute_wasserstein_distance) == [('data', E), ('gen_samples', E), ('manual_compute', False), ('num_samples', -1),
                                                         ('distance', 'euclidean'), ('normalized', True), ('bins', 'auto'), ('_range', None)]
    assert sig(metrics.wass) == [('first', E), ('second', E), ('bins', 'auto'), ('range', None), ('return_parts', False)]
    assert sig(metrics.wass_device) == [('first', E), ('second', E), ('bins', 'auto'), ('range', None), ('max_bins', 1 << 20)]
    assert sig(dlpm_amd.EvaluationManager.evaluate_wass)[1:] == [
        ('models', E), ('real_data', E), ('data_to_generate', E), ('batch_size', E), ('class_labels', None), ('bins', None),
        ('samples', None), ('kwargs', E)]
    assert sig(dlpm_amd.EvaluationManager.evaluate_metrics_2d)[1:] == [
        ('models', E), ('real_data', E), ('data_to_generate', E), ('batch_size', E), ('class_labels', None), ('seed', 0), ('kwargs', E)]
    assert '[:-1]' in metrics.compute_wasserstein_distance.__doc__


# ---------------------------------------------------------------- refusals
def test_workspace_bytes_refusals_and_growth():
    L = _lib.lib()
    ws = L.dlpm_wass_workspace_bytes
    for args, word in [((0, 4, 2, 16), 'bad shape'), ((4, 0, 2, 16), 'bad shape'), ((4, 4, 0, 16), 'bad shape'), ((4, 4, 2, 0), 'max_bins'),
                       ((4, 4, 2, (1 << 20) + 1), 'max_bins'), ((1 << 20, 4, 1 << 12, 16), 'out of range')]:
        assert ws(*args) == -1, args
        assert word.encode() in L.dlpm_last_error(), (args, L.dlpm_last_error())
    sizes = [ws(500, 400, 2, b) for b in (1, 250, 16384, 16385, 1 << 20)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert sizes[-1] >= 2 * 4 * (1 << 20)
    assert ws(8192, 8192, 3072, 250) == sizes[1]            # streaming: nothing per value


def test_c_entry_point_refuses_before_any_launch():
    """No GPU here: every one of these returns before a kernel is launched (the pointers are host addresses, never followed)."""
    L = _lib.lib()
    buf, base = buffers()
    P = [int(base) + 4096 * i for i in range(6)]
    need = L.dlpm_wass_workspace_bytes(8, 6, 2, 32)
    good = dict(x=P[0], n1=8, y=P[1], n2=6, D=2, bins=16, has=0, lo=0.0, hi=0.0, mb=32, ws=P[2], wsb=need, hist=P[3], out=P[4])

    def call(**o):
        a = dict(good, **o)
        return L.dlpm_wass_f32(a['x'], a['n1'], a['y'], a['n2'], a['D'], a['bins'], a['has'], a['lo'], a['hi'], a['mb'], a['ws'], a['wsb'],
                               a['hist'], a['out'], None)

    for over, word in [(dict(n1=0), 'bad shape'), (dict(n2=0), 'bad shape'), (dict(D=0), 'bad shape'), (dict(n1=-3), 'bad shape'),
                       (dict(mb=0), 'max_bins'), (dict(mb=(1 << 20) + 1), 'max_bins'), (dict(bins=-1), 'bins'),
                       (dict(x=None), 'null'), (dict(y=None), 'null'), (dict(ws=None), 'null'), (dict(out=None), 'null'),
                       (dict(ws=P[2] + 4), 'misaligned'), (dict(x=P[0] + 2), 'misaligned')]:
        with pytest.raises(ValueError, match=word):
            _lib.check(call(**over))
    with pytest.raises(_lib.DlpmError, match='workspace'):
        _lib.check(call(wsb=7))
    assert call(wsb=7) == -5 and call(wsb=need - 1) == -5                  # DLPM_ERR_NOMEM


def test_python_refusals_touch_no_device():
    x = torch.zeros(40, 2)
    for fn in (metrics.wass, metrics.wass_device):
        for bad, word in [((x.double(), x), 'float32'), ((x, x.to(torch.float16)), 'float32'), ((np.zeros((40, 2), np.int64), x), 'float32'),
                          ((x, torch.zeros(40, 3)), 'values'), ((torch.zeros(0, 2), x), 'at least one point'),
                          ((x, torch.zeros(0, 2)), 'at least one point')]:
            with pytest.raises(AssertionError, match=word):
                fn(*bad)
        with pytest.raises(ValueError, match='positive'):
            fn(x, x, bins=0)
        with pytest.raises(ValueError, match='estimator'):
            fn(x, x, bins='fd')
        with pytest.raises(TypeError, match='integer'):
            fn(x, x, bins=2.5)
    with pytest.raises(AssertionError, match='max_bins'):
        metrics.wass_device(x, x, max_bins=0)
    with pytest.raises(AssertionError, match='max_bins'):
        metrics.wass_device(x, x, bins=64, max_bins=32)
    with pytest.raises(NotImplementedError, match='DESIGN'):
        metrics.compute_wasserstein_distance(x, x, manual_compute=True)
    with pytest.raises(NotImplementedError, match='DESIGN'):
        metrics.compute_wasserstein_distance(x, x, distance=lambda a: a)
    with pytest.raises(NotImplementedError, match='DESIGN'):
        metrics.compute_wasserstein_distance(x, x, distance='cityblock')
    with pytest.raises(NotImplementedError, match='DESIGN'):
        metrics.compute_wasserstein_distance(x, x, normalized=False)
    with pytest.raises(AssertionError, match='at least one point'):
        metrics.compute_wasserstein_distance(x[:1], x[:1])               # [:-1] leaves nothing
    with pytest.raises(AssertionError, match='float32'):
        metrics.compute_wasserstein_distance(x.double(), x)


def test_evaluate_wass_refusals_leave_evals_untouched():
    ev = dlpm_amd.EvaluationManager(None, None, None, verbose=False)
    real = np.zeros((8, 1, 2), np.float32)
    for fn in (ev.evaluate_wass, ev.evaluate_metrics_2d):
        with pytest.raises(AssertionError, match='float32'):
            fn({}, np.zeros((8, 1, 2)), 8, 4)
        with pytest.raises(AssertionError, match='real samples'):
            fn({}, real[:4], 8, 4)
        with pytest.raises(AssertionError, match='positive'):
            fn({}, real, 0, 4)
        with pytest.raises(AssertionError, match='at least 2'):
            fn({}, real, 1, 4)
    with pytest.raises(AssertionError, match='samples given'):
        ev.evaluate_wass({}, real, 8, 4, samples=np.zeros((7, 1, 2), np.float32))
    with pytest.raises(AssertionError, match='float32 samples'):
        ev.evaluate_wass({}, real, 8, 4, samples=np.zeros((8, 1, 2)))
    with pytest.raises(AssertionError, match='values'):
        ev.evaluate_wass({}, real, 8, 4, samples=np.zeros((8, 1, 3), np.float32))
    with pytest.raises(AssertionError, match='samples given'):
        ev.evaluate_mmd({}, real, 8, 4, samples=np.zeros((7, 1, 2), np.float32))
    assert all(ev.evals[k] == [] for k in ('wass', 'mmd', 'precision', 'recall', 'density', 'coverage', 'fid', 'f_1_pr', 'f_1_dc', 'fig'))
