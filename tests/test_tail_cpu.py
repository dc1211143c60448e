"""The tail figures without a GPU: the host mirror of tests/tail_refs.py against numpy's own quantiles and against what the Hill
estimator and the upper-quantile MSLE must give on exact Pareto draws; the ABI of include/dlpm_amd_tail.h; every refusal of the C
entry points on a host buffer (a refusal comes before anything touches it) and of the Python functions and the parser."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

import dlpm_amd
from dlpm_amd import _lib, metrics
from metric_helpers import buffers
import tail_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NOMEM = -1, -5
PARETO_ALPHA, PARETO_N = 1.5, 100000


def pareto_pair():
    """Two sets of exact Pareto(1.5) draws U^(-1 / 1.5), fp32, and a light-tailed set 1 + |N(0, 1)|."""
    g = np.random.default_rng(0)
    a = (g.random(PARETO_N) ** (-1.0 / PARETO_ALPHA)).astype(np.float32)
    b = (g.random(PARETO_N) ** (-1.0 / PARETO_ALPHA)).astype(np.float32)
    light = (1.0 + np.abs(g.standard_normal(PARETO_N))).astype(np.float32)
    return a[:, None], b[:, None], light[:, None]


# ------------------------------------------------------------------------------------------ the mirror against its oracles
@pytest.mark.parametrize('n,xi,K', [(2, 0.5, 1), (3, 0.5, 7), (257, 0.95, 100), (1000, 0.999, 4096), (777, 0.5, 777)])
def test_mirror_quantiles_are_numpys_linear_quantiles(n, xi, K):
    s = np.sort(np.abs(np.random.default_rng(n).standard_cauchy(n)).astype(np.float32))
    u = R.levels_of(xi, K)
    assert u[0] == xi and (np.diff(u) > 0).all() and u[-1] < 1.0
    got, want = R.quantiles(s, u), np.quantile(s.astype(np.float64), u, method='linear')
    assert (np.abs(got - want) <= 2 * np.spacing(np.abs(want))).all()
    r0 = R.r0_of(n, xi)
    assert (np.floor(u * (n - 1)) >= r0).all() and 1 <= n - 1 - r0                   # one select at rank r0 serves every level


def test_k_is_not_the_ceiling_of_a_rounded_product():
    assert math.ceil((1 - 0.95) * 100000) == 5001                                     # what the definition avoids
    assert R.r0_of(100000, 0.95) == 94999 and 100000 - 1 - R.r0_of(100000, 0.95) == 5000
    assert R.r0_of(2, 0.5) == 0 and R.r0_of(3, 0.999) == 1 and R.r0_of(3, 0.5) == 1


def test_norm_marginal_is_the_sequential_fp64_sum():
    g = np.random.default_rng(2)
    x = g.standard_normal((5, 3, 4)).astype(np.float32)
    v = R.marginal_values(x, 'norm')
    assert v.dtype == np.float32 and v.shape == (5,)
    for i in range(5):
        acc = 0.0
        for t in x[i].reshape(-1).tolist():
            acc = acc + t * t
        assert v[i] == np.float32(math.sqrt(acc))
    a = R.marginal_values(x, 'abs')
    assert a.shape == (60,) and (a == np.abs(x).reshape(-1)).all()


def test_hill_on_exact_pareto_draws():
    a, b, _ = pareto_pair()
    m = R.mirror(a, b, xi=0.95, levels=100)
    assert m['status'] == 0 and m['k'] == [5000, 5000]
    half_width = 5 * PARETO_ALPHA / math.sqrt(5000)                                   # 0.106: five asymptotic deviations
    print('hill', m['hill'])
    for h in m['hill']:
        assert abs(h - PARETO_ALPHA) <= half_width
    s = np.sort(a.reshape(-1))
    logs = np.log(s[95000:].astype(np.float64)) - np.log(np.float64(s[94999]))
    assert m['hill'][0] == pytest.approx(5000 / math.fsum(logs.tolist()), rel=1e-12)  # the run order changes nothing visible
    assert m['threshold'][0] == s[94999]


def test_msle_separates_a_light_tail_from_a_heavy_one():
    a, b, light = pareto_pair()
    same, other = R.mirror(a, b)['msle'], R.mirror(a, light)['msle']
    print('msle', same, other)
    assert 0 <= same < 0.01 and other > 1
    assert R.mirror(a, a)['msle'] == 0.0


def test_mirror_ties_clamps_and_statuses():
    const = np.full((9, 2), 0.25, np.float32)
    m = R.mirror(const, const[:5], xi=0.5, levels=3)
    assert m['msle'] == 0.0 and m['hill'] == [math.inf, math.inf] and m['status'] == 0
    x = np.abs(np.random.default_rng(4).standard_normal((100, 1))).astype(np.float32)
    z = x.copy()
    z[:97] = 0.0                                                                      # zero beyond the 96th percentile
    m = R.mirror(x, z, marginal='abs')
    assert m['status'] == 2 and math.isnan(m['msle']) and math.isnan(m['hill'][1]) and math.isfinite(m['hill'][0])
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[3, 0] = bad
        m = R.mirror(x, y)
        assert m['status'] == 1 and math.isnan(m['msle']) and all(math.isnan(h) for h in m['hill']) and np.isnan(m['quantiles']).all()


def test_bound_is_the_derived_one():
    m = {'log_max': 3.0, 'mean_abs_d': 0.5, 'msle': 0.25, 'k': [10, 20], 'hill_sum': [5.0, 8.0]}
    d = 2.0 ** -50 * 3.0
    assert R.delta(0.2) == 2.0 ** -50 and R.delta(3.0) == d
    assert R.msle_bound(m) == 2 * 0.5 * d + d * d + 2.0 ** -50 * 0.25
    assert R.hill_rel_bound(m, 1) == 20 * d / 8.0 + 2.0 ** -50


# ------------------------------------------------------------------------------------------ ABI
def test_header_says_the_call_can_be_captured():
    header = open(os.path.join(ROOT, 'include', 'dlpm_amd_tail.h')).read()
    assert 'graph' in header.lower()


def test_python_surface():
    def sig(f):
        return [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    for name in ('tail', 'tail_device', 'msle', 'hill_index'):
        assert getattr(dlpm_amd, name) is getattr(metrics, name)
    assert sig(metrics.tail_device) == [('first', E), ('second', E), ('xi', 0.95), ('levels', 100), ('marginal', 'norm')]
    assert sig(metrics.tail) == [('first', E), ('second', E), ('xi', 0.95), ('levels', 100), ('marginal', 'norm'), ('return_parts', False)]
    assert sig(metrics.msle) == [('real', E), ('gen', E), ('xi', 0.95), ('levels', 100), ('marginal', 'norm')]
    assert sig(metrics.hill_index) == [('x', E), ('xi', 0.95), ('marginal', 'norm')]
    assert sig(dlpm_amd.EvaluationManager.evaluate_tail)[1:] == [
        ('models', E), ('real_data', E), ('data_to_generate', E), ('batch_size', E), ('class_labels', None), ('xi', 0.95), ('levels', 100),
        ('marginal', 'norm'), ('samples', None), ('kwargs', E)]
    assert 'graph' in metrics.tail_device.__doc__
    for doc in (metrics.tail.__doc__, dlpm_amd.EvaluationManager.evaluate_tail.__doc__):
        assert 'clamp' in doc and 'quantile_cutoff' in doc and '+inf' in doc
    assert 'batch_size' in dlpm_amd.EvaluationManager.evaluate_tail.__doc__


# ------------------------------------------------------------------------------------------ refusals, before any launch
def test_workspace_bytes_refuses_and_grows():
    ws = _lib.lib().dlpm_tail_workspace_bytes
    bad = [(1, 2, 2, 0, 0.95, 100), (2, 1, 2, 0, 0.95, 100), (0, 5, 2, 0, 0.95, 100), (5, -3, 2, 0, 0.95, 100), (5, 5, 0, 0, 0.95, 100),
           (1 << 30, 5, 2, 0, 0.95, 100), (5, 1 << 30, 2, 1, 0.95, 100), (5, 5, 2, 2, 0.95, 100), (5, 5, 2, -1, 0.95, 100),
           (5, 5, 2, 0, 0.4999, 100), (5, 5, 2, 0, 1.0, 100), (5, 5, 2, 0, 1.5, 100), (5, 5, 2, 0, math.nan, 100), (5, 5, 2, 0, 0.95, 0),
           (5, 5, 2, 0, 0.95, -4), (5, 5, 2, 0, 0.95, 65537)]
    for args in bad:
        assert ws(*args) == ERR_ARG, args
    assert ws((1 << 31) - 1, 2, 1, 0, 0.5, 1) > 0                                      # the largest set that is taken
    assert 0 < ws(2, 2, 1, 0, 0.5, 1) <= ws(2, 3, 1, 0, 0.5, 1) < ws(100003, 65537, 2, 0, 0.95, 100) < ws(100003, 65537, 2, 1, 0.95, 100)
    assert ws(1000, 1000, 2, 0, 0.95, 100) < ws(1000, 1000, 2, 0, 0.5, 100)           # the tail buffers are sized from xi
    assert ws(1000, 1000, 2, 0, 0.95, 100) < ws(1000, 1000, 2, 0, 0.95, 65536)
    assert ws(1000, 777, 2, 0, 0.95, 100) % 256 == 0 and ws(1000, 777, 2, 0, 0.95, 100) == ws(1000, 777, 17, 0, 0.95, 100)
    # the keys of both marginals and two buffers of k = N - 1 - r0 keys a set, no more than O(levels) beside them
    n, k = 1000000, 1000000 - 1 - R.r0_of(1000000, 0.95)
    runs = -(-k // 2048)                                                              # the radix sort's counters: 2 x 256 per run
    assert 4 * (2 * n + 4 * k) <= ws(n, n, 2, 0, 0.95, 100) <= 4 * (2 * n + 4 * k + 512 * runs) + 32 * 256 + 24 * 100


def test_tail_entry_point_refuses_on_a_host_buffer():
    L = _lib.lib()
    buf, base = buffers()
    n1, n2, D = 8, 9, 2
    need = L.dlpm_tail_workspace_bytes(n1, n2, D, 0, 0.95, 10)
    assert 0 < need <= 1 << 14
    ok = dict(x=base, n1=n1, y=base + 256, n2=n2, D=D, marginal=0, xi=0.95, levels=10, ws=base + 2048, wsb=need, q=base + 1024,
              out=base + 1536)

    def call(**o):
        a = dict(ok, **o)
        return L.dlpm_tail_f32(a['x'], a['n1'], a['y'], a['n2'], a['D'], a['marginal'], a['xi'], a['levels'], a['ws'], a['wsb'], a['q'],
                               a['out'], None)
    cases = [(dict(x=None), 'null'), (dict(y=None), 'null'), (dict(ws=None), 'null'), (dict(out=None), 'null'),
             (dict(x=base + 2), 'misaligned'), (dict(y=base + 257), 'misaligned'), (dict(out=base + 1540), 'misaligned'),
             (dict(q=base + 1028), 'misaligned'), (dict(ws=base + 2056), 'misaligned workspace'),
             (dict(n1=1), 'bad shape'), (dict(n2=1), 'bad shape'), (dict(n1=0), 'bad shape'), (dict(n2=-2), 'bad shape'), (dict(D=0), 'bad shape'),
             (dict(n1=1 << 31), 'out of range'), (dict(n2=1 << 30, D=2), 'out of range'),
             (dict(marginal=2), 'unknown marginal'), (dict(marginal=-1), 'unknown marginal'),
             (dict(xi=0.49), 'xi must be'), (dict(xi=1.0), 'xi must be'), (dict(xi=math.nan), 'xi must be'), (dict(xi=-0.95), 'xi must be'),
             (dict(levels=0), 'levels must be'), (dict(levels=-1), 'levels must be'), (dict(levels=65537), 'levels must be')]
    for override, word in cases:
        assert call(**override) == ERR_ARG, override
        assert word.encode() in L.dlpm_last_error(), (override, L.dlpm_last_error())
    assert call(wsb=need - 1) == ERR_NOMEM and b'workspace' in L.dlpm_last_error()
    assert call(wsb=0) == ERR_NOMEM
    assert call(levels=65536) == ERR_NOMEM and call(n1=4096) == ERR_NOMEM              # sized for the arguments of the call
    assert not buf.any()                                                               # nothing was touched


def test_python_refusals():
    x = torch.zeros(8, 2)
    for fn in (metrics.tail, metrics.tail_device, metrics.msle):
        with pytest.raises(ValueError, match='marginal'):
            fn(x, x, marginal='max')
        with pytest.raises(AssertionError, match=r'xi must be in \[0.5, 1\)'):
            fn(x, x, xi=1)
        with pytest.raises(AssertionError, match='xi must be'):
            fn(x, x, xi=0.3)
        with pytest.raises(AssertionError, match=r'levels must be in \[1, 65536\]'):
            fn(x, x, levels=0)
        with pytest.raises(AssertionError, match='levels must be'):
            fn(x, x, levels=65537)
        with pytest.raises(AssertionError, match='levels must be'):
            fn(x, x, levels=2.5)
        with pytest.raises(AssertionError, match='float32'):
            fn(x.double(), x)
        with pytest.raises(AssertionError, match='rows hold'):
            fn(x, torch.zeros(8, 3))
        with pytest.raises(AssertionError, match='at least 2 samples'):
            fn(x, x[:1])
    with pytest.raises(ValueError, match='marginal'):
        metrics.hill_index(x, marginal='max')
    with pytest.raises(AssertionError, match='xi must be'):
        metrics.hill_index(x, xi=1.0)


def test_evaluation_manager_refusals_leave_the_keys_alone():
    ev = dlpm_amd.EvaluationManager(None, None, None, verbose=False)
    before = set(ev.evals)
    assert not {'msle', 'tail_index_real', 'tail_index_gen'} & before
    real = np.zeros((8, 1, 2), np.float32)
    with pytest.raises(ValueError, match='marginal'):
        ev.evaluate_tail({}, real, 8, 4, marginal='max', samples=real)
    with pytest.raises(AssertionError, match='xi must be'):
        ev.evaluate_tail({}, real, 8, 4, xi=1.0, samples=real)
    with pytest.raises(AssertionError, match='levels must be'):
        ev.evaluate_tail({}, real, 8, 4, levels=0, samples=real)
    with pytest.raises(AssertionError, match='7 samples given'):
        ev.evaluate_tail({}, real, 8, 4, samples=real[:7])
    with pytest.raises(AssertionError, match='float32 samples'):
        ev.evaluate_tail({}, real, 8, 4, samples=real.astype(np.float64))
    assert set(ev.evals) == before


def test_cli_knows_the_flags():
    from dlpm_amd import cli
    a = cli.build_parser().parse_args(['--config', '2d_data', '--eval_tail', 'dataset', '--tail_xi', '0.9', '--tail_levels', '50',
                                       '--tail_marginal', 'abs', '--generate', '8'])
    assert (a.eval_tail, a.tail_xi, a.tail_levels, a.tail_marginal) == ('dataset', 0.9, 50, 'abs')
    d = cli.build_parser().parse_args(['--config', '2d_data'])
    assert (d.eval_tail, d.tail_xi, d.tail_levels, d.tail_marginal) == (None, 0.95, 100, 'norm')
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(['--config', '2d_data', '--tail_marginal', 'max'])
    with pytest.raises(SystemExit, match='--eval_tail needs --generate'):
        cli.main(['--config', '2d_data', '--eval_tail', 'dataset'])
    with pytest.raises(SystemExit, match='--eval_tail cannot be combined'):
        cli.main(['--config', '2d_data', '--eval_tail', 'dataset', '--generate', '8', '--gen_data_path', 'x'])
    assert '--eval_tail' in cli.__doc__ and 'tail msle <v> index real <a> generated <b> xi <x>' in ' '.join(cli.__doc__.split())
