"""The exact W1 without a GPU: the host mirror of tests/w1_refs.py (fp64 cost, quantisation, integer auction) against its oracles on
the whole case table of tests/test_gpu_w1.py -- scipy's linear_sum_assignment on the integer matrix (an integer EQUALITY) and on the
fp64 costs (the two-sided bound), brute force over all permutations for n <= 7 -- and against the fixture family
tests/golden/f26_w1.npz; the ABI of include/dlpm_amd_w1.h; every refusal of the C entry points on a host buffer (a refusal comes
before anything touches it) and of the Python functions."""
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import dlpm_amd
from dlpm_amd import _lib, metrics
from metric_helpers import buffers
import w1_refs as R

ROOT = R.ROOT
ERR_ARG, ERR_NOMEM = -1, -5


# ------------------------------------------------------------------------------------------ the mirror against its oracles
@pytest.mark.parametrize('name,ground', R.PAIRS)
def test_mirror_is_exactly_optimal(name, ground):
    m, f = R.mirror(name, ground), R.fixture()
    n = R.CASES[name][0]
    assert sorted(m['perm'].tolist()) == list(range(n))                                   # a permutation
    assert m['rounds'] <= R.MAX_TABLE_ROUNDS
    assert 0 <= m['q'].min() and m['q'].max() <= 1 << 24 and (m['cmax'] == 0 or m['q'].max() >= 1 << 23)
    q_opt = int(R.scipy_optimum(m['q'])[0].sum())
    assert m['integer_cost'] == q_opt == int(f['%s.%s.q_opt' % (name, ground)])           # integer equality
    terms, _ = R.scipy_optimum(m['c'])
    w_scipy = math.fsum(terms.tolist()) / n
    assert w_scipy == float(f['%s.%s.w_opt' % (name, ground)])
    assert 0 <= m['w'] - w_scipy <= R.w_bound(m['e'], n, m['cmax'])
    assert (m['x'] == f[name + '.x']).all() and (m['y'] == f[name + '.y']).all()
    if n <= 7:
        assert R.brute_optimum(m['q']) == m['integer_cost'] == int(f['%s.%s.q_brute' % (name, ground)])
        w_brute = R.brute_optimum(m['c']) / n
        assert w_brute == float(f['%s.%s.w_brute' % (name, ground)])
        assert 0 <= m['w'] - w_brute <= R.w_bound(m['e'], n, m['cmax'])


def test_the_table_covers_what_it_names():
    pairs = set(R.PAIRS)
    assert {R.CASES[n][0] for n, _ in pairs} == {1, 2, 3, 17, 63, 64, 65, 257, 512}
    for n in (1, 2, 3, 17, 63, 64, 65, 257):         # the whole cross product, both grounds
        assert {(R.CASES[c][1], g) for c, g in pairs if R.CASES[c][0] == n} >= {(D, g) for D in (1, 2, 3, 16, 17, 40) for g in R.GROUNDS}
    assert pairs == {(c, g) for c in R.CASES for g in R.GROUNDS} and len(R.PAIRS) == len(pairs)
    assert {(R.CASES[c][1], g) for c, g in pairs if R.CASES[c][0] == 512} == {(2, g) for g in R.GROUNDS}
    # every instantiation of the register form (rows padded to 2, 4, 8, 16 values) and the LDS form, under both grounds
    pad = lambda D: 2 if D <= 2 else 4 if D <= 4 else 8 if D <= 8 else 16 if D <= 16 else 0
    assert {(pad(R.CASES[c][1]), g) for c, g in pairs} == {(p, g) for p in (2, 4, 8, 16, 0) for g in R.GROUNDS}


def test_cost_is_the_reference_definition():
    """l1_mean is compute_mean_lploss(a, b, lploss=1) of the reference between single points: mean |a - b| (** 1 changes nothing)."""
    g = np.random.default_rng(5)
    x, y = g.standard_normal((5, 3)).astype(np.float32), g.standard_normal((5, 3)).astype(np.float32)
    c, ce = R.costs(x, y, 'l1_mean'), R.costs(x, y, 'euclidean')
    for i in range(5):
        for j in range(5):
            d = x[i].astype(np.float64) - y[j].astype(np.float64)
            assert c[i, j] == pytest.approx(np.abs(d).mean(), rel=1e-15)
            assert ce[i, j] == pytest.approx(np.sqrt((d * d).sum()), rel=1e-15)


def test_mirror_on_ties_and_degenerate_sets():
    lattice = np.array([[a, b] for a in range(4) for b in range(4)], np.float32)
    m = R.mirror_of(lattice, lattice[::-1].copy(), 'l1_mean')
    assert m['w'] == 0.0 and m['integer_cost'] == 0
    same = np.full((9, 2), 0.25, np.float32)
    m = R.mirror_of(same, same, 'euclidean')
    assert (m['cmax'], m['e'], m['phases'], m['rounds'], m['w']) == (0.0, 0, 1, 9, 0.0)
    one = R.mirror_of(np.ones((1, 3), np.float32), np.zeros((1, 3), np.float32), 'l1_mean')
    assert one['w'] == 1.0 and one['perm'].tolist() == [0] and one['integer_cost'] == 1 << 23


# ------------------------------------------------------------------------------------------ ABI
def test_header_says_the_call_can_be_captured():
    header = open(os.path.join(ROOT, 'include', 'dlpm_amd_w1.h')).read()
    assert 'graph' in header.lower()


def test_python_surface():
    def sig(f):
        return [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    for name in ('w1', 'w1_device', 'compute_w1_distance'):
        assert getattr(dlpm_amd, name) is getattr(metrics, name)
    assert sig(metrics.w1_device) == [('first', E), ('second', E), ('ground', 'l1_mean'), ('max_rounds', None), ('tail_threshold', None)]
    assert sig(metrics.w1) == [('first', E), ('second', E), ('ground', 'l1_mean'), ('return_parts', False)]
    assert sig(metrics.compute_w1_distance) == [('data', E), ('gen_samples', E), ('num_samples', -1)]
    assert sig(dlpm_amd.EvaluationManager.evaluate_w1)[1:] == [
        ('models', E), ('real_data', E), ('data_to_generate', E), ('batch_size', E), ('class_labels', None), ('ground', 'l1_mean'),
        ('samples', None), ('kwargs', E)]
    assert 'graph' in metrics.w1_device.__doc__
    assert metrics.W1_TAIL_THRESHOLD == 4
    for name, ground in R.PAIRS:                     # the default cap is 16 x above every count of the table
        assert metrics.w1_default_max_rounds(R.CASES[name][0]) >= 16 * R.mirror(name, ground)['rounds'], (name, ground)


# ------------------------------------------------------------------------------------------ refusals, before any launch
def test_workspace_bytes_refuses_and_grows():
    ws = _lib.lib().dlpm_w1_workspace_bytes
    for n, D in ((0, 2), (-1, 2), (32769, 2), (4, 0), (4, 4097), (4, -3)):
        assert ws(n, D) == ERR_ARG, (n, D)
    assert 0 < ws(1, 1) <= ws(2, 1) < ws(63, 2) < ws(4096, 2) < ws(32768, 4096)
    assert ws(4096, 2) >= 4096 * 4096 * 4 and ws(4096, 2) % 256 == 0 and ws(7, 1) == ws(7, 4096)


def test_w1_entry_point_refuses_on_a_host_buffer():
    L = _lib.lib()
    buf, base = buffers()
    n, D = 8, 2
    need = L.dlpm_w1_workspace_bytes(n, D)
    assert 0 < need <= 1 << 15
    ok = dict(x=base, y=base + 256, n=n, D=D, ground=0, max_rounds=100, tail=4, ws=base + 1024, wsb=need, perm=base + 512, prices=base + 768,
              out=base + 896)

    def call(**o):
        a = dict(ok, **o)
        return L.dlpm_w1_f32(a['x'], a['y'], a['n'], a['D'], a['ground'], a['max_rounds'], a['tail'], a['ws'], a['wsb'], a['perm'],
                             a['prices'], a['out'], None)
    cases = [(dict(x=None), 'null'), (dict(y=None), 'null'), (dict(ws=None), 'null'), (dict(out=None), 'null'),
             (dict(x=base + 2), 'misaligned'), (dict(y=base + 257), 'misaligned'), (dict(out=base + 900), 'misaligned'),
             (dict(perm=base + 514), 'misaligned'), (dict(prices=base + 772), 'misaligned'), (dict(ws=base + 1032), 'misaligned workspace'),
             (dict(n=0), 'n must be'), (dict(n=-5), 'n must be'), (dict(n=32769), 'n must be'), (dict(D=0), 'D must be'),
             (dict(D=4097), 'D must be'), (dict(ground=2), 'unknown ground'), (dict(ground=-1), 'unknown ground'),
             (dict(max_rounds=0), 'max_rounds'), (dict(max_rounds=-7), 'max_rounds'), (dict(tail=-1), 'tail_threshold')]
    for override, word in cases:
        assert call(**override) == ERR_ARG, override
        assert word.encode() in L.dlpm_last_error(), (override, L.dlpm_last_error())
    assert call(wsb=need - 1) == ERR_NOMEM and b'workspace' in L.dlpm_last_error()
    assert not buf.any()                                              # nothing was touched


def test_python_refusals():
    x = torch.zeros(8, 2)
    for fn in (metrics.w1, metrics.w1_device):
        with pytest.raises(AssertionError, match='equal counts'):
            fn(x, x[:7])
        with pytest.raises(AssertionError, match='float32'):
            fn(x.double(), x)
        with pytest.raises(AssertionError, match='float32'):
            fn(x, x.double())
        with pytest.raises(AssertionError, match='rows hold'):
            fn(x, torch.zeros(8, 3))
        with pytest.raises(ValueError, match='ground'):
            fn(x, x, ground='cityblock')
        with pytest.raises(AssertionError, match='at most 32768 points'):
            fn(torch.zeros(32769, 1), torch.zeros(32769, 1))
        with pytest.raises(AssertionError, match='at most 4096 values'):
            fn(torch.zeros(2, 4097), torch.zeros(2, 4097))
    with pytest.raises(AssertionError, match='max_rounds'):
        metrics.w1_device(x, x, max_rounds=0)
    with pytest.raises(AssertionError, match='tail_threshold'):
        metrics.w1_device(x, x, tail_threshold=-1)
    with pytest.raises(AssertionError, match='num_samples'):
        metrics.compute_w1_distance(x, x, num_samples=9)
    with pytest.raises(AssertionError, match='num_samples'):
        metrics.compute_w1_distance(x, x, num_samples=0)
    with pytest.raises(NotImplementedError, match='DESIGN') as err:
        metrics.compute_wasserstein_distance(x, x, manual_compute=True)
    assert 'metrics.compute_w1_distance' in str(err.value)


def test_evaluation_manager_keys_and_refusals():
    ev = dlpm_amd.EvaluationManager(None, None, None, verbose=False)
    assert 'w1' not in ev.evals
    before = set(ev.evals)
    real = np.zeros((8, 1, 2), np.float32)
    with pytest.raises(ValueError, match='ground'):
        ev.evaluate_w1({}, real, 8, 4, ground='cityblock', samples=real)
    with pytest.raises(AssertionError, match='7 samples given'):
        ev.evaluate_w1({}, real, 8, 4, samples=real[:7])
    with pytest.raises(AssertionError, match='float32 samples'):
        ev.evaluate_w1({}, real, 8, 4, samples=real.astype(np.float64))
    assert set(ev.evals) == before
    ev.evals['w1'] = [0.5]                                             # as after a call
    ev.reset(keep_evals=True)
    assert ev.evals['w1'] == [0.5]
    ev.reset()
    assert set(ev.evals) == before


def test_cli_knows_the_flags():
    from dlpm_amd import cli
    a = cli.build_parser().parse_args(['--config', '2d_data', '--eval_w1', 'dataset', '--w1_ground', 'euclidean', '--generate', '8'])
    assert a.eval_w1 == 'dataset' and a.w1_ground == 'euclidean'
    assert cli.build_parser().parse_args(['--config', '2d_data']).w1_ground == 'l1_mean'
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(['--config', '2d_data', '--w1_ground', 'cityblock'])
    with pytest.raises(SystemExit, match='--generate'):
        cli.main(['--config', '2d_data', '--eval_w1', 'dataset'])


# ------------------------------------------------------------------------------------------ the host program
def test_layout_program_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / 'check_w1_layout')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                           os.path.join(ROOT, 'dlpm_amd', 'csrc'), os.path.join(ROOT, 'tools', 'check_w1_layout.cpp'), '-o', exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith('ok'), out.stdout + out.stderr
    L = _lib.lib()
    totals = dict(re.findall(r'n (\d+): total (\d+)', out.stdout))
    assert {int(n): int(t) for n, t in totals.items()} == {n: L.dlpm_w1_workspace_bytes(n, 2) for n in (1, 2, 63, 4096, 32768)}
