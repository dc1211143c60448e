"""Device PRD precision / recall on the MI355X against the reference's recorded results (fixture family F19): histograms and curve of
given centres (exact labels), the library's own lockstep k-means (fixed-point, inertia and independence properties), statistical
parity with the reference's own run-to-run spread at full defaults, reproducibility, graph capture, and
EvaluationManager.evaluate_prd / the CLI end to end.  Every test prints the figures it measured before it asserts."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from dlpm_amd import metrics
from conftest import GOLDEN
from metric_helpers import managers, real_toy, toy
from test_prd_cpu import CASES, case, np_bins, np_curve, np_f_pair, np_labels

pytestmark = pytest.mark.gpu
DEV = 'cuda'
OWN = ['toy500_k20', 'heavy2000_k20', 'd17', 'k7_n64']
PARITY = ['toy500_k20', 'toy3000_k100', 'heavy2000_k20', 'same400_k20']


def tensors(f):
    return torch.from_numpy(f['x']), torch.from_numpy(f['y'])


# ---------------------------------------------------------------- 1. given centres: the reference's _cluster_into_bins + compute_prd
@pytest.mark.parametrize('name', CASES)
def test_given_centres_reproduce_labels_bins_and_curve(name):
    f = case(name)
    x, y = tensors(f)
    A = int(f['num_angles'])
    p, r, parts = metrics.prd(x, y, num_angles=A, centers=f['centers64'], return_parts=True)
    wrong = int((parts['labels'] != f['labels']).sum())
    dp, dr = np.abs(p - f['precision']).max(), np.abs(r - f['recall']).max()
    df = np.abs(np.array(parts['f_beta']) - f['f_pair']).max()
    print('\n%s: %d labels differ of %d  |precision - ref| %.3g  |recall - ref| %.3g  |F pair - ref| %.3g  (margin %.3g)' % (
        name, wrong, f['labels'].size, dp, dr, df, float(f['min_margin'])))
    assert parts['labels'].dtype == np.uint8 and wrong == 0                     # every point: no exclusions
    assert np.array_equal(parts['eval_bins'], f['eval_bins']) and np.array_equal(parts['ref_bins'], f['ref_bins'])
    assert np.array_equal(parts['centers'], f['centers64'])
    assert dp <= 1e-12 and dr <= 1e-12 and df <= 1e-12
    assert p.dtype == np.float64 and p.shape == (A,) and r.shape == (A,)


# ---------------------------------------------------------------- 2. the library's own clustering
@functools.lru_cache(maxsize=None)
def own(name, tol):
    f = case(name)
    pts = torch.from_numpy(np.concatenate([f['x'], f['y']]))
    return pts, metrics.kmeans(pts, int(f['num_clusters']), n_init=3, max_iter=300, seed=5, runs=3, tol=tol)


@pytest.mark.parametrize('tol', [0.0, 1e-4])
@pytest.mark.parametrize('name', OWN)
def test_own_clustering_is_consistent(name, tol):
    f = case(name)
    pts, (centres, labels, inertia, iters, conv) = own(name, tol)
    K, n = int(f['num_clusters']), len(pts)
    assert centres.shape == (3, K, pts.shape[1]) and centres.dtype == np.float64 and labels.shape == (3, n)
    want, dist = np_labels(pts.numpy()[:1], pts.numpy()[1:], centres)
    worst = 0.0
    for r in range(3):
        if conv[r]:
            for k in range(K):
                members = pts.numpy()[labels[r] == k].astype(np.float64)
                if len(members):
                    worst = max(worst, float(np.abs(members.mean(0) - centres[r, k]).max()))
    print('\n%s tol %g: rounds %s converged %s  inertia %s (reference %s)  |centre - mean of members| %.3g' % (
        name, tol, iters, conv, inertia, f['inertia'], worst))
    assert np.array_equal(labels, want)                                          # labels ARE the fp64 argmin of the returned centres
    assert np.abs(inertia - dist.sum(1)).max() <= 1e-9 * dist.sum(1).max()
    assert worst <= 1e-9
    assert inertia.min() <= f['inertia'].max()                                   # no worse than the reference's worst fit
    assert (iters >= 1).all() and (iters <= 300).all()
    if tol == 0.0:
        assert conv.any()                                                        # Lloyd reaches its fixed point well inside 300 rounds


@pytest.mark.parametrize('name', OWN)
def test_a_run_does_not_depend_on_its_neighbours(name):
    f = case(name)
    pts, several = own(name, 1e-4)
    alone = metrics.kmeans(pts, int(f['num_clusters']), n_init=3, max_iter=300, seed=5, runs=1, first_run=2)
    first = metrics.kmeans(pts, int(f['num_clusters']), n_init=3, max_iter=300, seed=5, runs=1)
    for got, r in ((alone, 2), (first, 0)):
        for a, b in zip(got, several):
            assert np.array_equal(a[0], b[r])
    assert not np.array_equal(several[0][0], several[0][2])                      # and the runs differ from each other


@pytest.mark.parametrize('name', OWN)
def test_counts_sum_to_the_set_sizes(name):
    f = case(name)
    x, y = tensors(f)
    K = int(f['num_clusters'])
    p, r, parts = metrics.prd(x, y, num_clusters=K, num_angles=51, num_runs=3, n_init=2, return_parts=True)
    assert (parts['eval_bins'].sum(1) == len(x)).all() and (parts['ref_bins'].sum(1) == len(y)).all()
    eb, rb = np_bins(parts['labels'], len(x), K)
    assert np.array_equal(eb, parts['eval_bins']) and np.array_equal(rb, parts['ref_bins'])
    want_p, want_r, raw = np_curve(eb, rb, len(x), len(y), 51)
    assert np.abs(p - want_p).max() <= 1e-12 and np.abs(r - want_r).max() <= 1e-12
    assert np.abs(np.array(parts['f_beta']) - np_f_pair(want_p, want_r)).max() <= 1e-12


# ---------------------------------------------------------------- 3. statistical parity with the reference at full defaults
def spread(f):
    return f['fb_calls'].mean(0), 3 * np.ptp(f['fb_calls'], axis=0)


@pytest.mark.parametrize('name', PARITY)
def test_figures_lie_inside_the_reference_spread(name):
    """Full defaults (10 runs x 10 inits, 201 angles).  The clustering here is full-batch k-means++ / Lloyd, the reference's is
    mini-batch: the bound is 3 x the (max - min) of eight unseeded reference calls around their mean."""
    f = case(name)
    x, y = tensors(f)
    curve = metrics.compute_precision_recall_curve(x, y, num_clusters=int(f['num_clusters']))
    got = metrics.compute_f_beta(*curve)
    mean, bound = spread(f)
    print('\n%s: F pair %s  reference mean %s  deviation %s  bound %s  (deviation / reference range %s)' % (
        name, got, mean, np.abs(got - mean), bound, np.abs(got - mean) / np.maximum(bound / 3, 1e-300)))
    assert curve[0].shape == (201,) and (np.abs(got - mean) <= bound).all()


def test_two_seeds_differ_and_agree():
    f = case('toy500_k20')
    x, y = tensors(f)
    mean, bound = spread(f)
    a = metrics.prd(x, y, num_angles=201, seed=1, return_parts=True)
    b = metrics.prd(x, y, num_angles=201, seed=2, return_parts=True)
    print('\nseeds 1 / 2: F pairs %s %s  reference mean %s bound %s' % (a[2]['f_beta'], b[2]['f_beta'], mean, bound))
    assert not np.array_equal(a[2]['centers'], b[2]['centers']) and a[2]['f_beta'] != b[2]['f_beta']
    for got in (a, b):
        assert (np.abs(np.array(got[2]['f_beta']) - mean) <= bound).all()


# ---------------------------------------------------------------- 4. reproducibility
@pytest.mark.parametrize('name', ['toy500_k20', 'd17'])
def test_same_bits_twice_and_from_the_device(name):
    f = case(name)
    x, y = tensors(f)
    kw = dict(num_clusters=int(f['num_clusters']), num_angles=101, num_runs=3, n_init=3, seed=4)
    a = metrics.prd_device(x, y, **kw).cpu()
    b = metrics.prd_device(x, y, **kw).cpu()
    c = metrics.prd_device(x.to(DEV), y.to(DEV), **kw).cpu()
    d = metrics.prd_device(x.to(DEV), y, **kw).cpu()
    assert a.shape == (2 * 101 + 3,) and a.dtype == torch.float64
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    p, r = metrics.prd(x, y, **kw)
    assert np.array_equal(p, a[:101].numpy()) and np.array_equal(r, a[101:202].numpy())


@pytest.mark.parametrize('name', ['toy500_k20', 'd17'])
def test_replays_from_a_captured_graph(name):
    f = case(name)
    x, y = (t.to(DEV) for t in tensors(f))
    kw = dict(num_clusters=int(f['num_clusters']), num_angles=101, num_runs=2, n_init=2, max_iter=30, seed=4)
    eager = metrics.prd_device(x, y, **kw)              # also the warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = metrics.prd_device(x, y, **kw)
    captured.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager) and float(eager[-1]) <= 1.001 and float(eager[-3]) > 0


# ---------------------------------------------------------------- 5. unequal counts
def test_unequal_counts_equal_the_restatement():
    g = torch.Generator().manual_seed(7)
    x, y = torch.randn(64, 2, generator=g), torch.randn(80, 2, generator=g) + 0.3
    with pytest.raises(ValueError, match='not equal'):
        metrics.compute_prd_from_embedding(x, y, num_clusters=7, num_angles=51, num_runs=3)
    p, r = metrics.compute_prd_from_embedding(x, y, num_clusters=7, num_angles=51, num_runs=3, enforce_balance=False)
    p2, r2, parts = metrics.prd(x, y, num_clusters=7, num_angles=51, num_runs=3, return_parts=True)
    assert np.array_equal(p, p2) and np.array_equal(r, r2)
    want, _ = np_labels(x.numpy(), y.numpy(), parts['centers'])
    assert np.array_equal(parts['labels'], want)
    eb, rb = np_bins(parts['labels'], 64, 7)
    assert (eb.sum(1) == 64).all() and (rb.sum(1) == 80).all()
    want_p, want_r, _ = np_curve(eb, rb, 64, 80, 51)
    print('\nunequal 64, 80: |precision - fp64| %.3g  |recall - fp64| %.3g' % (np.abs(p - want_p).max(), np.abs(r - want_r).max()))
    assert np.abs(p - want_p).max() <= 1e-12 and np.abs(r - want_r).max() <= 1e-12


# ---------------------------------------------------------------- 6. end to end
def test_evaluate_prd_does_not_depend_on_the_chunking_and_takes_samples():
    net, N, real = toy(), 512, real_toy(512)
    results = []
    for bs in (512, 200, 64):
        method, gm, ev = managers()
        res = ev.evaluate_prd({'default': net}, real, N, bs)
        assert set(res) == {'precision', 'recall', 'f_1_pr'} and method.calls == 1
        assert ev.evals['precision'] == [res['precision']] and ev.evals['recall'] == [res['recall']] and ev.evals['f_1_pr'] == [res['f_1_pr']]
        assert ev.evals['density'] == [] and ev.evals['coverage'] == [] and ev.evals['fid'] == [] and ev.evals['mmd'] == []
        results.append(res)
    print('\nevaluate_prd: %s' % results)
    assert results[0] == results[1] == results[2]
    p, r = results[0]['precision'], results[0]['recall']
    assert 0 <= p <= 1 and 0 <= r <= 1 and results[0]['f_1_pr'] == ((2 * p * r) / (p + r) if p + r > 0 else 0.)
    # samples= : no second generation, the same figures; and the figures of the drop-in functions on the same samples
    method, gm, ev = managers()
    value, samples = ev.evaluate_mmd({'default': net}, real, N, 200, return_samples=True)
    res = ev.evaluate_prd({'default': net}, real, N, 200, samples=samples)
    assert method.calls == 1 and res == results[0] and ev.evals['mmd'] == [value] and ev.evals['f_1_pr'] == [res['f_1_pr']]
    fb = metrics.compute_f_beta(*metrics.compute_precision_recall_curve(real[:N], samples.cpu()))
    assert abs(fb[0] - p) <= 1e-12 and abs(fb[1] - r) <= 1e-12      # the host's F pair of the same curve


def test_evaluate_mmd_is_unchanged_by_the_shared_generation_helper():
    with open(os.path.join(GOLDEN, 'f19_evaluate_mmd_pin.json')) as fh:
        pin = json.load(fh)
    method, gm, ev = managers()
    value = ev.evaluate_mmd({'default': toy()}, real_toy(512), 512, 200)
    print('\nevaluate_mmd %r  pinned %r' % (value, pin['toy_mlp_N512_seed9']))
    assert value == pin['toy_mlp_N512_seed9']


def test_cli_eval_prd_equals_the_api(tmp_path, capsys):
    from dlpm_amd import cli
    real = torch.randn(600, 1, 2, generator=torch.Generator().manual_seed(42)).numpy()
    path, out = str(tmp_path / 'real.npy'), str(tmp_path / 'gen.npy')
    np.save(path, real)
    base = ['--config', '2d_data', '--synthetic_weights', '1', '--set_seed', '3', '--reverse_steps', '10', '--generate', '512']
    got = cli.main(base + ['--eval_prd', path, '--batch_size', '200', '--out', out])
    printed = capsys.readouterr().out.strip().splitlines()[-1].split()
    assert printed[0] == 'prd' and printed[1::2][:3] == ['precision', 'recall', 'f_1_pr']
    assert printed[7:] == 'over 512 generated vs 512 real samples'.split()
    for key, text in zip(('precision', 'recall', 'f_1_pr'), printed[2::2]):
        assert float(text) == pytest.approx(got[key], rel=1e-8, abs=1e-12) and math.isfinite(got[key])
    samples = np.load(out)
    fb = metrics.compute_f_beta(*metrics.compute_precision_recall_curve(torch.from_numpy(real[:512]), torch.from_numpy(samples)))
    assert samples.shape == (512, 1, 2) and abs(fb[0] - got['precision']) <= 1e-12 and abs(fb[1] - got['recall']) <= 1e-12
    both = cli.main(base + ['--eval_prd', path, '--eval_mmd', path, '--batch_size', '512'])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-2].split()[0] == 'mmd' and lines[-1].split()[0] == 'prd'
    assert {k: both[k] for k in got} == got and both['mmd'] == metrics.mmd(samples, real[:512])
    other = cli.main(base + ['--eval_prd', path, '--prd_seed', '5'])
    assert other != got or got['precision'] in (0.0, 1.0)
    with pytest.raises(SystemExit):
        cli.main(base + ['--eval_prd', path, '--gen_data_path', str(tmp_path / 'png')])
