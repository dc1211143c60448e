"""Device PRDC on the MI355X against `np_prdc` (tests/test_prdc_cpu.py) and the fixture family f20: the four counts integer for
integer, the figures as counts / denominators, the radii within the fp64 bounds of the two forms; tile and segment edges, duplicates
and ties, fake = real, permutations, repeated calls and graph replay, a NaN in the input, and the three ways in (EvaluationManager,
a features callable, the command line)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dlpm_amd
from dlpm_amd import _lib, metrics
from metric_helpers import managers, real_toy, toy
from test_prdc_cpu import ALL_NAMES, centred_norms, figures_of, fixture, gauss_rows, np_prdc, sq_dists

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
KEYS = ('precision', 'recall', 'density', 'coverage')


def run(real, fake, k):
    fig, parts = metrics.prdc(real, fake, nearest_k=k, return_parts=True, return_radii=True)
    return fig, parts


def check_against(tag, real, fake, k, want_counts, want_rr, want_rf):
    """Counts equal, figures = counts / denominators, radii within the bound of the form; returns the measured radius errors."""
    fig, parts = run(real, fake, k)
    n1, n2, D = len(real), len(fake), int(np.prod(np.shape(real)[1:]))
    counts = parts['counts']
    if D <= 16:
        # direct form: sum (a - b)^2 in d order, D additions and D multiplications of one rounding each, then one square root
        err = max(np.abs(parts['radii_real'] / np.where(want_rr > 0, want_rr, 1) - (want_rr > 0)).max(),
                  np.abs(parts['radii_fake'] / np.where(want_rf > 0, want_rf, 1) - (want_rf > 0)).max())
        bound = 4 * D * EPS
        zeros_ok = bool((parts['radii_real'][want_rr == 0] == 0).all() and (parts['radii_fake'][want_rf == 0] == 0).all())
    else:
        # Gram form: |c_i|^2 + |c_j|^2 - 2 c_i.c_j, each term a D-term fp64 sum of values bounded by max |c|^2
        cr, cg = centred_norms(real, fake)
        err = max(np.abs(parts['radii_real'] ** 2 - want_rr ** 2).max(), np.abs(parts['radii_fake'] ** 2 - want_rf ** 2).max())
        bound = 4 * (D + 8) * EPS * 2 * max(cr.max(), cg.max())
        zeros_ok = True
    print('\n%s: counts %s (want %s)  %s  radius error %.3g  bound %.3g' % (tag, counts.tolist(), np.asarray(want_counts).tolist(),
                                                                       ' '.join('%s %.6f' % (key, fig[key]) for key in KEYS), err, bound))
    assert counts.dtype == np.int64 and np.array_equal(counts, want_counts)
    assert fig == figures_of(counts, n1, n2, k)
    assert err <= bound and zeros_ok
    return err, bound


# ---------------------------------------------------------------- 1, 2: the fixture family
@pytest.mark.parametrize('name', ALL_NAMES)
def test_fixture_counts_are_equal_and_radii_within_the_fp64_bound(name):
    f = fixture(name)
    check_against(name, f['real'], f['fake'], f['k'], f['counts'], f['radii_real'], f['radii_fake'])


def test_lattice_radii_are_exact_and_ties_stay_outside():
    """Integer coordinates: the direct form is exact, so strict `<`, multiplicity in the order statistic and duplicates at distance 0
    come out as the definition has them, radii bit for bit."""
    f = fixture(ALL_NAMES[-1])
    fig, parts = run(f['real'], f['fake'], f['k'])
    assert np.array_equal(parts['counts'], f['counts'])
    assert np.array_equal(parts['radii_real'], f['radii_real']) and np.array_equal(parts['radii_fake'], f['radii_fake'])
    assert (f['radii_real'] == 0).any()                                  # a point with k duplicates: nothing is strictly inside its ball
    # `<=` in place of `<` would count these pairs too
    rg = sq_dists(f['real'], f['fake'])
    assert ((rg <= (f['radii_real'] ** 2)[:, None]).sum()) > f['counts'][2]


# ---------------------------------------------------------------- 3: sizes around the edges
@pytest.fixture(scope='module')
def edge_rows():
    """One row pool per width; every edge case takes its first n1 / n2 rows, and the reference of a case is computed once."""
    pools = {D: gauss_rows(31 + D, 129, 129, D, 1.04, 0.3) for D in (2, 17)}
    for a in pools.values():
        a[0].setflags(write=False)
        a[1].setflags(write=False)
    return pools


@pytest.mark.parametrize('D', [2, 17])
@pytest.mark.parametrize('n1,n2', [(a, b) for a in (127, 128, 129) for b in (127, 128, 129)])
def test_sizes_around_the_tile_edge(edge_rows, n1, n2, D):
    real, fake = edge_rows[D][0][:n1], edge_rows[D][1][:n2]
    counts, _, rr, rf, _ = np_prdc(real, fake, 5)
    check_against('edge %dx%dx%d' % (n1, n2, D), real, fake, 5, counts, rr, rf)


@pytest.mark.parametrize('D', [2, 17])
def test_largest_legal_k_against_the_smallest_set(D):
    real, fake = gauss_rows(40 + D, 33, 33, D, 1.0, 0.2)
    counts, _, rr, rf, _ = np_prdc(real, fake, 32)
    check_against('k = n - 1 = 32, D = %d' % D, real, fake, 32, counts, rr, rf)
    assert rr.tolist() == np.sqrt(sq_dists(real, real).max(axis=1)).tolist()                 # the radius is the farthest point


@pytest.mark.parametrize('D', [2, 17])
def test_ragged_last_column_segment(D):
    """The segment rule (prdc.hip, `segments_of`): T = ceil(n / 128) column tiles, want = min(T, ceil(512 / T)), per = ceil(T / want)
    tiles per segment, ceil(T / per) segments.  n = 5130: T = 41, want = 13, per = 4 -> 11 segments, the last of ONE tile, and that tile
    holds 10 rows."""
    n1, n2 = 5130, 300
    T = -(-n1 // 128)
    per = -(-T // min(T, -(-512 // T)))
    assert (T, per, -(-T // per), T - (-(-T // per) - 1) * per, n1 - (T - 1) * 128) == (41, 4, 11, 1, 10)
    real, fake = gauss_rows(50 + D, n1, n2, D, 1.0, 0.0)
    counts, _, rr, rf, _ = np_prdc(real, fake, 5)
    check_against('ragged %dx%dx%d' % (n1, n2, D), real, fake, 5, counts, rr, rf)


# ---------------------------------------------------------------- 4: fake = real
@pytest.mark.parametrize('n,D', [(5000, 2), (1500, 256)])
def test_fake_equal_to_real(n, D):
    real, _ = gauss_rows(60 + D, n, 1, D, 1.0, 0.0)
    fig, parts = run(real, real, 5)
    print('\nfake = real [%d, %d]: %s counts %s' % (n, D, fig, parts['counts'].tolist()))
    assert fig['precision'] == 1.0 and fig['recall'] == 1.0 and fig['coverage'] == 1.0
    assert np.array_equal(parts['radii_real'], parts['radii_fake'])
    if n == 1500:
        # density from the radii pass alone: the pairs of the set with itself strictly inside a ball, on the host
        rr2 = sq_dists(real, real)
        want_r2 = np.partition(rr2, 5, axis=1)[:, 5]
        pairs = int((rr2 < want_r2[:, None]).sum())
        assert parts['counts'][2] == pairs and fig['density'] == pairs / (5 * n)


# ---------------------------------------------------------------- 5: permutation invariance
@pytest.mark.parametrize('name', ['gauss200x173x2k5', 'gauss300x260x64k5'])
def test_row_permutations_leave_the_counts(name):
    f = fixture(name)
    rs = np.random.RandomState(7)
    pr, pf = rs.permutation(f['n1']), rs.permutation(f['n2'])
    for real, fake in ((f['real'], f['fake'][pf]), (f['real'][pr], f['fake']), (f['real'][pr], f['fake'][pf])):
        fig, parts = run(np.ascontiguousarray(real), np.ascontiguousarray(fake), f['k'])
        assert np.array_equal(parts['counts'], f['counts'])
    if f['D'] <= 16:            # the direct form knows no row order at all; the Gram form's pooled mean is summed in row order
        assert np.array_equal(np.sort(parts['radii_real']), np.sort(run(f['real'], f['fake'], f['k'])[1]['radii_real']))


# ---------------------------------------------------------------- 6: repeated calls and graphs
@pytest.mark.parametrize('name', ['gauss200x173x2k5', 'gauss300x260x64k5'])
def test_same_bits_twice_and_under_graph_replay(name):
    f = fixture(name)
    x, y = torch.from_numpy(f['real']).to(DEV), torch.from_numpy(f['fake']).to(DEV)
    eager = metrics.prdc_device(x, y, f['k'], return_radii=True)                    # also the warm-up
    again = metrics.prdc_device(x, y, f['k'], return_radii=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = metrics.prdc_device(x, y, f['k'], return_radii=True)
    replays = []
    for _ in range(2):
        for t in captured:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in captured])
    assert eager[0].dtype == torch.float64 and eager[0].shape == (8,) and eager[1].dtype == torch.int64 and eager[1].shape == (4,)
    assert float(eager[0][6]) == 0 and np.array_equal(eager[1].cpu().numpy(), f['counts'])
    for other in [again] + replays:
        assert torch.equal(eager[1], other[1])
        for a, b in ((eager[0], other[0]), (eager[2], other[2]), (eager[3], other[3])):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))


# ---------------------------------------------------------------- 7: a NaN in the input
@pytest.mark.parametrize('name', ['gauss200x173x2k5', 'gauss129x131x17k5'])
def test_nan_in_one_row_gives_status_1_and_the_next_call_is_right(name):
    f = fixture(name)
    fake = f['fake'].copy()
    fake[17, 1] = float('nan')
    out, counts = metrics.prdc_device(f['real'], fake, f['k'])
    o = out.cpu().numpy()
    print('\nNaN in fake[17, 1]: out %s counts %s' % (o, counts.cpu().numpy()))
    assert int(o[6]) == 1 and all(math.isnan(v) for v in o[:6])
    with pytest.raises(ValueError, match='non-finite'):
        metrics.prdc(f['real'], fake, f['k'])
    real = f['real'].copy()
    real[3, 0] = float('inf')
    assert int(metrics.prdc_device(real, f['fake'], f['k'])[0][6]) == 1
    fig, parts = run(f['real'], f['fake'], f['k'])                                  # the process goes on, and a clean call is correct
    assert np.array_equal(parts['counts'], f['counts']) and fig == figures_of(f['counts'], f['n1'], f['n2'], f['k'])


def test_compute_prdc_drop_in_takes_fp64_and_rounds_once():
    f = fixture('gauss129x131x16k3')
    want = figures_of(f['counts'], f['n1'], f['n2'], f['k'])
    assert metrics.compute_prdc(real_features=f['real'].astype(np.float64), fake_features=f['fake'].astype(np.float64), nearest_k=f['k']) == want
    assert metrics.compute_prdc(torch.from_numpy(f['real']).to(DEV), f['fake'], f['k']) == want


# ---------------------------------------------------------------- 8: end to end
def test_evaluate_prdc_does_not_depend_on_the_chunking():
    net, N, real = toy(), 300, real_toy(300)
    results = []
    for bs in (128, 300):
        method, gm, ev = managers()
        results.append(ev.evaluate_prdc({'default': net}, real, N, bs))
        assert method.calls == 1
        for key in KEYS + ('f_1_pr', 'f_1_dc'):
            assert ev.evals[key] == [results[-1][key]]
        assert ev.evals['mmd'] == [] and ev.evals['wass'] == [] and ev.evals['fid'] == []
    method, gm, ev = managers()
    _, samples = ev.evaluate_mmd({'default': net}, real, N, 300, return_samples=True)
    _, _, other = managers()
    results.append(other.evaluate_prdc({}, real, N, 64, samples=samples))
    results.append(other.evaluate_prdc({}, real, N, 64, samples=samples))
    print('\nevaluate_prdc: %s' % results[0])
    assert results[0] == results[1] == results[2] == results[3]
    assert all(len(other.evals[key]) == 2 for key in KEYS + ('f_1_pr', 'f_1_dc'))
    r = results[0]
    assert set(r) == set(KEYS) | {'f_1_pr', 'f_1_dc'} and all(isinstance(v, float) for v in r.values())
    assert r['f_1_dc'] == 2 * r['density'] * r['coverage'] / (r['density'] + r['coverage'])
    assert r['f_1_pr'] == 2 * r['precision'] * r['recall'] / (r['precision'] + r['recall'])
    counts, fig, _, _, _ = np_prdc(real[:N].numpy().reshape(N, -1), samples.cpu().numpy().reshape(N, -1), 5)
    assert {key: r[key] for key in KEYS} == fig and 0 < r['coverage'] <= 1


def test_evaluate_prdc_with_a_features_callable():
    net, N, real = toy(), 200, real_toy(200)
    W = torch.randn(2, 32, generator=torch.Generator().manual_seed(5)).to(DEV)
    seen = []

    def features(x):
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape[1:]) == (1, 2)
        seen.append(x.shape[0])
        return x.reshape(x.shape[0], -1) @ W

    method, gm, ev = managers()
    _, samples = ev.evaluate_mmd({'default': net}, real, N, 200, return_samples=True)
    res = [ev.evaluate_prdc({}, real, N, bs, nearest_k=3, features=features, samples=samples) for bs in (64, 200)]
    assert seen == [64, 64, 64, 8] * 2 + [200, 200]
    want = metrics.prdc(real[:N].reshape(N, -1).to(DEV) @ W, samples.reshape(N, -1) @ W, nearest_k=3)
    print('\nfeatures=: %s' % res[0])
    # x @ W of a chunk and of the whole set may round differently in a BLAS; the figures of both chunkings are those of their own rows
    mapped = [torch.cat([t[i:i + 64].reshape(-1, 2).to(DEV) @ W for i in range(0, N, 64)]) for t in (real[:N], samples)]
    assert {key: res[0][key] for key in KEYS} == metrics.prdc(mapped[0], mapped[1], nearest_k=3)
    assert {key: res[1][key] for key in KEYS} == want
    assert res[0]['f_1_dc'] == metrics.f_1(res[0]['density'], res[0]['coverage'])
    with pytest.raises(AssertionError, match=r'float32 \[B, F\]'):
        ev.evaluate_prdc({}, real, N, 64, features=lambda x: x.double().reshape(x.shape[0], -1), samples=samples)


def test_cli_eval_prdc_prints_the_api_figures(tmp_path):
    real = torch.randn(300, 1, 2, generator=torch.Generator().manual_seed(42)).numpy()
    path, out = str(tmp_path / 'real.npy'), str(tmp_path / 'gen.npy')
    np.save(path, real)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'dlpm_amd.cli', '--config', '2d_data', '--synthetic_weights', '1', '--set_seed', '3',
                        '--reverse_steps', '10', '--generate', '256', '--batch_size', '100', '--eval_prdc', path, '--nearest_k', '4', '--out',
                        out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    words = r.stdout.strip().splitlines()[-1].split()
    print('\ncli: %s' % ' '.join(words))
    assert words[0] == 'prdc' and words[13:] == 'over 256 generated vs 256 real samples'.split()
    printed = {words[i]: float(words[i + 1]) for i in range(1, 13, 2)}
    samples = np.load(out)
    want = metrics.prdc(real[:256], samples, nearest_k=4)
    want.update(f_1_pr=metrics.f_1(want['precision'], want['recall']), f_1_dc=metrics.f_1(want['density'], want['coverage']))
    assert samples.shape == (256, 1, 2) and set(printed) == set(want)
    for key, v in want.items():
        assert printed[key] == pytest.approx(v, rel=1e-8), key


# ---------------------------------------------------------------- 9: the C entry point's refusals, with device pointers
def test_c_entry_point_refusals_leave_the_outputs_alone():
    L = _lib.lib()
    x, y = torch.zeros(40, 3, device=DEV), torch.zeros(30, 3, device=DEV)
    need = L.dlpm_prdc_workspace_bytes(40, 30, 3, 5)
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=DEV)
    out = torch.full((8,), -7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    good = dict(x=x.data_ptr(), n1=40, y=y.data_ptr(), n2=30, D=3, k=5, ws=ws.data_ptr(), wsb=need, rr=None, rf=None, counts=counts.data_ptr(),
                out=out.data_ptr())

    def call(**o):
        a = dict(good, **o)
        return L.dlpm_prdc_f32(a['x'], a['n1'], a['y'], a['n2'], a['D'], a['k'], a['ws'], a['wsb'], a['rr'], a['rf'], a['counts'], a['out'],
                               _lib.stream_ptr())

    for over, code in [(dict(n1=0), -1), (dict(n2=0), -1), (dict(D=0), -1), (dict(k=0), -1), (dict(k=33), -1), (dict(k=30), -1), (dict(n2=5), -1),
                       (dict(x=None), -1), (dict(y=None), -1), (dict(ws=None), -1), (dict(counts=None), -1), (dict(out=None), -1),
                       (dict(ws=ws.data_ptr() + 8), -1), (dict(wsb=need - 1), -5), (dict(wsb=0), -5)]:
        assert call(**over) == code, over
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (counts == -7).all()                   # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert float(out[6]) == 0 and (counts >= 0).all()
