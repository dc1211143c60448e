"""The 2-D toy data distributions on the MI355X.  Stage B (normalisation, quantile clamp) against the reference's own post-processing
of its own points (F23, injected with raw=); stage A's structure exactly (reproducibility, chunk invariance, exact proportions and the
permutation of sas_grid, the geometry of every kind at std = 0); stage A's distributions at a fixed seed against bounds derived from
N and delta alone; and EvaluationManager / the CLI from the config alone.  Every test prints the figures it measured before it asserts."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden, ROOT
import dlpm_amd
from dlpm_amd import datasets
from metric_helpers import toy
from toy_helpers import KINDS, SIZES, U, norm_bound, np_between, np_normalize

pytestmark = pytest.mark.gpu
DEV = 'cuda'
WEIGHTS = [0.01, 0.1, 0.3, 0.2, 0.02, 0.15, 0.02, 0.15, 0.05]
FN = dict(gmm_2=datasets.sample_2_gmm, gmm_grid=datasets.sample_grid_gmm, swiss_roll=datasets.gen_swiss_roll,
          sas_grid=datasets.sample_grid_sas)
KW = dict(gmm_2=dict(std=0.1, theta=3.0), gmm_grid=dict(n=3, std=0.1, weights=WEIGHTS), swiss_roll=dict(std=0.1),
          sas_grid=dict(alpha=1.7, n=3, std=0.1, weights=WEIGHTS, isotropic=True))


@functools.lru_cache(maxsize=None)
def f23(kind):
    return {k: v for k, v in golden('f23_toy_' + kind).items()}


def host(x):
    return x.cpu().numpy()


def on_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def clamp_bound(kind, ref_norm, raw, m, s, ref_out, c_ref):
    """|device - reference| after normalise + clamp + divide.  An order statistic moves by at most the largest element error
    (sorting is 1-Lipschitz in the sup norm), the clamp is 1-Lipschitz, and y = clamp(x) / c:
    |dy| <= (d_i + |y| d_max) / c + 2 u |y| for the two fp32 divisions."""
    d = norm_bound(kind, ref_norm, raw, m, s)
    y = np.abs(ref_out.astype(np.float64))
    return ((d + y * d.max()) / c_ref.astype(np.float64)) * (1 + 2.0 ** -20) + 2 * U * y


# ---------------------------------------------------------------- stage B against the reference (F23)
@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('kind', [k for k in KINDS if k != 'swiss_roll'])
def test_clamp_without_normalisation_equals_the_reference_bit_for_bit(kind, N):
    f = f23(kind)
    raw = f['raw_%d' % N]
    for tag, q in (('bt99', 0.99), ('bt100', 1.0)):
        assert not int(f['%s_%d_raises' % (tag, N)])
        out = FN[kind](N, raw=raw, between_minus_1_1=True, quantile_cutoff=q, **KW[kind])
        x, parts, status = datasets.finish(on_device(raw), between_minus_1_1=True, quantile_cutoff=q, check=False)
        _, _, (hi, lo, c) = np_between(raw, q)
        parts = parts.numpy()
        print('\n%s N=%d q=%g: hi %s lo %s c %s  device %s' % (kind, N, q, hi, lo, c, parts[2:]))
        assert status == 0 and np.isnan(parts[:2]).all()
        # the same array elements the reference picked
        assert np.array_equal(parts[[2, 5]].astype(np.float32), hi) and np.array_equal(parts[[3, 6]].astype(np.float32), lo)
        assert np.array_equal(parts[[4, 7]].astype(np.float32), c)
        assert np.array_equal(host(out), f['%s_%d' % (tag, N)]) and np.array_equal(host(x), host(out))


@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('kind', KINDS)
def test_normalisation_differs_from_the_reference_only_through_rounding(kind, N):
    """norm_bound (tests/toy_helpers.py): for the three numpy kinds derived from the two roundings -- the reference
    normalises fp64 points and rounds once, the device normalises their fp32 roundings with fp64 moments and rounds once; for sas_grid
    4 x the deviation measured on these cases (0.382 of the same expression)."""
    f = f23(kind)
    raw, ref = f['raw_%d' % N], f['norm_%d' % N]
    out = host(FN[kind](N, raw=raw, normalize=True, **KW[kind]))
    _, m, s = np_normalize(raw, torch_std=kind == 'sas_grid')
    err, bound = np.abs(out.astype(np.float64) - ref), norm_bound(kind, ref, raw, m, s)
    _, parts, _ = datasets.finish(on_device(raw), normalize=True, torch_std=kind == 'sas_grid', check=False)
    print('\n%s N=%d: max |device - reference| %.3g, largest share of the bound %.3f; m %.17g (numpy %.17g) s %.17g (numpy %.17g)' % (
        kind, N, err.max(), (err / bound).max(), parts[0], m, parts[1], s))
    assert abs(float(parts[0]) - m) <= 1e-13 * (abs(m) + s) and abs(float(parts[1]) - s) <= 1e-13 * s
    assert np.all(err <= bound)
    if int(f['norm_bt99_%d_raises' % N]) and kind != 'swiss_roll':
        return
    # normalise, then clamp: the reference's own output where it gives one, else (swiss_roll, whose clamp the reference cannot run)
    # the clamp of the reference's normalised points
    want, status, (_, _, c) = np_between(ref, 0.99)
    if kind != 'swiss_roll':
        assert np.array_equal(want, f['norm_bt99_%d' % N])
    assert status == 0
    got = host(FN[kind](N, raw=raw, normalize=True, between_minus_1_1=True, quantile_cutoff=0.99, **KW[kind]))
    err, bound = np.abs(got.astype(np.float64) - want), clamp_bound(kind, ref, raw, m, s, want, c)
    print('%s N=%d normalise + clamp: max |device - reference| %.3g, largest share of the bound %.3f' % (kind, N, err.max(), (err / bound).max()))
    assert np.all(err <= bound) and np.abs(got).max() == 1.0


def test_a_one_sided_column_raises_as_the_reference_asserts():
    f = f23('gmm_2')
    assert int(f['norm_bt99_64_raises'])
    _, status, _ = np_between(f['norm_64'], 0.99)
    with pytest.raises(ValueError, match='high quantile is negative' if status & 1 else 'low quantile is positive'):
        datasets.sample_2_gmm(64, raw=f['raw_64'], normalize=True, between_minus_1_1=True, quantile_cutoff=0.99, **KW['gmm_2'])
    raw = np.abs(f['raw_64']) + 1.0
    with pytest.raises(ValueError, match='low quantile is positive'):
        datasets.sample_grid_gmm(64, raw=raw, between_minus_1_1=True, n=3, std=0.1)
    with pytest.raises(ValueError, match='high quantile is negative and a low quantile is positive'):
        datasets.sample_grid_gmm(64, raw=raw * np.array([1, -1], np.float32), between_minus_1_1=True, n=3, std=0.1)
    x, parts, status = datasets.finish(on_device(raw), between_minus_1_1=True, check=False)
    assert status == 2 and np.array_equal(host(x), raw)             # refused data is left as it was


@pytest.mark.parametrize('N', [1, 2, 63, 64, 65, 257, 1000])
def test_stage_b_at_the_rank_and_wave_edges(N):
    """Against the NumPy restatement of the device's own arithmetic: the clamp exactly, the normalisation to one fp32 ulp (fp64 sums in
    another order may move a result across a rounding boundary)."""
    g = np.random.default_rng(230 + N)
    raw = g.standard_normal((N, 2)).astype(np.float32) * np.float32(3)
    for torch_std in (False, True):
        want, m, s = np_normalize(raw, torch_std)
        x, parts, _ = datasets.finish(on_device(raw), normalize=True, torch_std=torch_std, check=False)
        err = np.abs(host(x).astype(np.float64) - want)
        print('\nN=%d torch_std=%s: m %.17g (numpy %.17g) s %.17g (numpy %.17g), max error %.3g' % (N, torch_std, parts[0], m, parts[1], s, err.max()))
        assert abs(float(parts[0]) - m) <= 1e-13 * (abs(m) + s) and abs(float(parts[1]) - s) <= 1e-13 * s
        assert np.all(err <= 2 * U * np.abs(want) + 1e-30)
    for q in (0.99, 1.0, 0.75, 0.5 + 2.0 ** -20):
        want, wstatus, (hi, lo, c) = np_between(raw, q)
        x, parts, status = datasets.finish(on_device(raw), between_minus_1_1=True, quantile_cutoff=q, check=False)
        parts = parts.numpy()
        print('N=%d q=%g: status %d (numpy %d) hi %s lo %s' % (N, q, status, wstatus, parts[[2, 5]], parts[[3, 6]]))
        assert status == wstatus
        assert np.array_equal(parts[[2, 5]].astype(np.float32), hi) and np.array_equal(parts[[3, 6]].astype(np.float32), lo)
        assert np.array_equal(host(x), want if status == 0 else raw)


# ---------------------------------------------------------------- stage A: structure, exact
def draw(kind, N, **over):
    kw = dict(KW[kind], **over)
    return host(FN[kind](N, **kw))


@pytest.mark.parametrize('kind', KINDS)
def test_two_calls_give_identical_bits_and_seeds_differ(kind):
    a, b, c, d = draw(kind, 257, seed=5), draw(kind, 257, seed=5), draw(kind, 257, seed=6), draw(kind, 257, seed=5, stream=1)
    assert a.shape == (257, 2) and a.dtype == np.float32 and np.isfinite(a).all()
    assert np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(a, d)
    assert (a != c).mean() > 0.9 and (a != d).mean() > 0.9


@pytest.mark.parametrize('kind', ['gmm_2', 'gmm_grid', 'swiss_roll'])
def test_chunk_invariance(kind):
    over = dict(seed=11)
    if kind == 'swiss_roll':                    # (its normalisation acts on the rows of a call: the raw draw is what is chunked)
        fn = lambda N, first: host(datasets.draw('swiss_roll', N, std=0.1, seed=11, first_index=first))
    else:
        fn = lambda N, first: draw(kind, N, first_index=first, **over)
    for whole, cut in ((1000, 257), (129, 64)):
        full = fn(whole, 0)
        assert np.array_equal(full, np.concatenate([fn(cut, 0), fn(whole - cut, cut)]))
        assert not np.array_equal(full[:cut], full[cut:2 * cut])


def test_sas_grid_is_drawn_whole():
    with pytest.raises(ValueError, match='drawn\\s+whole'):
        datasets.sample_grid_sas(64, first_index=64, **KW['sas_grid'])


@pytest.mark.parametrize('N', [1, 2, 3, 64, 257, 1000, 32000])
def test_sas_grid_exact_proportions_and_permutation(N):
    bounds = golden('f23_toy_tables')['bounds_%d' % N]
    x, perm = datasets.draw('sas_grid', N, n=3, std=0.0, weights=WEIGHTS, alpha=1.7, isotropic=True, seed=4, return_perm=True)
    x, perm = host(x), host(perm)
    assert np.array_equal(np.sort(perm), np.arange(N))                          # pi is a bijection of [0, N)
    grid = x + 1.5
    assert np.array_equal(grid, np.rint(grid)) and grid.min() >= 0 and grid.max() <= 2          # exactly on grid points
    comp = (3 * grid[:, 0] + grid[:, 1]).astype(np.int64)
    want = np.searchsorted(bounds, perm, side='right') - 1                      # bounds[k] <= r < bounds[k + 1]
    uncovered = perm >= bounds[-1]
    want[uncovered] = 0                                                         # no offset: (-n / 2, -n / 2), where component 0 sits too
    counts = np.bincount(comp, minlength=9)
    expect = np.diff(bounds)
    expect[0] += N - bounds[-1]
    print('\nN=%d: counts %s, boundary differences %s, uncovered %d' % (N, counts, np.diff(bounds), uncovered.sum()))
    assert np.array_equal(comp, want) and np.array_equal(counts, expect)
    assert np.array_equal(x[uncovered], np.full((uncovered.sum(), 2), -1.5, np.float32))
    if N >= 64:
        assert (np.diff(comp) < 0).sum() > N // 16 and not np.array_equal(perm, np.arange(N))       # shuffled, not sorted
        other = host(datasets.draw('sas_grid', N, n=3, std=0.0, weights=WEIGHTS, alpha=1.7, seed=5, return_perm=True)[1])
        assert not np.array_equal(other, perm)


def test_gmm_grid_rows_sit_on_the_means_at_std_0_in_the_weights_proportions():
    """N = 20000: every component count within 5 sqrt(N w (1 - w)) of N w (a binomial count; 5 sigma, P < 6e-7 per component)."""
    N = 20000
    x = draw('gmm_grid', N, std=0.0, seed=7)
    assert np.array_equal(x, np.rint(x)) and x.min() == 0 and x.max() == 2      # the means (i, j), not centred
    counts = np.bincount((3 * x[:, 0] + x[:, 1]).astype(np.int64), minlength=9)
    w = np.array(WEIGHTS)
    dev = np.abs(counts - N * w) / np.sqrt(N * w * (1 - w))
    print('\ngmm_grid counts %s, expected %s, deviations in sigma %s' % (counts, N * w, np.round(dev, 2)))
    assert counts.sum() == N and np.all(dev <= 5)
    y = draw('gmm_2', 4096, std=0.0, theta=3.0, weights=[0.25, 0.75], seed=7)
    assert set(map(tuple, y)) == {(3.0, 0.0), (-3.0, 0.0)}
    n_plus = (y[:, 0] > 0).sum()
    assert abs(n_plus - 1024) <= 5 * math.sqrt(4096 * 0.25 * 0.75)
    u = draw('gmm_grid', 4096, std=0.0, weights=None, seed=7)                   # default weights 1 / n^2
    cu = np.bincount((3 * u[:, 0] + u[:, 1]).astype(np.int64), minlength=9)
    assert np.all(np.abs(cu - 4096 / 9) <= 5 * math.sqrt(4096 * (1 / 9) * (8 / 9)))
    last = draw('gmm_grid', 64, std=0.0, weights=[0.0] * 9, seed=7)             # u at or beyond the last entry: the last component
    assert np.array_equal(last, np.full((64, 2), 2.0, np.float32))


def test_swiss_roll_geometry_at_std_0():
    x = host(datasets.draw('swiss_roll', 4096, std=0.0, seed=8)).astype(np.float64)
    r, ang = np.hypot(x[:, 0], x[:, 1]), np.arctan2(x[:, 1], x[:, 0])
    d = np.abs((ang - r + np.pi) % (2 * np.pi) - np.pi)                         # atan2(z, x) against t mod 2 pi, wrapped
    print('\nswiss_roll: t in [%.6f, %.6f] (1.5 pi = %.6f, 4.5 pi = %.6f), largest angle error %.3g' % (
        r.min(), r.max(), 1.5 * np.pi, 4.5 * np.pi, d.max()))
    assert r.min() >= 1.5 * np.pi * (1 - 1e-6) and r.max() <= 4.5 * np.pi * (1 + 1e-6) and d.max() <= 1e-5
    assert r.max() - r.min() > 0.99 * 3 * np.pi
    n = host(datasets.gen_swiss_roll(4096, std=0.0, seed=8)).astype(np.float64)      # always normalised
    assert abs(n.mean()) < 1e-6 and abs(n.std() - 1) < 1e-6


def test_sas_grid_a_is_per_row_when_isotropic_and_per_element_otherwise():
    """The normals do not depend on data_alpha, and at data_alpha = 2 the point is sqrt(2) z: dividing a heavy-tailed draw by it gives
    sqrt(a / 2) per coordinate.  Isotropic: the two quotients of a row agree (so x0 / x1 is the ratio of its two normals, a Cauchy
    variable, and a row with a huge |x0| has a huge |x1| to the same factor); non-isotropic: they differ.  fp32: each value carries
    a few roundings relative to max(|v|, 0.5), so rows are compared where |v| >= 0.1 at 1e-4."""
    kw = dict(n=1, std=1.0, weights=[1.0], seed=12)
    N = 4096
    g = draw('sas_grid', N, **dict(kw, alpha=2.0, isotropic=True)) + 0.5
    iso = draw('sas_grid', N, **dict(kw, alpha=1.7, isotropic=True)) + 0.5
    non = draw('sas_grid', N, **dict(kw, alpha=1.7, isotropic=False)) + 0.5
    keep = (np.abs(g) >= 0.1).all(axis=1) & (np.abs(iso) >= 0.1).all(axis=1) & (np.abs(non) >= 0.1).all(axis=1)
    qi, qn = (iso / g)[keep].astype(np.float64), (non / g)[keep].astype(np.float64)
    ri, rn = np.abs(qi[:, 0] / qi[:, 1] - 1), np.abs(qn[:, 0] / qn[:, 1] - 1)
    print('\n%d rows kept; isotropic: largest |q0 / q1 - 1| %.3g; non-isotropic: %.1f %% of rows beyond 1e-3' % (
        keep.sum(), ri.max(), 100 * (rn > 1e-3).mean()))
    assert keep.sum() > N // 2 and (qi > 0).all() and (qn > 0).all()
    assert ri.max() <= 1e-4 and (rn > 1e-3).mean() >= 0.99
    assert not np.array_equal(iso[:, 0], iso[:, 1]) and (iso[:, 0] != iso[:, 1]).all()
    assert np.array_equal(non[:, 0] / g[:, 0], iso[:, 0] / g[:, 0])             # element 0's a is the row's a
    top = np.argsort(qi[:, 0])[-8:]                                             # the rows with the largest a: both coordinates carry it
    print('largest sqrt(a / 2): %s by coordinate 0, %s by coordinate 1' % (np.round(qi[top, 0], 3), np.round(qi[top, 1], 3)))
    assert (qi[top, 1] >= qi[top, 0] * (1 - 1e-4)).all()


def test_dim_1_keeps_column_0():
    p = dlpm_amd.load_config('2d_data')
    small = dict(p, data=dict(p['data'], nsamples=300))
    two = dlpm_amd.get_dataset(small, DEV, 3)
    one = dlpm_amd.get_dataset(dict(small, data=dict(small['data'], dim=1)), DEV, 3)
    assert all(t.shape == (300, 1, 2) and t.is_cuda and t.dtype == torch.float32 for t in two)
    assert all(t.shape == (300, 1, 1) for t in one)
    assert torch.equal(one[0], two[0][..., :1]) and torch.equal(one[1], two[1][..., :1])
    assert not torch.equal(two[0], two[1])                                      # train and test: two stream keys
    again = dlpm_amd.get_dataset(small, DEV, 3)
    assert torch.equal(again[0], two[0]) and torch.equal(again[1], two[1])
    assert not torch.equal(dlpm_amd.get_dataset(small, DEV, 4)[0], two[0])
    assert torch.equal(two[0][:, 0], datasets.sample_grid_gmm(300, n=3, std=0.1, weights=WEIGHTS, seed=3, stream=0))
    g = dlpm_amd.Generator('gmm_grid', n=3, std=0.1, weights=WEIGHTS, seed=3)
    assert torch.equal(g.generate(n_samples=300), two[0][:, 0]) and g.samples is not None and len(g) == 300


# ---------------------------------------------------------------- stage A: distributions at a fixed seed
DKW_N = 65536
DKW = math.sqrt(math.log(2 / 1e-6) / (2 * DKW_N))         # sup |F_N - F| <= 0.01052 with probability 1 - 1e-6


def ecdf(v, grid):
    return np.searchsorted(np.sort(v), grid, side='right') / len(v)


def test_gmm_normals_pass_dkw():
    grid = np.linspace(-4, 4, 41)
    x = draw('gmm_2', DKW_N, std=1.0, theta=0.0, weights=[1.0, 0.0], seed=21)
    want = np.array([0.5 * (1 + math.erf(t / math.sqrt(2))) for t in grid])     # the standard normal CDF
    for col in (0, 1):
        d = np.abs(ecdf(x[:, col], grid) - want).max()
        print('\ngmm_2 column %d: sup |F_N - Phi| on the grid %.5f (DKW %.5f); largest |z| %.3f' % (col, d, DKW, np.abs(x[:, col]).max()))
        assert d <= DKW
    assert abs(np.corrcoef(x[:, 0], x[:, 1])[0, 1]) <= 5 / math.sqrt(DKW_N)


@pytest.mark.parametrize('alpha', [1.7, 1.0, 2.0])
def test_sas_grid_law_passes_dkw_against_the_references_own_draw(alpha):
    t = golden('f23_toy_tables')
    grid, want = t['cdf_grid'], t['cdf_%s' % str(alpha).replace('.', 'p')]
    x = draw('sas_grid', DKW_N, n=1, std=1.0, weights=[1.0], alpha=alpha, isotropic=True, seed=22).astype(np.float64) + 0.5
    for col in (0, 1):
        d = np.abs(ecdf(x[:, col], grid) - want).max()
        print('\nsas_grid alpha=%g column %d: sup |F_N - F_ref| on the grid %.5f (DKW %.5f + 0.001)' % (alpha, col, d, DKW))
        assert d <= DKW + 1e-3


# ---------------------------------------------------------------- end to end
def managers_from_config(seed=3, batch=100):
    p = dlpm_amd.load_config('2d_data')
    method = dlpm_amd.GenerativeLevyProcess(1.7, DEV, 5, rescale_timesteps=True, seed=9)
    loader = dlpm_amd.ToyLoader(dlpm_amd.get_dataset(p, DEV, seed)[0], batch)
    gm = dlpm_amd.GenerationManager(method, loader, False, reverse_steps=5)
    return gm, dlpm_amd.EvaluationManager(method, gm, None, verbose=False, is_image=False)


def test_evaluate_metrics_2d_from_the_config_alone():
    models = {'default': toy()}
    gm, ev = managers_from_config()
    res = ev.evaluate_metrics_2d(models, None, 257, 100)
    print('\nfrom the config alone: %s' % {k: res[k] for k in ('wass', 'mmd', 'precision', 'recall', 'f_1_pr')})
    for k in ('wass', 'mmd', 'precision', 'recall', 'f_1_pr'):
        assert math.isfinite(res[k]) and ev.evals[k] == [res[k]]
    gm2, ev2 = managers_from_config()
    real = gm2.load_original_data(257)
    assert real.shape == (257, 1, 2) and real.is_cuda
    explicit = ev2.evaluate_metrics_2d(models, real, 257, 100)
    gm3, ev3 = managers_from_config()
    again = ev3.evaluate_metrics_2d(models, None, 257, 100)
    for k in ('wass', 'mmd', 'precision', 'recall', 'f_1_pr'):
        assert res[k] == explicit[k] == again[k]
    assert torch.equal(res['samples'], explicit['samples']) and torch.equal(res['samples'], again['samples'])
    assert ev.evaluate_mmd(models, None, 257, 100, samples=res['samples']) == res['mmd']
    whole = torch.cat([b[0] for b in gm.original_data])
    assert whole.shape == (32000, 1, 2)
    for n in (1, 99, 100, 101, 257):
        assert torch.equal(gm.load_original_data(n), whole[:n])
    means = np.array([[i, j] for i in range(3) for j in range(3)], np.float64)
    dist = np.abs(host(real)[:, 0, None, :] - means[None]).max(axis=2).min(axis=1)
    assert dist.max() <= 0.6


def test_cli_eval_2d_runs_from_the_config_alone(tmp_path):
    out = str(tmp_path / 'real.npy')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'dlpm_amd.cli', '--config', '2d_data', '--synthetic_weights', '1', '--set_seed', '3',
                        '--reverse_steps', '5', '--generate', '257', '--eval_2d', '--dump_dataset', out],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    words = r.stdout.strip().splitlines()[-1].split()
    print('\ncli: %s' % ' '.join(words))
    assert words[0] == 'eval_2d' and words[1::2][:5] == ['wass', 'mmd', 'precision', 'recall', 'f_1_pr']
    assert all(math.isfinite(float(v)) for v in words[2::2][:5]) and words[11:] == 'over 257 generated vs 257 real samples'.split()
    real = np.load(out)
    assert real.shape == (257, 1, 2) and real.dtype == np.float32 and np.isfinite(real).all()
    means = np.array([[i, j] for i in range(3) for j in range(3)], np.float64)
    dist = np.linalg.norm(real[:, 0, None, :] - means[None], axis=2).min(axis=1)
    print('largest distance to a mean %.3f (6 std = 0.6)' % dist.max())
    assert dist.max() <= 0.6
    assert np.array_equal(real, host(dlpm_amd.get_dataset(dlpm_amd.load_config('2d_data'), DEV, 3)[0][:257]))


def test_cli_dataset_override(tmp_path, capsys):
    """--dataset names another kind of the same description; gmm_2 cannot take the config's nine grid weights and gets equal ones."""
    from dlpm_amd import cli
    base = ['--config', '2d_data', '--synthetic_weights', '1', '--set_seed', '3', '--reverse_steps', '5', '--generate', '64', '--eval_2d']
    out = str(tmp_path / 'gmm2.npy')
    res = cli.main(base + ['--dataset', 'gmm_2', '--dump_dataset', out])
    err = capsys.readouterr().err
    real = np.load(out)
    print('\n--dataset gmm_2: %s; stderr: %s' % ({k: res[k] for k in ('wass', 'mmd')}, err.strip()))
    assert 'two components get equal weights' in err and math.isfinite(res['wass']) and math.isfinite(res['mmd'])
    assert real.shape == (64, 1, 2) and np.all(np.abs(np.abs(real[:, 0, 0]) - 3.0) <= 0.6) and np.all(np.abs(real[:, 0, 1]) <= 0.6)
    assert (real[:, 0, 0] > 0).any() and (real[:, 0, 0] < 0).any()
    p = dlpm_amd.load_config('2d_data')
    want = dlpm_amd.get_dataset(dict(p, data=dict(p['data'], dataset='gmm_2', weights=None)), DEV, 3)[0][:64]
    assert np.array_equal(real, host(want))
    out = str(tmp_path / 'sas.npy')
    res = cli.main(base + ['--dataset', 'sas_grid', '--dump_dataset', out])
    assert 'equal weights' not in capsys.readouterr().err and math.isfinite(res['mmd'])
    want = dlpm_amd.get_dataset(dict(p, data=dict(p['data'], dataset='sas_grid')), DEV, 3)[0][:64]
    assert np.array_equal(np.load(out), host(want))
