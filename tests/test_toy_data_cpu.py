"""The 2-D toy data distributions, the parts that need no GPU: the C ABI of the three entry points of include/dlpm_amd_toy.h, every
refusal of the C entry points (all before any launch), Generator's interface, the config's `data:` keys with the experiment hash of
the parent commit, and the integrity of fixture family F23 under a NumPy re-computation."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden
import dlpm_amd
from dlpm_amd import _lib, datasets
from metric_helpers import buffers
from toy_helpers import KINDS, SIZES, norm_bound, np_between, np_normalize

WEIGHTS = [0.01, 0.1, 0.3, 0.2, 0.02, 0.15, 0.02, 0.15, 0.05]


# ---------------------------------------------------------------- refusals of the C entry points
def test_draw_refuses_before_any_launch():
    """No GPU here: every one of these returns before a kernel is launched (the device pointers are host addresses, never followed)."""
    L = _lib.lib()
    buf, p = buffers()
    w9, w2 = np.array(WEIGHTS), np.array([0.5, 0.5])

    def args(name, w, **o):
        a = _lib.ToyDrawArgs()
        a.out_dev = a.cum_dev = a.bounds_dev = p
        a.kind, a.N, a.std, a.theta, a.data_alpha, a.isotropic = datasets.KINDS[name], 8, 0.1, 3.0, 1.7, 1
        a.n_mixture = 9 if name.endswith('grid') else 0
        if w is not None:
            a.weights_host, a.count, a.held = w.ctypes.data, len(w), w
        for k, v in o.items():
            setattr(a, k, v)
        return a
    bad = lambda i, v: np.array([v if k == i else x for k, x in enumerate(WEIGHTS)])
    held = [bad(3, -0.1), bad(0, np.nan), bad(8, np.inf), bad(2, 0.3 + 1e-9), np.array(WEIGHTS[:8]), np.array([1 / 3] * 3)]
    cases = [(args('gmm_grid', w9, N=0), 'N must lie'), (args('gmm_grid', w9, N=-4), 'N must lie'), (args('swiss_roll', None, N=0), 'N must lie'),
             (args('gmm_grid', w9, N=1 << 31), 'N must lie'), (args('gmm_grid', w9, kind=4), 'unknown kind'),
             (args('gmm_grid', w9, kind=-1), 'unknown kind'), (args('gmm_grid', w9, n_mixture=8), 'not a perfect square'),
             (args('sas_grid', w9, n_mixture=10), 'not a perfect square'), (args('gmm_grid', w9, n_mixture=0), 'n_mixture must lie'),
             (args('gmm_grid', held[4]), '8 weights for 9 components'), (args('gmm_2', held[5]), '3 weights for 2 components'),
             (args('sas_grid', w2), '2 weights for 9 components'), (args('gmm_grid', held[0]), 'weight 3 is'),
             (args('gmm_grid', held[1]), 'weight 0 is'), (args('sas_grid', held[2]), 'weight 8 is'),
             (args('gmm_grid', held[3]), 'above 1'), (args('gmm_2', np.array([0.5, 0.5 + 1e-9])), 'above 1'),
             (args('sas_grid', w9, data_alpha=0.0), 'Wrong value of alpha'), (args('sas_grid', w9, data_alpha=2.5), 'Wrong value of alpha'),
             (args('sas_grid', w9, data_alpha=-1.0), 'Wrong value of alpha'), (args('gmm_2', w2, std=-0.1), 'std must be'),
             (args('swiss_roll', None, std=float('nan')), 'std must be'), (args('sas_grid', w9, std=-1.0), 'std must be'),
             (args('gmm_grid', np.full(4225, 1 / 4225), n_mixture=4225), 'n_mixture must lie'),
             (args('sas_grid', w9, first_index=5), 'drawn\\s+whole'), (args('gmm_2', w2, first_index=-1), 'first_index'),
             (args('gmm_2', w2, stream=1 << 24), 'stream'), (args('gmm_2', w2, out_dev=None), 'null pointer'),
             (args('gmm_2', w2, cum_dev=None), 'null cumulative'), (args('sas_grid', w9, bounds_dev=None), 'null bounds'),
             (args('gmm_2', None, count=2), 'null weights'), (args('gmm_2', w2, out_dev=p + 4), 'misaligned')]
    for a, word in cases:
        with pytest.raises(ValueError, match=word):
            _lib.check(L.dlpm_toy_draw_f32(C.byref(a), None))
    with pytest.raises(ValueError, match='null pointer'):
        _lib.check(L.dlpm_toy_draw_f32(None, None))
    # 4096 components are admitted by the checks: 64 x 64 with a weight count that does not match is refused for the COUNT
    with pytest.raises(ValueError, match='9 weights for 4096 components'):
        _lib.check(L.dlpm_toy_draw_f32(C.byref(args('gmm_grid', w9, n_mixture=4096)), None))
    assert buf.sum() == 0
    with pytest.raises(ValueError, match='N must lie'):
        datasets.sample_grid_gmm(0, n=3, std=0.1, weights=WEIGHTS)
    with pytest.raises(ValueError, match='unknown toy distribution'):
        datasets.draw('rose', 8, std=0.1)
    with pytest.raises(ValueError, match='std is required'):
        datasets.sample_2_gmm(8)
    with pytest.raises(ValueError, match='n is required'):
        datasets.sample_grid_sas(8, std=0.1)


def test_finish_refuses_before_any_launch():
    L = _lib.lib()
    buf, p = buffers()
    good = dict(x=p, N=8, normalize=1, divisor=0, between=1, q=0.99, ws=p + 256, ws_bytes=256, out=p + 512, status=p + 1024)

    def call(**o):
        g = dict(good, **o)
        return L.dlpm_toy_finish_f32(g['x'], g['N'], g['normalize'], g['divisor'], g['between'], g['q'], g['ws'], g['ws_bytes'], g['out'],
                                     g['status'], None)
    for o, word in [(dict(N=0), 'N must lie'), (dict(N=-1), 'N must lie'), (dict(q=0.5), 'quantile_cutoff'), (dict(q=1.0 + 1e-9), 'quantile_cutoff'),
                    (dict(q=0.2), 'quantile_cutoff'), (dict(q=float('nan')), 'quantile_cutoff'), (dict(x=None), 'null pointer'),
                    (dict(ws=None), 'null pointer'), (dict(status=None), 'null pointer'), (dict(divisor=2), 'std_divisor'),
                    (dict(x=p + 4), 'misaligned'), (dict(out=p + 4), 'misaligned'), (dict(ws=p + 8), 'misaligned workspace')]:
        with pytest.raises(ValueError, match=word):
            _lib.check(call(**o))
    with pytest.raises(_lib.DlpmError, match='256 needed'):
        _lib.check(call(ws_bytes=255))
    assert L.dlpm_toy_workspace_bytes(8) == 256 and L.dlpm_toy_workspace_bytes(0) < 0 and L.dlpm_toy_workspace_bytes(-2) < 0
    assert buf.sum() == 0


def test_no_cpu_fallback():
    with pytest.raises(_lib.DlpmError, match='no CPU fallback'):
        datasets.sample_2_gmm(8, std=0.1, theta=3.0, device='cpu')
    with pytest.raises(_lib.DlpmError, match='no CPU fallback'):
        datasets.sample_2_gmm(8, std=0.1, raw=np.zeros((8, 2), np.float32), device='cpu', normalize=True)


# ---------------------------------------------------------------- Generator, get_dataset, the loader, load_original_data
def test_generator_interface():
    G = dlpm_amd.Generator
    assert G.available_distributions == ['gmm_2', 'gmm_grid', 'swiss_roll', 'sas_grid']
    g = G('gmm_grid', n=3, std=0.1)
    assert g.generator is datasets.sample_grid_gmm and g.samples is None and len(g) == 0
    assert G('gmm_2').generator is datasets.sample_2_gmm and G('swiss_roll').generator is datasets.gen_swiss_roll
    assert G('sas_grid').generator is datasets.sample_grid_sas
    g.setParams(std=0.2, weights=WEIGHTS)
    assert g.kwargs == dict(n=3, std=0.2, weights=WEIGHTS)
    h = G('gmm_grid', None, 100, None, 3)
    h.setParams(None, 1.7, None, 0.5)                    # positional slots: None keeps what is stored, extra values are dropped
    assert h.args == (100, 1.7, 3)
    with pytest.raises(Exception, match='without a parameter'):
        g.setParams()
    with pytest.raises(Exception, match='none are stored'):
        G('gmm_2').generate()
    for name in ('skewed_levy', 'sas'):
        with pytest.raises(NotImplementedError, match='dlpm_amd.process'):
            G(name)
    with pytest.raises(Exception, match='not a toy distribution'):
        G('rose')
    seen = {}
    g = G('gmm_grid', transform=lambda x: ('t', x), n=3)
    g.generator = lambda *a, **k: seen.update(a=a, k=k) or 'x'
    assert g.generate(n_samples=5, std=0.3) == ('t', 'x') == g.samples and seen == dict(a=(), k=dict(n=3, n_samples=5, std=0.3))
    assert g.kwargs == dict(n=3)
    import inspect
    for fn in (datasets.sample_2_gmm, datasets.sample_grid_gmm, datasets.gen_swiss_roll, datasets.sample_grid_sas):
        names = list(inspect.signature(fn).parameters)
        assert names[:11] == ['n_samples', 'alpha', 'n', 'std', 'theta', 'weights', 'device', 'normalize', 'isotropic', 'between_minus_1_1',
                              'quantile_cutoff'] and names[11:] == ['seed', 'first_index', 'raw', 'stream']


def test_config_describes_its_distribution_and_keeps_its_hash():
    p = dlpm_amd.load_config('2d_data')
    d = p['data']
    assert (d['dataset'], d['n_mixture'], d['std'], d['theta'], d['data_alpha']) == ('gmm_grid', 9, 0.1, 3.0, 1.7)
    assert d['weights'] == WEIGHTS and sum(d['weights']) <= 1 + 1e-12
    assert (d['normalized'], d['between_minus_1_1'], d['quantile_cutoff'], d['nsamples']) == (False, False, 1.0, 32000)
    assert (d['nfeatures'], d['dim'], d['isotropic']) == (2, 2, True)
    # the parent commit's values: the experiment hash reads dataset / channels / image_size only, checkpoints stay where they are
    assert dlpm_amd.checkpoint.get_exp_hash(p) == 'adf2a415ea922608' and dlpm_amd.checkpoint.get_eval_hash(p) == '639c4fed'


def test_get_dataset_refusals():
    p = dlpm_amd.load_config('2d_data')
    for change, err, word in [(dict(dim=3), ValueError, 'data.dim = 3'), (dict(dim=0), ValueError, 'data.dim = 0'), (dict(dataset='mnist'), ValueError, 'not available'),
                              (dict(dataset='rose'), ValueError, 'not available'), (dict(n_mixture=8), ValueError, 'perfect square'),
                              (dict(std=None), ValueError, 'data.std missing')]:
        q = dict(p, data=dict(p['data'], **change))
        with pytest.raises(err, match=word):
            dlpm_amd.get_dataset(q, 'cuda', 0)
    with pytest.raises(_lib.DlpmError, match='no CPU fallback'):
        dlpm_amd.get_dataset(p, 'cpu', 0)


def test_loader_and_load_original_data():
    data = torch.arange(10 * 2, dtype=torch.float32).reshape(10, 1, 2)
    loader = dlpm_amd.ToyLoader(data, 4)
    batches = list(loader)
    assert len(loader) == 3 == len(batches) and [len(b[0]) for b in batches] == [4, 4, 2]
    assert all(b[1].shape == (len(b[0]),) and not b[1].any() for b in batches)
    assert torch.equal(torch.cat([b[0] for b in batches]), data)
    gm = dlpm_amd.GenerationManager(None, loader, False)
    for n in (1, 3, 4, 5, 10):
        assert torch.equal(gm.load_original_data(n), data[:n])
    with pytest.raises(ValueError, match='holds 10 samples, 11 asked'):
        gm.load_original_data(11)
    probe = dlpm_amd.GenerationManager(None, dlpm_amd.ShapeProbe([1, 2]), False)
    for n in (1, 5):                                     # a shape probe carries no data: refused, not read
        with pytest.raises(ValueError, match='ShapeProbe.*ToyLoader'):
            probe.load_original_data(n)
    with pytest.raises(ValueError, match='ShapeProbe'):
        dlpm_amd.EvaluationManager(None, probe, None, verbose=False).evaluate_mmd({}, None, 1, 1, samples=torch.zeros(1, 1, 2))
    img = dlpm_amd.GenerationManager(None, loader, True)
    assert torch.equal(img.load_original_data(5), (data[:5] + 1) / 2)


# ---------------------------------------------------------------- F23
def test_sas_grid_bounds_are_the_references():
    t = golden('f23_toy_tables')
    assert t['weights'].tolist() == WEIGHTS
    for N in t['bound_sizes']:
        b = datasets.sas_grid_bounds(WEIGHTS, int(N))
        assert b.dtype == np.int64 and np.array_equal(b, t['bounds_%d' % N]) and b[0] == 0 and np.all(np.diff(b) >= 0) and b[-1] <= N
    assert t['bounds_32000'].tolist() == [0, 320, 3520, 13120, 19520, 20160, 24960, 25600, 30400, 32000]
    for key in ('cdf_1p7', 'cdf_1p0', 'cdf_2p0'):
        c = t[key]
        assert c.shape == (41,) and np.all(np.diff(c) >= 0) and abs(c[20] - 0.5) < 1e-3 and np.all(np.abs(c + c[::-1] - 1) < 2e-3)


@pytest.mark.parametrize('kind', KINDS)
def test_f23_pairs_are_consistent_under_numpy(kind):
    """Every processed array is the post-processing of its raw array: the clamp exactly (same order statistics, same fp32 operations),
    the normalisation within the bound DESIGN 3.16 derives for fp32 points against the reference's fp64 points (sas_grid: the measured
    bound), and exactly from swiss_roll's fp64 replay."""
    f = golden('f23_toy_' + kind)
    for N in SIZES:
        raw = f['raw_%d' % N]
        assert raw.shape == (N, 2) and raw.dtype == np.float32 and np.isfinite(raw).all()
        norm = f['norm_%d' % N]
        dev, m, s = np_normalize(raw, torch_std=kind == 'sas_grid')
        assert np.all(np.abs(dev.astype(np.float64) - norm) <= norm_bound(kind, dev, raw, m, s))
        if kind == 'swiss_roll':
            r64 = f['raw64_%d' % N]
            assert np.array_equal(r64.astype(np.float32), raw)
            assert np.array_equal(((r64 - r64.mean()) / r64.std()).astype(np.float32), norm)
        for tag, q, src in (('bt99', 0.99, raw), ('bt100', 1.0, raw), ('norm_bt99', 0.99, norm)):
            if int(f['%s_%d_raises' % (tag, N)]):
                assert kind == 'swiss_roll' or np_between(src, q)[1] != 0     # the reference's own sign asserts
                continue
            out, status, _ = np_between(src, q)
            assert status == 0 and np.array_equal(out, f['%s_%d' % (tag, N)])
            assert np.abs(out).max() == 1.0
    assert kind != 'gmm_2' or int(f['norm_bt99_64_raises'])          # the one-sided column the GPU test feeds the status word
