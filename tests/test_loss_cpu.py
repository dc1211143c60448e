"""Held-out denoising loss, the parts that need no GPU: the refusals of the loss entry points, the argument checks of
training_losses (all before any device work), the rng='reference' host draws against the reference's recorded draws (F17),
and a NumPy fp64 restatement of the three steps (elements, terms, estimator) that reproduces every F17 case -- which pins the
reference's index quirk (replica r reads a[(r mod outer) * B + b], the estimator reads [outer, inner, B]) and the lower
median independently of the kernels."""
import numpy as np
import pytest
import torch

from conftest import golden
import dlpm_amd
from dlpm_amd import _lib

CASES = ['mlp_l2', 'mlp_l1', 'mlp_sq', 'mlp_median', 'tiny_l2', 'tiny_l1', 'tiny_sq', 'tiny_median', 'tiny_median_even',
         'tiny_clamp', 'tiny_noniso', 'tiny_exploding', 'mnist_l2', 'cond_l2']


def case(name):
    """(fixture, meta dict) of one F17 case."""
    f = golden('f17_loss_' + name)
    B, T, alpha, outer, inner, lploss, clamp_a, median, iso, exploding = (float(v) for v in f['meta'])
    m = dict(B=int(B), T=int(T), alpha=alpha, outer=int(outer), inner=int(inner), lploss=int(lploss),
             clamp_a=None if clamp_a < 0 else clamp_a, estimator='median' if median else 'mean', isotropic=bool(iso),
             scale='scale_exploding' if exploding else 'scale_preserving', input_scaling=bool(exploding), seed=int(f['seed']))
    return f, m


def method_for(m, device='cpu', **kw):
    return dlpm_amd.GenerativeLevyProcess(m['alpha'], device, m['T'], rescale_timesteps=True, isotropic=m['isotropic'],
                                          scale=m['scale'], input_scaling=m['input_scaling'], **kw)


def loss_kwargs(m):
    return dict(lploss=m['lploss'], loss_monte_carlo=m['estimator'], monte_carlo_outer=m['outer'], monte_carlo_inner=m['inner'],
                clamp_a=m['clamp_a'])


# ---------------------------------------------------------------- NumPy fp64 restatement of the three steps
def np_elements(x0, t, A, z, bg, bs, outer, inner, in_scale=None):
    """Step 1.  x0 [B, ...], t [B], A as drawn ([outer*B] or [outer*B, ...]), z [outer*inner*B, ...] -> x_t, eps_t, x_in (fp64)."""
    B = x0.shape[0]
    R = outer * inner
    tail = (1,) * (x0.ndim - 1)
    x0e = np.tile(x0.astype(np.float64), (R,) + tail)                    # x_start.repeat
    te = np.tile(t, R)                                                   # t.repeat
    A = A.astype(np.float64).reshape((outer * B,) + (tail if A.ndim == 1 else x0.shape[1:]))
    Ae = np.tile(A, (inner,) + tail)                                     # A.repeat(inner): extended sample j reads a[j mod (outer*B)]
    bge, bse = (v.astype(np.float64)[te].reshape((-1,) + tail) for v in (bg, bs))
    x_t = bge * x0e + np.sqrt(Ae * bse ** 2) * z.astype(np.float64)
    eps = (x_t - x0e * bge) / bse
    x_in = x_t if in_scale is None else x_t * in_scale.astype(np.float64)[te].reshape((-1,) + tail)
    return x_t, eps, x_in


def np_terms(model_eps, eps_t, lploss):
    """Step 2 (compute_loss_terms)."""
    d = model_eps.astype(np.float64) - eps_t.astype(np.float64)
    d = d.reshape(d.shape[0], -1)
    if lploss == 2:
        return np.sqrt((d * d).mean(axis=1))
    if lploss == 1:
        return np.where(np.abs(d) < 1, 0.5 * d * d, np.abs(d) - 0.5).mean(axis=1)
    assert lploss == -1
    return (d * d).mean(axis=1)


def np_reduce(terms, B, outer, inner, estimator):
    """Step 3.  Returns (loss, index of the chosen outer mean per sample or None)."""
    terms = np.asarray(terms, np.float64)
    if estimator == 'mean':
        return terms.mean(), None
    means = terms.reshape(outer, inner, B).mean(axis=1)                  # [outer, B]
    order = np.argsort(means, axis=0, kind='stable')
    at = order[(outer - 1) // 2]                                         # the LOWER of the two middle values (torch.median)
    return means[at, np.arange(B)].mean(), at


def host_schedule(m):
    bg, bs = (v.numpy() for v in dlpm_amd.DLPM(m['alpha'], 'cpu', m['T'], scale=m['scale']).host_schedule[1::2])
    return bg, bs


# ---------------------------------------------------------------- refusals of the C entry points
def test_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes as C
    L = _lib.lib()
    a = _lib.LossArgs()
    with pytest.raises(ValueError, match='null pointer'):
        _lib.check(L.dlpm_loss_elements_f32(C.byref(a), None))
    with pytest.raises(ValueError, match='lploss must be 2, 1 or -1'):
        _lib.check(L.dlpm_loss_terms_f32(8, 8, 8, 1, 1, 4, 3, 1, 0, None))
    with pytest.raises(ValueError, match='outside the row stride'):
        _lib.check(L.dlpm_loss_terms_f32(8, 8, 8, 4, 1, 4, 2, 6, 3, None))
    with pytest.raises(ValueError, match='monte_carlo_outer <= 64'):
        _lib.check(L.dlpm_loss_reduce_f32(8, 4, 65, 1, 1, 8, 8, None, None))
    with pytest.raises(ValueError, match='unknown mode'):
        _lib.check(L.dlpm_at_t_f32(3, 8, 8, 8, 8, 8, 8, 1, 1, 2, None))


# ---------------------------------------------------------------- argument checks of the Python entry points
def toy_model():
    torch.manual_seed(1)
    return dlpm_amd.MLPModel(dlpm_amd.load_config('2d_data'))


def test_argument_checks_fire_before_device_work():
    model = toy_model()
    x = torch.zeros(4, 1, 2)
    m = dlpm_amd.GenerativeLevyProcess(1.7, 'cpu', 100, rescale_timesteps=True)
    with pytest.raises(ValueError, match='lploss'):
        m.training_losses({'default': model}, x, lploss=1.5)
    with pytest.raises(AssertionError, match='only epsilon loss is supported for the moment'):
        m.training_losses({'default': model}, x, loss_type='VAR_KL')
    with pytest.raises(AssertionError, match='only epsilon loss is supported for the moment'):
        m.training_losses({'default': model}, x, loss_type='EPSILON')          # the reference's own default fails its assertion
    with pytest.raises(ValueError, match='monte_carlo_outer <= 64'):
        m.training_losses({'default': model}, x, loss_monte_carlo='median', monte_carlo_outer=65)
    with pytest.raises(_lib.DlpmError, match='no CPU fallback'):
        m.training_losses({'default': model}, x)
    with pytest.raises(_lib.DlpmError, match='no CPU fallback'):
        m.training_losses_dlpm(model, x)
    m2 = dlpm_amd.GenerativeLevyProcess(1.7, 'cpu', 100, rescale_timesteps=True, model_mean_type='START_X')
    with pytest.raises(AssertionError, match='only epsilon model output is supported for the moment'):
        m2.training_losses({'default': model}, x)
    lim = dlpm_amd.GenerativeLevyProcess(1.7, 'cpu', 100, rescale_timesteps=True, LIM=True)
    with pytest.raises(NotImplementedError, match='training_losses_lim'):
        lim.training_losses({'default': model}, x)
    # the stateful setParams happens only once the checks have passed
    assert m.dlpm.gen_a.get('clamp_a') is None
    with pytest.raises(_lib.DlpmError):
        m.dlpm.predict_eps(x, 3, x)


def test_conditional_label_checks_fire_before_device_work():
    net = dlpm_amd.UNetModel(1, 32, 1, 1, [2], channel_mult=[1, 2], num_heads=4, use_scale_shift_norm=True, num_classes=10)
    m = dlpm_amd.GenerativeLevyProcess(1.7, 'cpu', 100, rescale_timesteps=True)
    x = torch.zeros(4, 1, 16, 16)
    with pytest.raises(AssertionError, match='if and only if'):
        m.training_losses({'default': net}, x)
    with pytest.raises(IndexError):
        m.training_losses({'default': net}, x, model_kwargs={'y': torch.tensor([0, 1, 2, 10])})
    with pytest.raises(IndexError):                                             # the nested form of a reference caller
        m.training_losses({'default': net}, x, model_kwargs={'model_kwargs': {'y': torch.tensor([0, 1, 2, 10])}})


# ---------------------------------------------------------------- rng='reference': the host draws
@pytest.mark.parametrize('name', CASES)
def test_reference_rng_host_draws_equal_the_recorded_draws(name):
    """t and z come from torch's own generator (exact); A from the restated numpy stream + CMS, held to the bounds
    test_host_skewed_levy_stream holds it to."""
    f, m = case(name)
    meth = method_for(m, rng='reference', seed=m['seed'])
    d = meth._loss_host_draws(list(f['x_start'].shape), m['outer'], m['inner'], m['clamp_a'])
    assert d['t'].dtype == torch.int64 and np.array_equal(d['t'].numpy(), f['t'])
    assert f['t'].min() >= 1 and f['t'].max() <= m['T'] - 1
    A = d['a'].numpy().reshape(f['A'].shape)
    np.testing.assert_allclose(A, f['A'], rtol=2e-7)
    assert (A == f['A']).mean() > 0.99
    assert np.array_equal(d['z'].numpy(), f['z'])
    if m['clamp_a'] is not None:
        assert (f['A'] == m['clamp_a']).any(), 'the clamp case does not clamp anything'


# ---------------------------------------------------------------- the fp64 restatement against every F17 case
@pytest.mark.parametrize('name', CASES)
def test_numpy_restatement_reproduces_the_reference(name):
    f, m = case(name)
    B, outer, inner = m['B'], m['outer'], m['inner']
    bg, bs = host_schedule(m)
    isc = (1 / (1 + torch.from_numpy(bs))).numpy() if m['input_scaling'] else None
    assert f['A'].shape[0] == outer * B and f['z'].shape[0] == outer * inner * B == f['losses'].shape[0]
    # step 1: fp64 against the recorded fp32 tensors.  x_t is a sum of two products: 3 roundings of <= 2^-24 relative to the
    # larger operand; eps_t divides a cancelling difference of x_t by bs[t], so it is held against the RECORDED x_t
    x_t, eps, x_in = np_elements(f['x_start'], f['t'], f['A'], f['z'], bg, bs, outer, inner, isc)
    u = 2.0 ** -24
    tail = (1,) * (f['x_start'].ndim - 1)
    te = np.tile(f['t'], outer * inner)
    bge, bse = (v.astype(np.float64)[te].reshape((-1,) + tail) for v in (bg, bs))
    x0e = np.tile(f['x_start'].astype(np.float64), (outer * inner,) + tail)
    mag = np.abs(bge * x0e) + np.abs(x_t - bge * x0e)
    assert (np.abs(f['x_t'] - x_t) <= 4 * u * mag + 1e-30).all()
    eps_from_recorded = (f['x_t'].astype(np.float64) - x0e * bge) / bse
    assert (np.abs(f['eps_t'] - eps_from_recorded) <= 4 * u * (np.abs(f['x_t']) + np.abs(bge * x0e)) / bse + 1e-30).all()
    want_in = f['x_t'].astype(np.float64) * (1.0 if isc is None else isc.astype(np.float64)[te].reshape((-1,) + tail))
    np.testing.assert_allclose(f['x_in'], want_in, rtol=2 * u)
    np.testing.assert_allclose(f['t_in'], te.astype(np.float32) * np.float32(1.0 / m['T']), rtol=0, atol=0)
    # step 2: a sum of D <= 1024 * 3 non-negative fp32 terms carries <= (log2 D + 3) 2^-24 ~ 1e-6 relative error
    terms = np_terms(f['model_eps'], f['eps_t'], m['lploss'])
    np.testing.assert_allclose(f['losses'], terms, rtol=2e-6)
    # step 3
    loss, at = np_reduce(f['losses'], B, outer, inner, m['estimator'])
    np.testing.assert_allclose(float(f['loss']), loss, rtol=1e-6)
    if at is not None:
        means32 = torch.from_numpy(f['losses']).reshape(outer, inner, B).mean(dim=1)
        vals, idx = means32.median(dim=0)
        assert np.array_equal(idx.numpy(), at)
        if outer % 2 == 0:                     # the lower of the two middle values, not their average
            srt = np.sort(means32.numpy(), axis=0)
            assert np.array_equal(vals.numpy(), srt[outer // 2 - 1])
