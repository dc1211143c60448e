"""Held-out LIM loss, the parts that need no GPU: the C ABI of the two entry points of include/dlpm_amd_lim.h, the refusals of
training_losses_lim / evaluate_loss / the CLI (all before any device work), the rng='reference' host draws against the reference's
recorded draws (F22), and a NumPy fp64 restatement (elements from the recorded coefficients, smooth-L1 per-sample mean, mean) that
reproduces every F22 case -- which pins that the reference's scalar smooth_l1_loss(reduction='mean') over B * D elements is the mean
of the per-sample means the kernels compute."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden
import dlpm_amd
from dlpm_amd import _lib

CASES = ['mlp', 'mlp_gauss', 'synth_odd', 'synth_long', 'tiny', 'tiny_b1', 'mnist']
T_SDE = 0.9946


def case(name):
    """(fixture, meta dict) of one F22 case."""
    f = golden('f22_limloss_' + name)
    B, alpha, clamp_eps = (float(v) for v in f['meta'])
    return f, dict(B=int(B), alpha=alpha, clamp_eps=None if clamp_eps < 0 else clamp_eps, seed=int(f['seed']))


def method_for(m, device='cpu', **kw):
    return dlpm_amd.GenerativeLevyProcess(m['alpha'], device, 100, rescale_timesteps=True, LIM=True, **kw)


def toy_model():
    torch.manual_seed(1)
    return dlpm_amd.MLPModel(dlpm_amd.load_config('2d_data'))


# ---------------------------------------------------------------- NumPy fp64 restatement
def np_coeffs(t, alpha):
    """VPSDE(alpha, 'cosine').diffusion_coeff / marginal_std in fp64 (LIM/functions/sde.py:35-47)."""
    t = np.asarray(t, np.float64)
    s = 0.008
    lm = np.log(np.cos((t + s) / (1 + s) * np.pi / 2)) - np.log(np.cos(s / (1 + s) * np.pi / 2))
    return np.exp(lm), (-np.expm1(alpha * lm)) ** (1 / alpha)


def np_elements(x0, e, x_coeff, sigma, alpha):
    """x_t and score in fp64 from fp32 inputs (loss.py:24-29)."""
    tail = (-1,) + (1,) * (x0.ndim - 1)
    x_t = x0.astype(np.float64) * x_coeff.astype(np.float64).reshape(tail) + e.astype(np.float64) * sigma.astype(np.float64).reshape(tail)
    score = -e.astype(np.float64) if alpha == 2.0 else -(e.astype(np.float64) / np.float64(np.float32(alpha)))
    return x_t, score


def np_terms(output, score):
    """Per-sample mean of smooth-L1 (beta = 1)."""
    d = (output.astype(np.float64) - score.astype(np.float64)).reshape(output.shape[0], -1)
    return np.where(np.abs(d) < 1, 0.5 * d * d, np.abs(d) - 0.5).mean(axis=1)


# ---------------------------------------------------------------- refusals of the C entry points
def test_c_entry_points_refuse_before_any_launch():
    """No GPU here: every one of these returns before a kernel is launched (the pointers are host addresses, never followed)."""
    L = _lib.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data

    def args(**o):
        a = _lib.LimLossArgs()
        a.x0_dev = a.x_t_dev = a.score_dev = a.tvec_out_dev = p
        a.B, a.D, a.alpha, a.clamp_eps, a.t_max = 2, 4, 1.7, -1.0, T_SDE
        for k, v in o.items():
            setattr(a, k, v)
        return a
    for o, word in [(dict(x0_dev=None), 'null pointer'), (dict(x_t_dev=None), 'null pointer'), (dict(score_dev=None), 'null pointer'),
                    (dict(tvec_out_dev=None), 'null pointer'), (dict(B=0), 'bad shape'), (dict(D=0), 'bad shape'), (dict(B=-3), 'bad shape'),
                    (dict(B=1 << 31), 'bad shape'), (dict(alpha=0.0), 'Wrong value of alpha'), (dict(alpha=2.5), 'Wrong value of alpha'),
                    (dict(t_max=1.0), 't_max'), (dict(t_max=0.0), 't_max'), (dict(x_coeff_dev=p), 'together'), (dict(sigma_dev=p), 'together')]:
        with pytest.raises(ValueError, match=word):
            _lib.check(L.dlpm_lim_loss_elements_f32(C.byref(args(**o)), None))
    with pytest.raises(ValueError, match='null pointer'):
        _lib.check(L.dlpm_lim_loss_elements_f32(None, None))
    for a, word in [((None, 4, 1.7, p, p), 'null pointer'), ((p, 4, 1.7, None, p), 'null pointer'), ((p, 4, 1.7, p, None), 'null pointer'),
                    ((p, 0, 1.7, p, p), 'bad shape'), ((p, 4, 2.1, p, p), 'Wrong value of alpha'), ((p, 4, 0.0, p, p), 'Wrong value of alpha')]:
        with pytest.raises(ValueError, match=word):
            _lib.check(L.dlpm_lim_coeffs_f32(*a, None))


# ---------------------------------------------------------------- refusals of the Python entry points
def test_a_lim_method_on_the_cpu_is_refused_first():
    """Before any other work and before the stateful setParams -- even arguments that would be refused themselves."""
    model = toy_model()
    x = torch.zeros(4, 1, 2)
    lim = method_for(dict(alpha=1.7))
    for call in (lambda: lim.training_losses({'default': model}, x, clamp_a=3.0, clamp_eps=5.0),
                 lambda: lim.training_losses_lim(model, x, clamp_a=3.0, clamp_eps=5.0),
                 lambda: lim.training_losses_lim(model, x, y=torch.zeros(4), noise={'bogus': 1})):
        with pytest.raises(NotImplementedError, match='training_losses_lim runs on the GPU only; there is no CPU fallback'):
            call()
    assert lim.dlpm.gen_a.get('clamp_a') is None and lim.dlpm.gen_eps.get('clamp_eps') is None
    ev = dlpm_amd.EvaluationManager(lim, None, None, verbose=False)
    with pytest.raises(NotImplementedError, match='no CPU fallback'):
        ev.evaluate_loss({'default': model}, x, 2)
    assert ev.evals['losses'].shape == (0,) and lim.calls == 0


def test_argument_checks_need_no_device():
    model = toy_model()
    x = torch.zeros(4, 1, 2)
    lim = method_for(dict(alpha=1.7))
    with pytest.raises(NotImplementedError, match=r'GenerativeLevyProcess\.py:706'):
        lim._lim_check_args(model, x, y=torch.zeros(4, dtype=torch.int64))
    net = dlpm_amd.UNetModel(1, 32, 1, 1, [2], channel_mult=[1, 2], num_heads=4, use_scale_shift_norm=True, num_classes=10)
    with pytest.raises(NotImplementedError, match=r'GenerativeLevyProcess\.py:706'):
        lim._lim_check_args(net, torch.zeros(4, 1, 16, 16))
    with pytest.raises(AssertionError, match='noise takes the keys'):
        lim._lim_check_args(model, x, noise={'t': torch.zeros(4), 'a': torch.ones(4)})
    with pytest.raises(AssertionError, match='noise takes the keys'):
        lim._lim_check_args(model, x, noise={'z': torch.zeros(4, 1, 2)})
    with pytest.raises(ValueError, match='together'):
        lim._lim_check_args(model, x, noise={'x_coeff': torch.ones(4)})
    with pytest.raises(ValueError, match='together'):
        lim._lim_check_args(model, x, noise={'sigma': torch.ones(4)})
    for bad in ({'t': torch.zeros(3)}, {'t': torch.zeros(4, 1)}, {'e': torch.zeros(4, 2)}, {'e': torch.zeros(3, 1, 2)},
                {'x_coeff': torch.ones(4), 'sigma': torch.ones(5)}):
        with pytest.raises(AssertionError, match='must'):
            lim._lim_check_args(model, x, noise=bad)
    with pytest.raises(AssertionError):
        lim._lim_check_args(model, torch.zeros(4, 1, 3))                     # not the MLP's feature count
    with pytest.raises(AssertionError, match='x_start must be'):
        lim._lim_check_args(model, torch.zeros(4))
    with pytest.raises(AssertionError, match='LIM=True'):
        dlpm_amd.GenerativeLevyProcess(1.7, 'cpu', 100, rescale_timesteps=True)._lim_check_args(model, x)
    ok = lim._lim_check_args(model, x, noise={'t': np.full(4, 0.5), 'e': None})
    assert set(ok) == {'t'} and ok['t'].dtype == torch.float32


def test_evaluate_loss_refuses_the_dlpm_keywords_by_name():
    model = toy_model()
    x = torch.zeros(4, 1, 2)
    ev = dlpm_amd.EvaluationManager(method_for(dict(alpha=1.7)), None, None, verbose=False)
    for kw in (dict(lploss=1.0), dict(loss_monte_carlo='median'), dict(monte_carlo_outer=3), dict(monte_carlo_inner=2),
               dict(loss_type='EPS_LOSS')):
        with pytest.raises(TypeError, match=list(kw)[0]):
            ev.evaluate_loss({'default': model}, x, 2, **kw)
    with pytest.raises(AssertionError, match='unknown loss arguments'):
        ev.evaluate_loss({'default': model}, x, 2, model_kwargs={})
    with pytest.raises(NotImplementedError, match=r'GenerativeLevyProcess\.py:706'):
        ev.evaluate_loss({'default': model}, x, 2, class_labels=[0, 1, 2, 3])
    assert ev.evals['losses'].shape == (0,)


@pytest.mark.parametrize('flags', [['--lploss', '1'], ['--median', '3', '2']])
def test_cli_refuses_the_dlpm_flags_with_method_lim(flags, tmp_path, capsys):
    from dlpm_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(['--config', '2d_data', '--method', 'lim', '--eval_loss', str(tmp_path / 'absent.npy')] + flags)
    assert e.value.code == 2 and '--lploss / --median' in capsys.readouterr().err


def test_signature_and_docstring():
    import inspect
    sig = [(p.name, p.default) for p in inspect.signature(dlpm_amd.GenerativeLevyProcess.training_losses_lim).parameters.values()]
    E = inspect.Parameter.empty
    assert sig == [('self', E), ('model', E), ('x_start', E), ('y', None), ('clamp_a', None), ('clamp_eps', None), ('noise', None),
                   ('return_terms', False), ('check_finite', True)]
    doc = dlpm_amd.GenerativeLevyProcess.training_losses_lim.__doc__
    assert 'fp64' in doc and '1.614e-4' in doc and '1.541e-4' in doc


# ---------------------------------------------------------------- rng='reference': the host draws
@pytest.mark.parametrize('name', CASES)
def test_reference_rng_host_draws_equal_the_recorded_draws(name):
    """z and t come from torch's own generator, a from the restated numpy stream + CMS, e = clamp(sqrt(a) z) from the correctly
    rounded fp32 root and torch's fp32 product: all four equal the recorded draws bit for bit on these seeds.  (torch.sqrt itself is
    not the same on every host's CPU: on one MI355X host sqrt(a) z formed with it from the RECORDED a and z missed the recorded e on
    12 of 64 elements of `mlp` and 554 of 1536 of `tiny`, while the recorded e is the product with the IEEE root in every case.)"""
    f, m = case(name)
    meth = method_for(m, rng='reference', seed=m['seed'])
    d = meth._lim_loss_host_draws(list(f['x_start'].shape), m['clamp_eps'])
    assert d['t'].dtype == torch.float32 and np.array_equal(d['t'].numpy(), f['t'])
    assert f['t'].min() >= 1e-5 and f['t'].max() < T_SDE
    assert np.array_equal(d['z'].numpy(), f['z'])
    if m['alpha'] == 2.0:
        assert d['a'] is None and 'a' not in f.files and np.array_equal(f['e'], f['z'])
    else:
        assert np.array_equal(d['a'].numpy(), f['a'])
    assert np.array_equal(d['e'].numpy(), f['e'])
    if m['clamp_eps'] is not None:
        assert (np.abs(f['e']) == m['clamp_eps']).any(), 'the clamp case does not clamp anything'
        assert np.abs(f['e']).max() == m['clamp_eps']


# ---------------------------------------------------------------- the fp64 restatement against every F22 case
@pytest.mark.parametrize('name', CASES)
def test_numpy_restatement_reproduces_the_reference(name):
    f, m = case(name)
    B = m['B']
    assert f['x_start'].shape[0] == B == f['t'].shape[0] == f['x_coeff'].shape[0] == f['sigma'].shape[0]
    x_t, score = np_elements(f['x_start'], f['e'], f['x_coeff'], f['sigma'], m['alpha'])
    # two fp32 products and one fp32 sum against fp64: three roundings of half an ulp each, of the two products and of the result.  (One
    # ulp of the RESULT cannot hold where the products cancel -- the recorded tensors are up to 1e4 ulps of x_t from fp64 there -- and
    # one ulp of the largest of the three magnitudes is missed by the reference itself, by up to 1.22; the sum of the three half
    # ulps is the rigorous form of "one ulp" and is what the recorded tensors meet, at 0.90 - 0.99 of it.)
    tail = (-1,) + (1,) * (f['x_start'].ndim - 1)
    p1, p2 = f['x_start'] * f['x_coeff'].reshape(tail), f['e'] * f['sigma'].reshape(tail)
    bound = 0.5 * (np.spacing(np.abs(p1)).astype(np.float64) + np.spacing(np.abs(p2)) + np.spacing(np.abs(f['x_t'])))
    assert p1.dtype == np.float32 and (np.abs(f['x_t'] - x_t) <= bound).all()
    assert (np.abs(f['score'] - score) <= np.spacing(np.abs(f['score']).astype(np.float32))).all()
    # the recorded score IS -(e / float32(alpha)) in fp32, bit for bit (asserted by the tool when it recorded)
    want = -f['e'] if m['alpha'] == 2.0 else -(f['e'] / np.float32(m['alpha']))
    assert want.dtype == np.float32 and np.array_equal(f['score'], want)
    # F.smooth_l1_loss(reduction='mean') over B * D elements == the mean of the per-sample means
    terms = np_terms(f['output'], f['score'])
    assert abs(float(f['loss']) - terms.mean()) <= 2e-7 * abs(float(f['loss']))
    # the recorded coefficients against fp64: diffusion_coeff within 2e-5 (what the issue measured, 1.8e-5), marginal_std within
    # 12 % -- the fp32 evaluation's own error, the reason the coefficients are inputs
    cx, sg = np_coeffs(f['t'], m['alpha'])
    np.testing.assert_allclose(f['x_coeff'], cx, rtol=2e-5)
    np.testing.assert_allclose(f['sigma'], sg, rtol=0.12)
    # the host's own evaluation (lim.VPSDE, torch ops) on the recorded times: what rng='reference' passes to the kernel
    sde = method_for(m).sde
    t = torch.from_numpy(f['t'])
    same = (sde.marginal_std(t).numpy() == f['sigma']) & (sde.diffusion_coeff(t).numpy() == f['x_coeff'])
    print('%s: host coefficients equal the recorded ones on %d of %d samples' % (name, same.sum(), B))
