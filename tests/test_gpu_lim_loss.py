"""Held-out LIM loss on the MI355X: k_lim_loss_elements against the reference's recorded tensors (F22), the fp64 coefficients against
NumPy, the reused terms / estimator kernels on the recorded model output, the whole training_losses call against the reference for
every conv generation x GEMM pipe, rng='reference', the Philox draws (statistics, composition over chunks / offsets / evaluate_loss),
graph capture, a generic callable and the CLI."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dlpm_amd
from dlpm_amd import _lib
from dlpm_amd.method import ReferenceStreams
from dlpm_amd.weights import state_digest
from test_host_mirror import build_unet
from test_gpu_cond import GENERATIONS
from test_lim_loss_cpu import CASES, T_SDE, case, method_for, np_coeffs, np_terms

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FORWARD_CONTRACT = 1e-4        # max |eps - eps_ref| of a forward (tests/test_gpu_models.py)
MLP_CASES = ['mlp', 'mlp_gauss']
SYNTH_CASES = ['synth_odd', 'synth_long']
UNET_CASES = ['tiny', 'tiny_b1', 'mnist']


def net_for(name):
    if name.startswith('mlp'):
        torch.manual_seed(1)
        return dlpm_amd.MLPModel(dlpm_amd.load_config('2d_data'))
    if name.startswith('synth'):
        return synth_model
    return build_unet('mnist' if name.startswith('mnist') else 'tiny')[0]


def synth_model(x, t):
    """The synthetic callable the synth cases were recorded with: 0.5 x + t."""
    return 0.5 * x + t.view(-1, *([1] * (x.dim() - 1)))


def zero_model(x, t):
    return torch.zeros_like(x)


def injected(f, coeffs=True):
    keys = ('t', 'e', 'x_coeff', 'sigma') if coeffs else ('t', 'e')
    return {k: torch.from_numpy(f[k]) for k in keys}


def raw_elements(B, D, alpha, seed, offset=0, clamp_eps=-1.0, x0=None, t=None, e=None, x_coeff=None, sigma=None):
    """dlpm_lim_loss_elements_f32 itself; what is not given comes from Philox / the fp64 evaluation.  Host arrays back."""
    dev = lambda v: None if v is None else torch.as_tensor(v, dtype=torch.float32).contiguous().to(DEV)      # noqa: E731
    x0 = torch.zeros(B, D, device=DEV) if x0 is None else dev(x0)
    t, e, x_coeff, sigma = dev(t), dev(e), dev(x_coeff), dev(sigma)
    out = {k: torch.empty(B, D, device=DEV) for k in ('x_t', 'score', 'e')}
    out.update({k: torch.empty(B, device=DEV) for k in ('t', 'a', 'x_coeff', 'sigma')})
    a = _lib.LimLossArgs()
    a.x0_dev, a.t_dev, a.e_dev, a.x_coeff_dev, a.sigma_dev = x0.data_ptr(), _lib.ptr(t), _lib.ptr(e), _lib.ptr(x_coeff), _lib.ptr(sigma)
    a.x_t_dev, a.score_dev, a.tvec_out_dev = out['x_t'].data_ptr(), out['score'].data_ptr(), out['t'].data_ptr()
    a.a_out_dev, a.e_out_dev = out['a'].data_ptr(), out['e'].data_ptr()
    a.x_coeff_out_dev, a.sigma_out_dev = out['x_coeff'].data_ptr(), out['sigma'].data_ptr()
    a.B, a.D, a.alpha, a.clamp_eps, a.t_max, a.seed, a.sample_offset = B, D, alpha, clamp_eps, T_SDE, seed, offset
    _lib.check(_lib.lib().dlpm_lim_loss_elements_f32(C.byref(a), _lib.stream_ptr()))
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---------------------------------------------------------------- 1. elements, everything injected: bit-exact
@pytest.mark.parametrize('name', CASES)
def test_elements_with_injected_draws_and_coefficients_are_bit_exact(name):
    """Two products, a sum and a division, each correctly rounded in the reference's order; nothing transcendental."""
    f, m = case(name)
    meth = method_for(m, DEV)
    x = torch.from_numpy(f['x_start']).to(DEV)
    with torch.inference_mode():
        r = meth._lim_loss_terms(zero_model, x, m['clamp_eps'], meth._lim_check_args(zero_model, x, noise=injected(f)), keep=True)
    for key, want in (('x_t', f['x_t']), ('score', f['score']), ('t', f['t']), ('e', f['e']), ('x_coeff', f['x_coeff']), ('sigma', f['sigma'])):
        got = r[key].cpu().numpy()
        print('%s %s: %d of %d elements differ' % (name, key, (got != want).sum(), got.size))
        assert np.array_equal(got, want), key
    assert (r['a'].cpu().numpy() == 1).all()          # nothing was drawn


# ---------------------------------------------------------------- 2. the fp64 coefficients
def coefficient_times():
    g = np.random.default_rng(2)
    t = np.concatenate([[1e-5, T_SDE], np.geomspace(1e-5, 1e-2, 1022), g.uniform(1e-5, T_SDE, 4096 - 1024)]).astype(np.float32)
    assert t.shape == (4096,) and t[0] == np.float32(1e-5) and t[1] == np.float32(0.9946)
    return t


@pytest.mark.parametrize('alpha', [1.2, 1.5, 1.7, 2.0])
def test_in_kernel_coefficients_against_fp64_numpy(alpha):
    """dlpm_lim_coeffs_f32 against the fp64 NumPy formula on the same fp32 times at rtol 1.2e-7: one fp32 rounding of an fp64 result.
    The elements kernel with null coefficient pointers gives the same bits as with these arrays injected."""
    t = coefficient_times()
    t_d = torch.from_numpy(t).to(DEV)
    cx, sg = torch.empty(4096, device=DEV), torch.empty(4096, device=DEV)
    _lib.check(_lib.lib().dlpm_lim_coeffs_f32(t_d.data_ptr(), 4096, alpha, cx.data_ptr(), sg.data_ptr(), _lib.stream_ptr()))
    cx, sg = cx.cpu().numpy(), sg.cpu().numpy()
    want_cx, want_sg = np_coeffs(t, alpha)
    print('alpha %g: max rel err x_coeff %.3g, sigma %.3g' % (alpha, np.abs(cx / want_cx - 1).max(), np.abs(sg / want_sg - 1).max()))
    np.testing.assert_allclose(cx, want_cx, rtol=1.2e-7, atol=0)
    np.testing.assert_allclose(sg, want_sg, rtol=1.2e-7, atol=0)
    g = np.random.default_rng(3)
    for D in (5, 8):                       # the scalar and the 16-byte path
        x0, e = g.standard_normal((4096, D)).astype(np.float32), g.standard_normal((4096, D)).astype(np.float32)
        own = raw_elements(4096, D, alpha, 1, x0=x0, t=t, e=e)
        given = raw_elements(4096, D, alpha, 1, x0=x0, t=t, e=e, x_coeff=cx, sigma=sg)
        assert np.array_equal(own['x_coeff'], cx) and np.array_equal(own['sigma'], sg)
        assert np.array_equal(own['x_t'], given['x_t']) and np.array_equal(own['score'], given['score'])
        assert np.array_equal(own['x_t'], x0 * cx[:, None] + e * sg[:, None])


# ---------------------------------------------------------------- 3. terms and loss from the recorded output
@pytest.mark.parametrize('name', CASES)
def test_terms_and_loss_from_the_recorded_output(name):
    """Through the reused entry points, at the tolerances tests/test_gpu_loss.py holds lploss = 1 to: terms rtol 2e-6 against fp64, the
    estimator rtol 1e-6."""
    f, m = case(name)
    out, score = torch.from_numpy(f['output']).to(DEV), torch.from_numpy(f['score']).to(DEV)
    B = m['B']
    terms = torch.empty(B, device=DEV)
    _lib.check(_lib.lib().dlpm_loss_terms_f32(out.data_ptr(), score.data_ptr(), terms.data_ptr(), B, 1, out[0].numel(), 1, B, 0,
                                              _lib.stream_ptr()))
    want = np_terms(f['output'], f['score'])
    np.testing.assert_allclose(terms.cpu().numpy(), want, rtol=2e-6)
    loss = method_for(m, DEV)._loss_reduce(terms, B, 1, 1, 'mean', True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    np.testing.assert_allclose(float(loss), want.mean(), rtol=1e-6)
    np.testing.assert_allclose(float(loss), float(f['loss']), rtol=1e-6)


# ---------------------------------------------------------------- 4. end to end against the reference
def run_case(name, net, **kw):
    f, m = case(name)
    meth = method_for(m, DEV, **kw)
    x = torch.from_numpy(f['x_start']).to(DEV)
    out = meth.training_losses({'default': net}, x, noise=injected(f), clamp_eps=m['clamp_eps'])
    meth.close()
    return f, m, out


def check_against_reference(tag, f, m, out):
    """|loss - ref| <= FORWARD_CONTRACT + 1e-6 |ref|: smooth-L1 is 1-Lipschitz, so a forward within 1e-4 moves no term by more, and the
    rest is fp32 summation.  The terms are held to the same bound against the fp64 restatement on the reference's recorded output."""
    assert set(out) == {'loss', 'losses', 't'} and out['loss'].dim() == 0 and out['loss'].is_cuda and not out['loss'].requires_grad
    assert out['losses'].shape == (m['B'],) and out['t'].dtype == torch.float32 and np.array_equal(out['t'].cpu().numpy(), f['t'])
    want = np_terms(f['output'], f['score'])
    err = np.abs(out['losses'].cpu().numpy().astype(np.float64) - want)
    err_loss = abs(float(out['loss']) - float(f['loss']))
    print('%s: max |term - reference| = %.3g, |loss - reference| = %.3g' % (tag, err.max(), err_loss))
    assert (err <= FORWARD_CONTRACT + 1e-6 * np.abs(want)).all()
    assert err_loss <= FORWARD_CONTRACT + 1e-6 * abs(float(f['loss']))


@pytest.mark.parametrize('name', MLP_CASES + SYNTH_CASES)
def test_training_losses_against_reference_mlp_and_callable(name):
    net = net_for(name)
    f, m, out = run_case(name, net)
    if 'digest' in f.files:
        assert state_digest(net) == bytes(f['digest']).hex()
    check_against_reference(name, f, m, out)


@pytest.mark.parametrize('gemm', ['bf16x3', 'f32'])
@pytest.mark.parametrize('gen', GENERATIONS)
@pytest.mark.parametrize('name', UNET_CASES)
def test_training_losses_against_reference_unet(name, gen, gemm):
    net = net_for(name)
    net.set_conv_policy(gen)
    net.set_gemm_policy(gemm)
    f, m, out = run_case(name, net)
    assert state_digest(net) == bytes(f['digest']).hex()
    check_against_reference('%s (%s, %s)' % (name, gen, gemm), f, m, out)


def test_direct_call_and_coefficients_from_a_host_t():
    """training_losses_lim itself; and with only t and e injected (host tensors) the coefficients come from the host's torch ops."""
    f, m = case('mlp')
    net = net_for('mlp')
    x = torch.from_numpy(f['x_start']).to(DEV)
    loss, terms, t = method_for(m, DEV).training_losses_lim(net, x, noise=injected(f), return_terms=True)
    assert float(loss) == pytest.approx(float(terms.mean(dtype=torch.float64)), rel=1e-6) and np.array_equal(t.cpu().numpy(), f['t'])
    assert torch.equal(method_for(m, DEV).training_losses_lim(net, x, noise=injected(f)), loss)
    meth = method_for(m, DEV)
    loss2 = meth.training_losses_lim(net, x, noise=injected(f, coeffs=False))
    t_host = torch.from_numpy(f['t'])
    if np.array_equal(meth.sde.marginal_std(t_host).numpy(), f['sigma']) and np.array_equal(meth.sde.diffusion_coeff(t_host).numpy(), f['x_coeff']):
        assert torch.equal(loss2, loss)                     # this host's torch evaluates the coefficients as the recording one did
    assert math.isfinite(float(loss2))
    with pytest.raises(NotImplementedError, match=r'GenerativeLevyProcess\.py:706'):
        method_for(m, DEV).training_losses({'default': net}, x, model_kwargs={'y': torch.zeros(m['B'], dtype=torch.int64)})


# ---------------------------------------------------------------- 5. rng='reference', nothing injected
@pytest.mark.parametrize('name', ['mlp', 'tiny'])
def test_reference_rng_end_to_end(name):
    """Same seeds as the fixture: the draws are the recorded ones, the coefficients come from this host's torch ops.  The loss is held
    to the end-to-end bound; the net input is compared with F22's x_t bit for bit on the samples whose host-computed coefficients
    equal the recorded ones bit for bit.  The share of samples left out by that rule is capped at 10 %, and the cap is a condition
    of the test: a host whose torch differs beyond it fails here, which is a finding about that host's torch."""
    f, m = case(name)
    net = net_for(name)
    seen = {}

    def recording(x, t):
        seen['x'], seen['t'] = x.clone(), t.clone()
        return net(x, t)
    x = torch.from_numpy(f['x_start']).to(DEV)
    meth = method_for(m, DEV, rng='reference', seed=m['seed'])
    out = meth.training_losses({'default': recording}, x, clamp_eps=m['clamp_eps'])
    assert np.array_equal(out['t'].cpu().numpy(), f['t']) and np.array_equal(seen['t'].cpu().numpy(), f['t'])
    t = torch.from_numpy(f['t'])
    same = (meth.sde.marginal_std(t).numpy() == f['sigma']) & (meth.sde.diffusion_coeff(t).numpy() == f['x_coeff'])
    left_out = 1 - same.mean()
    print("%s rng='reference': host coefficients differ from the recorded ones on %d of %d samples" % (name, (~same).sum(), same.size))
    assert left_out <= 0.10
    assert np.array_equal(seen['x'].cpu().numpy()[same], f['x_t'][same])
    err_loss = abs(float(out['loss']) - float(f['loss']))
    print("%s rng='reference': |loss - reference| = %.3g" % (name, err_loss))
    assert err_loss <= FORWARD_CONTRACT + 1e-6 * abs(float(f['loss']))


# ---------------------------------------------------------------- 6. Philox draws
def test_philox_draw_statistics():
    n, D = 16384, 4
    g2 = raw_elements(n, D, 2.0, seed=123)
    t = g2['t']
    assert t.dtype == np.float32 and (t >= np.float32(1e-5)).all() and (t.astype(np.float64) < T_SDE).all()
    assert abs(t.astype(np.float64).mean() - (T_SDE + 1e-5) / 2) <= 5 * (T_SDE / math.sqrt(12)) / math.sqrt(n)
    assert len(np.unique(t)) > 0.99 * n
    # alpha = 2: e = z, not sqrt(2) z; the std of n D normals has standard error 1 / sqrt(2 n D)
    assert abs(g2['e'].astype(np.float64).std() - 1) <= 5 / math.sqrt(2 * n * D)
    assert (g2['a'] == 1).all() and np.array_equal(g2['score'], -g2['e'])
    # the clamp
    c = raw_elements(n, D, 1.7, seed=123, clamp_eps=3.0)
    assert np.abs(c['e']).max() == 3.0 and (c['e'] == 3.0).any() and (c['e'] == -3.0).any()
    # alpha = 1.7: one unclamped a per sample, its median between the 0.5 +- 5 * 0.5 / sqrt(n) quantiles of 1e6 host CMS draws
    h = raw_elements(n, D, 1.7, seed=123)
    a = h['a'].astype(np.float64)
    assert (a > 0).all() and np.isfinite(a).all()
    host = ReferenceStreams(0, 0).skewed_levy(1.7, 10 ** 6).numpy().astype(np.float64)
    lo, hi = np.quantile(host, [0.5 - 5 * 0.5 / math.sqrt(n), 0.5 + 5 * 0.5 / math.sqrt(n)])
    print('median a = %.5f, host quantiles [%.5f, %.5f]' % (np.median(a), lo, hi))
    assert lo <= np.median(a) <= hi
    assert np.array_equal(h['t'], t) and np.array_equal(c['t'], t)              # the time does not depend on alpha or the clamp
    assert np.array_equal(h['score'], -(h['e'] / np.float32(1.7)))
    # determinism, seeds, offsets, and the scalar path drawing what the 16-byte path draws
    again = raw_elements(n, D, 1.7, seed=123)
    assert all(np.array_equal(h[k], again[k]) for k in h)
    other = raw_elements(n, D, 1.7, seed=124)
    assert not np.array_equal(h['t'], other['t']) and not np.array_equal(h['e'], other['e']) and not np.array_equal(h['a'], other['a'])
    tail = raw_elements(n - 100, D, 1.7, seed=123, offset=100)
    assert all(np.array_equal(h[k][100:], tail[k]) for k in h)
    odd = raw_elements(64, 7, 1.7, seed=123)
    even = raw_elements(64, 8, 1.7, seed=123)
    assert np.array_equal(odd['e'], even['e'][:, :7]) and np.array_equal(odd['a'], even['a'])


# ---------------------------------------------------------------- 7. composition
def test_philox_composition_over_offsets_chunks_and_evaluate_loss():
    net = build_unet('tiny')[0]
    x = 0.5 * torch.randn(64, 3, 16, 16, generator=torch.Generator().manual_seed(3))

    def method(offset=0):
        return dlpm_amd.GenerativeLevyProcess(1.7, DEV, 100, rescale_timesteps=True, LIM=True, seed=21, sample_offset=offset)
    whole = method().training_losses({'default': net}, x.to(DEV), clamp_eps=20)
    lo = method(0).training_losses({'default': net}, x[:32].to(DEV), clamp_eps=20)
    hi = method(32).training_losses({'default': net}, x[32:].to(DEV), clamp_eps=20)
    assert torch.equal(whole['losses'], torch.cat([lo['losses'], hi['losses']]))
    assert torch.equal(whole['t'], torch.cat([lo['t'], hi['t']]))
    x7 = x[:7]
    want = method().training_losses_lim(net, x7.to(DEV), clamp_eps=20, return_terms=True)
    figures = []
    for bs in (7, 3, 1):
        ev = dlpm_amd.EvaluationManager(method(), None, None, verbose=False)
        loss, t, terms = ev.evaluate_loss({'default': net}, x7, bs, per_timestep=True, clamp_eps=20)
        assert torch.equal(terms, want[1].cpu()) and torch.equal(t, want[2].cpu()) and t.dtype == torch.float32
        assert isinstance(loss, float) and ev.evals['losses'].shape == (1,) and float(ev.evals['losses'][0]) == loss
        figures.append(loss)
    assert figures[0] == figures[1] == figures[2] == float(want[0])
    assert ev.evaluate_loss({'default': net}, x7, 4, clamp_eps=20) != figures[0] and ev.evals['losses'].shape == (2,)      # a second pass draws afresh


def test_second_call_draws_fresh_noise_and_the_key_reproduces():
    net = net_for('mlp')
    x = torch.randn(32, 1, 2, generator=torch.Generator().manual_seed(4)).to(DEV)
    m = dlpm_amd.GenerativeLevyProcess(1.8, DEV, 100, rescale_timesteps=True, LIM=True, seed=5)
    a = m.training_losses({'default': net}, x)
    b = m.training_losses({'default': net}, x)
    assert m.calls == 2 and not torch.equal(a['losses'], b['losses']) and not torch.equal(a['t'], b['t'])
    m2 = dlpm_amd.GenerativeLevyProcess(1.8, DEV, 100, rescale_timesteps=True, LIM=True, seed=5)
    assert torch.equal(m2.training_losses({'default': net}, x)['losses'], a['losses'])


# ---------------------------------------------------------------- 8. graph capture
def test_training_losses_lim_replays_from_a_captured_graph():
    """With check_finite=False and Philox draws the call holds no allocation outside the caching allocator, no synchronisation and no
    host read: it captures into a torch.cuda.graph and the replay gives the eager call's bits."""
    net = net_for('mlp')
    x = torch.randn(32, 1, 2, generator=torch.Generator().manual_seed(6)).to(DEV)
    kw = dict(clamp_eps=20, check_finite=False, return_terms=True)
    m = dlpm_amd.GenerativeLevyProcess(1.8, DEV, 100, rescale_timesteps=True, LIM=True, seed=8)
    eager = m.training_losses_lim(net, x, **kw)           # also the warm-up: native handle, workspace
    torch.cuda.synchronize()
    m.calls = 0                                           # the captured call carries the same Philox key
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = m.training_losses_lim(net, x, **kw)
    with torch.inference_mode():
        for v in captured[1:]:
            v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, eager):
        assert torch.equal(got, want)
    assert float(eager[0]) > 0


# ---------------------------------------------------------------- 9. a generic callable
def test_generic_callable_that_returns_zero():
    """loss = mean smooth-L1(e / alpha), checked against NumPy on the e the kernel reports (Philox draws, synth_long's shape)."""
    f, m = case('synth_long')
    x = torch.from_numpy(f['x_start']).to(DEV)
    out = method_for(m, DEV, seed=7).training_losses({'default': lambda x, t: torch.zeros_like(x)}, x)
    with torch.inference_mode():
        r = method_for(m, DEV, seed=7)._lim_loss_terms(zero_model, x, None, {}, keep=True)
    assert torch.equal(r['losses'], out['losses']) and torch.equal(r['t'], out['t'])
    e = r['e'].cpu().numpy()
    assert np.array_equal(r['score'].cpu().numpy(), -(e / np.float32(m['alpha'])))
    want = np_terms(np.zeros_like(e), -(e.astype(np.float64) / np.float64(np.float32(m['alpha']))))
    np.testing.assert_allclose(out['losses'].cpu().numpy(), want, rtol=2e-6)
    np.testing.assert_allclose(float(out['loss']), want.mean(), rtol=1e-6)
    # the fp64 coefficients of the drawn times, and x_t from them
    cx, sg = np_coeffs(r['t'].cpu().numpy(), m['alpha'])
    np.testing.assert_allclose(r['x_coeff'].cpu().numpy(), cx, rtol=1.2e-7)
    np.testing.assert_allclose(r['sigma'].cpu().numpy(), sg, rtol=1.2e-7)
    tail = (-1, 1, 1, 1)
    assert np.array_equal(r['x_t'].cpu().numpy(), f['x_start'] * r['x_coeff'].cpu().numpy().reshape(tail) + e * r['sigma'].cpu().numpy().reshape(tail))


# ---------------------------------------------------------------- 10. CLI
def test_cli_eval_loss_with_method_lim_equals_the_api(tmp_path, capsys):
    from dlpm_amd import cli
    from dlpm_amd import checkpoint as ck
    p = dlpm_amd.load_config('2d_data')
    p['device'] = 'cuda'
    p['method'] = 'lim'
    torch.manual_seed(11)
    model = dlpm_amd.init_model_by_parameter(p)
    ckpt = ck.save_checkpoint(str(tmp_path / 'model.pt'), {'default': model})
    x = torch.randn(48, 1, 2, generator=torch.Generator().manual_seed(12)).numpy()
    path = str(tmp_path / 'held_out.npy')
    np.save(path, x)
    base = ['--config', '2d_data', '--method', 'lim', '--checkpoint', ckpt, '--set_seed', '3', '--eval_loss', path]
    got = cli.main(base + ['--batch_size', '16'])
    printed = capsys.readouterr().out.strip().splitlines()[-1]
    assert printed.startswith('loss ') and printed.endswith(' over 48 samples') and float(printed.split()[1]) == pytest.approx(got, rel=1e-8)
    assert math.isfinite(got) and got == cli.main(base + ['--batch_size', '48'])
    meth = dlpm_amd.init_method_by_parameter(p, rng='philox', seed=3)
    assert meth.LIM
    ev = dlpm_amd.EvaluationManager(meth, None, None, verbose=False)
    assert got == ev.evaluate_loss({'default': model}, x, 48)
