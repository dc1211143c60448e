"""Held-out denoising loss on the MI355X: the three loss kernels against the reference's recorded tensors (F17), the whole
training_losses call against the reference's terms and loss for every conv generation x GEMM pipe, rng='reference', the Philox
draws (statistics, composition over chunks / offsets / evaluate_loss), graph capture, the CLI, a generic callable, and labels
following their sample into every replica."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import golden
import dlpm_amd
from dlpm_amd import _lib
from dlpm_amd.weights import state_digest
from test_host_mirror import build_unet
from test_gpu_cond import cond_net, GENERATIONS
from test_loss_cpu import CASES, case, method_for, loss_kwargs, np_terms, np_reduce

pytestmark = pytest.mark.gpu
DEV = 'cuda'
UNET_CASES = [c for c in CASES if not c.startswith('mlp')]
FORWARD_CONTRACT = 1e-4        # max |eps - eps_ref| of a forward (tests/test_gpu_models.py)


def net_for(name):
    if name.startswith('mlp'):
        torch.manual_seed(1)
        return dlpm_amd.MLPModel(dlpm_amd.load_config('2d_data'))
    if name.startswith('cond'):
        return cond_net('mnist')[0]
    return build_unet('mnist' if name.startswith('mnist') else 'tiny')[0]


def injected(f):
    return {'t': torch.from_numpy(f['t']), 'a': torch.from_numpy(f['A']), 'z': torch.from_numpy(f['z'])}


def model_kwargs(f):
    return {'y': torch.from_numpy(f['y'])} if 'y' in f.files else None


def zero_model(x, t, **kw):
    return torch.zeros_like(x)


# ---------------------------------------------------------------- 1. elements, injected draws: bit-exact
@pytest.mark.parametrize('name', CASES)
def test_elements_with_injected_draws_are_bit_exact(name):
    """Same fp32 operation order as the reference, one correctly rounded operation each: x_t, eps_t and the net input equal the
    recorded tensors bit for bit, and so do the timesteps the net is fed.

    ONE operation cannot be matched: the square root Sigma' ** (1/2) (dlpm.py:247).  The torch CPU build that recorded F17 returns
    a sqrt within 1 ulp that is not the correctly rounded one for 0.7 % of its inputs (7604 of 2^20 uniform values differ from the
    IEEE result, for every ATEN_CPU_CAPABILITY); F17 stores Sigma' and the reference's own Sigma' ** (1/2).  So:
      * the kernel's square root alone (x0 = 0, z = 1 gives x_t = sqrt(Sigma')) is held to the recorded one at 1 ulp, rtol = 1.2e-7
        (the figure test_coeff_tables_bit_exact uses for its sqrt), and IS the correctly rounded value everywhere;
      * every element whose recorded sqrt is the correctly rounded one -- all of them in 12 of the 14 cases, > 99 % in the two
        with hundreds of distinct Sigma' -- is bit-exact in all three arrays;
      * on the others the three arrays stay within what ONE ulp of the square root s can move them, with u = 2^-23, P = |s z| =
        |eps_t| bs: |d x_t| <= 2 u P + u |x_t| (the product moves by the ulp of s plus one rounding flip, the sum may flip one ulp),
        |d eps_t| <= (|d x_t| + u P) / bs + u |eps_t|, |d x_in| <= |d x_t| in_scale + u |x_in|."""
    f, m = case(name)
    meth = method_for(m, DEV)
    x = torch.from_numpy(f['x_start']).to(DEV)
    args = (m['lploss'], m['outer'], m['inner'], model_kwargs(f), m['clamp_a'])
    with torch.inference_mode():
        r = meth._loss_terms(zero_model, x, *args, injected(f), keep=True)
        ones = dict(injected(f), z=torch.ones(f['z'].shape))
        r0 = meth._loss_terms(zero_model, torch.zeros_like(x), *args, ones, keep=True)
    n = f['x_t'].shape[0]
    sq_ieee = np.sqrt(f['sigma'].astype(np.float64)).astype(np.float32)
    got_sq = r0['x_t'].cpu().numpy().reshape(n, -1)
    got_sq = got_sq[:, 0] if f['sigma'].ndim == 1 else got_sq
    np.testing.assert_allclose(got_sq, f['sqrt_sigma'], rtol=1.2e-7)
    assert np.array_equal(got_sq, sq_ieee)
    exact = f['sqrt_sigma'] == sq_ieee
    print('%s: the recorded sqrt is the correctly rounded one for %d of %d values' % (name, exact.sum(), exact.size))
    assert exact.mean() > 0.99
    exact = np.broadcast_to(exact.reshape((n, -1) if exact.ndim > 1 else (n, 1)), (n, f['x_t'][0].size)).reshape(f['x_t'].shape)
    u = 2.0 ** -23
    tail = (1,) * (f['x_t'].ndim - 1)
    te = np.tile(f['t'], m['outer'] * m['inner'])
    bs = meth.dlpm.host_schedule[3].numpy().astype(np.float64)[te].reshape((-1,) + tail)
    isc = 1.0 if not m['input_scaling'] else 1 / (1 + bs)
    P = np.abs(f['eps_t']) * bs
    dx = 2 * u * P + u * np.abs(f['x_t'])
    bounds = {'x_t': dx, 'eps_t': (dx + u * P) / bs + u * np.abs(f['eps_t']), 'x_in': dx * isc + u * np.abs(f['x_in'])}
    for key in ('x_t', 'eps_t', 'x_in'):
        got = r[key].cpu().numpy()
        diff = np.abs(got.astype(np.float64) - f[key])
        print('%s %s: max |hip - reference| = %.3g, %d of %d elements differ' % (name, key, diff.max(), (got != f[key]).sum(), got.size))
        assert np.array_equal(got[exact], f[key][exact]), key
        assert (diff[~exact] <= bounds[key][~exact]).all(), key
    assert np.array_equal(r['t'].cpu().numpy(), f['t'])
    if m['input_scaling']:
        assert not np.array_equal(f['x_in'], f['x_t'])


def test_per_sample_t_helpers_against_the_recorded_tensors():
    """DLPM.get_one_rv_loss_elements / predict_eps / predict_xstart / sample_x_t_from_xstart / q_sample on extended tensors."""
    f, m = case('tiny_median')
    meth = method_for(m, DEV)
    R = m['outer'] * m['inner']
    x0 = torch.from_numpy(f['x_start']).repeat(R, 1, 1, 1).to(DEV)
    t = torch.from_numpy(f['t']).repeat(R).to(DEV)
    a = torch.from_numpy(f['A']).repeat(m['inner']).to(DEV)
    z = torch.from_numpy(f['z']).to(DEV)
    x_t, eps_t = meth.dlpm.get_one_rv_loss_elements(t, x0, a, z)
    assert np.array_equal(x_t.cpu().numpy(), f['x_t']) and np.array_equal(eps_t.cpu().numpy(), f['eps_t'])
    assert torch.equal(meth.dlpm.predict_eps(x_t, t, x0), eps_t)
    bg, bs = (v[t.long()].view(-1, 1, 1, 1) for v in (meth.dlpm.bargammas, meth.dlpm.barsigmas))
    torch.testing.assert_close(meth.dlpm.predict_xstart(x_t, t, eps_t), (x_t - eps_t * bs) / bg, rtol=2.4e-7, atol=1e-30)   # torch's divide
    xq, e = meth.q_sample(x0, t, eps_t)
    assert e is eps_t and torch.equal(xq, bg * x0 + bs * eps_t)
    xq2, e2 = meth.q_sample(x0, 7)
    assert torch.isfinite(xq2).all() and torch.equal(xq2, meth.dlpm.bargammas[7] * x0 + meth.dlpm.barsigmas[7] * e2)


# ---------------------------------------------------------------- 2. terms from the recorded model_eps
@pytest.mark.parametrize('name', CASES)
def test_terms_from_recorded_model_eps_against_fp64(name):
    """rtol 2e-6: a fixed-order sum of D <= 12288 non-negative fp32 terms carries <= (log2 D + 3) 2^-24 ~ 1e-6 relative error, the
    sqrt halves it, factor 2 of margin (the kernel accumulates in fp64, so what is left is the fp32 rounding of each term)."""
    f, m = case(name)
    me, et = torch.from_numpy(f['model_eps']).to(DEV), torch.from_numpy(f['eps_t']).to(DEV)
    n = me.shape[0]
    out = torch.empty(n, device=DEV)
    _lib.check(_lib.lib().dlpm_loss_terms_f32(me.data_ptr(), et.data_ptr(), out.data_ptr(), n, 1, me[0].numel(), m['lploss'], n, 0,
                                              _lib.stream_ptr()))
    want = np_terms(f['model_eps'], f['eps_t'], m['lploss'])
    got = out.cpu().numpy()
    print('%s: terms max rel err vs fp64 = %.3g' % (name, float(np.abs(got / want - 1).max())))
    np.testing.assert_allclose(got, want, rtol=2e-6)
    # the (replicas, B) view with a row stride: a chunk's terms land where one call on the whole set would put them
    B, R = m['B'], m['outer'] * m['inner']
    wide = torch.full((R * (B + 5),), -1.0, device=DEV)
    _lib.check(_lib.lib().dlpm_loss_terms_f32(me.data_ptr(), et.data_ptr(), wide.data_ptr(), B, R, me[0].numel(), m['lploss'], B + 5, 3,
                                              _lib.stream_ptr()))
    wide = wide.cpu().numpy().reshape(R, B + 5)
    assert np.array_equal(wide[:, 3:3 + B].ravel(), got) and (wide[:, :3] == -1).all() and (wide[:, 3 + B:] == -1).all()


# ---------------------------------------------------------------- 3. the estimator
@pytest.mark.parametrize('estimator', ['mean', 'median'])
@pytest.mark.parametrize('name', CASES)
def test_reduce_from_recorded_terms(name, estimator):
    f, m = case(name)
    B, outer, inner = m['B'], m['outer'], m['inner']
    terms = torch.from_numpy(f['losses']).to(DEV)
    meth = method_for(m, DEV)
    idx = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    got = meth._loss_reduce(terms, B, outer, inner, estimator, True, median_index=idx)
    assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda
    want, at = np_reduce(f['losses'], B, outer, inner, estimator)
    np.testing.assert_allclose(float(got), want, rtol=1e-6)
    if estimator == m['estimator']:
        np.testing.assert_allclose(float(got), float(f['loss']), rtol=1e-6)
    if estimator == 'median':
        assert np.array_equal(idx.cpu().numpy(), at)          # the chosen outer mean (the LOWER middle one for even outer)
    # the non-finite flag
    bad = terms.clone()
    bad[bad.numel() // 2] = float('nan')
    with pytest.raises(AssertionError, match='Nan in losses'):
        meth._loss_reduce(bad, B, outer, inner, estimator, True)
    assert not math.isfinite(float(meth._loss_reduce(bad, B, outer, inner, 'mean', False)))


# ---------------------------------------------------------------- 4. end to end against the reference
def term_bounds(f, m):
    """L * 1e-4 per term: L = 1 for p = 2 (|d sqrt(mean d^2)| <= rms of the move) and p = 1 (|smooth-L1'| <= 1),
    L = 2 sqrt(term) + 1e-4 for p = -1."""
    L = np.ones_like(f['losses'], dtype=np.float64) if m['lploss'] in (2, 1) else 2 * np.sqrt(f['losses'].astype(np.float64)) + 1e-4
    return L * FORWARD_CONTRACT


def run_case(name, net, **kw):
    f, m = case(name)
    meth = method_for(m, DEV, **kw)
    x = torch.from_numpy(f['x_start']).to(DEV)
    out = meth.training_losses({'default': net}, x, model_kwargs=model_kwargs(f), noise=injected(f), **loss_kwargs(m))
    meth.close()
    return f, m, out


def check_against_reference(tag, f, m, out, factor=1.0):
    assert set(out) >= {'loss', 'losses'} and out['loss'].dim() == 0 and out['loss'].is_cuda and not out['loss'].requires_grad
    bound = factor * term_bounds(f, m)
    err = np.abs(out['losses'].cpu().numpy().astype(np.float64) - f['losses'])
    err_loss = abs(float(out['loss']) - float(f['loss']))
    print('%s: max |term - reference| = %.3g (bound %.3g), |loss - reference| = %.3g' % (tag, err.max(), bound.min(), err_loss))
    assert (err <= bound).all()
    assert err_loss <= bound.max()


@pytest.mark.parametrize('name', [c for c in CASES if c.startswith('mlp')])
def test_training_losses_against_reference_mlp(name):
    net = net_for(name)
    f, m, out = run_case(name, net)
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


def test_nested_model_kwargs_and_direct_call_agree():
    """The nested form a reference caller has to write, the flat form, and training_losses_dlpm itself."""
    net = net_for('cond_l2')
    f, m = case('cond_l2')
    x, y = torch.from_numpy(f['x_start']).to(DEV), torch.from_numpy(f['y'])
    outs = []
    for mk in ({'y': y}, {'model_kwargs': {'y': y}}):
        outs.append(method_for(m, DEV).training_losses({'default': net}, x, model_kwargs=mk, noise=injected(f))['losses'].cpu())
    loss = method_for(m, DEV).training_losses_dlpm(net, x, model_kwargs={'y': y.to(DEV)}, noise=injected(f))
    assert torch.equal(outs[0], outs[1]) and float(loss) == pytest.approx(float(outs[0].mean(dtype=torch.float64)), rel=1e-6)


# ---------------------------------------------------------------- 5. rng='reference', nothing injected
@pytest.mark.parametrize('name', ['mlp_l2', 'tiny_median'])
def test_reference_rng_is_injection_of_the_host_draws(name):
    """Same seeds as the fixture.  The terms equal those of a call that injects the same host draws explicitly (the mode IS
    injection); the loss stays within 2 x the end-to-end bound of the reference's value: the restated numpy stream moves eps_t by
    at most 4e-7 sqrt(a) + 2e-7 |eps_t| (~3e-6 at a <= 50), two orders below the forward contract, and the factor covers the
    net's response to that input move."""
    f, m = case(name)
    net = net_for(name)
    x = torch.from_numpy(f['x_start']).to(DEV)
    out = method_for(m, DEV, rng='reference', seed=m['seed']).training_losses({'default': net}, x, **loss_kwargs(m))
    draws = method_for(m, 'cpu', rng='reference', seed=m['seed'])._loss_host_draws(list(x.shape), m['outer'], m['inner'], m['clamp_a'])
    out2 = method_for(m, DEV).training_losses({'default': net}, x, noise=draws, **loss_kwargs(m))
    assert torch.equal(out['losses'], out2['losses']) and torch.equal(out['loss'], out2['loss'])
    assert np.array_equal(out['t'].cpu().numpy(), f['t'])
    check_against_reference(name + " rng='reference'", f, m, out, factor=2.0)


# ---------------------------------------------------------------- 6. Philox draws
def raw_elements(B, D, T, alpha, seed, offset=0, outer=1, inner=1, clamp_a=-1.0, elementwise=False):
    """dlpm_loss_elements_f32 with every draw from Philox; returns (t[B], a as drawn, x_t) on the host."""
    g, bg, s, bs = (v.to(DEV) for v in dlpm_amd.DLPM(alpha, 'cpu', T).host_schedule)
    R = outer * inner
    x0 = torch.zeros(B, D, device=DEV)
    x_in, eps, x_t = (torch.empty(R * B, D, device=DEV) for _ in range(3))
    t = torch.empty(B, dtype=torch.int32, device=DEV)
    a_out = torch.empty(outer * B * (D if elementwise else 1), device=DEV)
    a = _lib.LossArgs()
    a.x0_dev, a.bg_dev, a.bs_dev = x0.data_ptr(), bg.data_ptr(), bs.data_ptr()
    a.x_in_dev, a.eps_dev, a.x_t_dev, a.t_out_dev, a.a_out_dev = x_in.data_ptr(), eps.data_ptr(), x_t.data_ptr(), t.data_ptr(), a_out.data_ptr()
    a.B, a.D, a.T, a.outer, a.inner, a.flags = B, D, T, outer, inner, _lib.LOSS_ELEMENTWISE if elementwise else 0
    a.alpha, a.clamp_a, a.seed, a.sample_offset = alpha, clamp_a, seed, offset
    _lib.check(_lib.lib().dlpm_loss_elements_f32(C.byref(a), _lib.stream_ptr()))
    return t.cpu().numpy(), a_out.cpu().numpy(), eps.cpu().numpy(), bs.cpu().numpy()


def test_philox_draw_statistics():
    B, T, alpha = 1 << 16, 100, 1.7
    t, a, eps, bs = raw_elements(B, 4, T, alpha, seed=123)
    assert t.min() == 1 and t.max() == T - 1 and np.array_equal(np.unique(t), np.arange(1, T))
    # uniform on [1, T-1]: mean T/2, variance ((T-1)^2 - 1)/12
    se = math.sqrt(((T - 1) ** 2 - 1) / 12.0 / B)
    assert abs(t.mean() - T / 2) < 4 * se
    # the a draws: the check test_philox_noise_statistics_and_sharding applies to the sampler's (its reference quantiles:
    # scipy.stats.levy_stable.ppf([0.1, 0.25, 0.5, 0.75, 0.9], alpha / 2, 1, scale=2 cos(pi alpha / 4)^(2 / alpha)))
    a = a.astype(np.float64)
    assert np.all(a > 0) and np.all(np.isfinite(a))
    want_q = np.array([1.18521284, 1.37370291, 1.75562623, 2.67362479, 5.30812354])
    np.testing.assert_allclose(np.quantile(a, [0.1, 0.25, 0.5, 0.75, 0.9]), want_q, rtol=0.06)
    # z: with x0 = 0, eps_t = sqrt(a bs^2) z / bs
    z = (eps / np.sqrt(a)[:, None]).ravel().astype(np.float64)
    n = z.size
    assert abs(z.mean()) < 5 / math.sqrt(n) and abs(z.var() - 1) < 5 * math.sqrt(2 / n) + 1e-5
    # per-element a (non-isotropic), the clamp and alpha = 2
    _, ae, _, _ = raw_elements(512, 64, T, alpha, seed=5, elementwise=True)
    np.testing.assert_allclose(np.quantile(ae.astype(np.float64), [0.1, 0.25, 0.5, 0.75, 0.9]), want_q, rtol=0.06)
    _, ac, _, _ = raw_elements(4096, 4, T, alpha, seed=5, clamp_a=3.0)
    assert ac.max() == 3.0 and ac.min() >= 0.0
    _, a2, _, _ = raw_elements(64, 4, T, 2.0, seed=5)
    assert (a2 == 2.0).all()
    # replicas: a is drawn per (sample, r mod outer), z per (sample, r); an offset shifts the global index
    t1, a1, e1, _ = raw_elements(64, 8, T, alpha, seed=9, outer=3, inner=2)
    t2, a2, e2, _ = raw_elements(32, 8, T, alpha, seed=9, offset=32, outer=3, inner=2)
    assert np.array_equal(t1[32:], t2) and np.array_equal(a1.reshape(3, 64)[:, 32:], a2.reshape(3, 32))
    assert np.array_equal(e1.reshape(6, 64, 8)[:, 32:], e2.reshape(6, 32, 8))
    assert len(np.unique(a1)) == a1.size and len(np.unique(e1)) > 0.99 * e1.size


@pytest.mark.parametrize('estimator,outer,inner', [('mean', 1, 1), ('median', 3, 2)])
def test_philox_composition_over_chunks_offsets_and_evaluate_loss(estimator, outer, inner):
    net = build_unet('tiny')[0]
    N = 64
    x = 0.5 * torch.randn(N, 3, 16, 16, generator=torch.Generator().manual_seed(3))
    kw = dict(loss_monte_carlo=estimator, monte_carlo_outer=outer, monte_carlo_inner=inner, clamp_a=20)

    def method(offset=0):
        return dlpm_amd.GenerativeLevyProcess(1.7, DEV, 100, rescale_timesteps=True, seed=21, sample_offset=offset)
    whole = method().training_losses({'default': net}, x.to(DEV), **kw)
    lo = method(0).training_losses({'default': net}, x[:32].to(DEV), **kw)
    hi = method(32).training_losses({'default': net}, x[32:].to(DEV), **kw)
    R = outer * inner
    halves = torch.cat([lo['losses'].view(R, 32), hi['losses'].view(R, 32)], dim=1).reshape(-1)
    assert torch.equal(whole['losses'], halves)
    assert torch.equal(whole['t'], torch.cat([lo['t'], hi['t']]))
    figures = []
    for bs in (16, 64, 24):
        ev = dlpm_amd.EvaluationManager(method(), None, None, verbose=False)
        loss, t, terms = ev.evaluate_loss({'default': net}, x, bs, per_timestep=True, **kw)
        assert torch.equal(terms, whole['losses'].cpu()) and torch.equal(t, whole['t'].cpu())
        assert isinstance(loss, float) and ev.evals['losses'].shape == (1,) and float(ev.evals['losses'][0]) == loss
        figures.append(loss)
    assert figures[0] == figures[1] == figures[2] == float(whole['loss'])
    # an iterable of batches is the same data
    ev = dlpm_amd.EvaluationManager(method(), None, None, verbose=False)
    assert ev.evaluate_loss({'default': net}, [(x[:40], None), (x[40:], None)], 16, **kw) == figures[0]


def test_second_call_draws_fresh_noise_and_the_key_reproduces():
    net = net_for('mlp_l2')
    x = torch.randn(32, 1, 2, generator=torch.Generator().manual_seed(4)).to(DEV)
    m = dlpm_amd.GenerativeLevyProcess(1.7, DEV, 100, rescale_timesteps=True, seed=5)
    a = m.training_losses({'default': net}, x)
    b = m.training_losses({'default': net}, x)
    assert m.calls == 2 and not torch.equal(a['losses'], b['losses']) and not torch.equal(a['t'], b['t'])
    m2 = dlpm_amd.GenerativeLevyProcess(1.7, DEV, 100, rescale_timesteps=True, seed=5)
    assert torch.equal(m2.training_losses({'default': net}, x)['losses'], a['losses'])
    m2.calls = 1
    assert torch.equal(m2.training_losses({'default': net}, x)['losses'], b['losses'])


# ---------------------------------------------------------------- 7. graph capture
def test_training_losses_replays_from_a_captured_graph():
    """With check_finite=False the call holds no allocation outside the caching allocator, no synchronisation and no host read:
    it captures into a torch.cuda.graph (three kernel launches with the tiny net's forward between them) and the replay gives
    the eager call's bits."""
    net = build_unet('tiny')[0]
    x = (0.5 * torch.randn(8, 3, 16, 16, generator=torch.Generator().manual_seed(6))).to(DEV)
    kw = dict(loss_monte_carlo='median', monte_carlo_outer=3, monte_carlo_inner=2, check_finite=False, return_terms=True)
    m = dlpm_amd.GenerativeLevyProcess(1.7, DEV, 100, rescale_timesteps=True, seed=8)
    eager = m.training_losses_dlpm(net, x, **kw)          # also the warm-up: native handle, workspace
    torch.cuda.synchronize()
    m.calls = 0                                           # the captured call carries the same Philox key
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = m.training_losses_dlpm(net, x, **kw)
    with torch.inference_mode():
        for v in captured[1:]:
            v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, eager):
        assert torch.equal(got, want)
    assert float(eager[0]) > 0


# ---------------------------------------------------------------- 8. CLI
def test_cli_eval_loss_equals_the_api(tmp_path, capsys):
    from dlpm_amd import cli
    x = (0.5 * torch.randn(48, 1, 32, 32, generator=torch.Generator().manual_seed(12))).numpy()
    path = str(tmp_path / 'held_out.npy')
    np.save(path, x)
    base = ['--config', 'mnist', '--synthetic_weights', '1', '--set_seed', '3', '--eval_loss', path]
    got = cli.main(base + ['--batch_size', '16'])
    printed = capsys.readouterr().out.strip().splitlines()[-1]
    assert printed.startswith('loss ') and printed.endswith(' over 48 samples') and float(printed.split()[1]) == pytest.approx(got, rel=1e-8)
    assert math.isfinite(got) and got == cli.main(base + ['--batch_size', '48'])
    p = dlpm_amd.load_config('mnist')
    p['device'] = 'cuda'
    torch.manual_seed(3)
    model = dlpm_amd.init_model_by_parameter(p)
    dlpm_amd.rerandomize_(model, 1)
    meth = dlpm_amd.init_method_by_parameter(p, rng='philox', seed=3)
    with meth.dataset_stream():
        want = meth.training_losses({'default': model}, torch.from_numpy(x).to(DEV))
    assert got == float(want['loss'])
    med = cli.main(base + ['--batch_size', '16', '--median', '3', '2', '--lploss', '1'])
    assert math.isfinite(med) and med != got


# ---------------------------------------------------------------- 9. a generic callable
@pytest.mark.parametrize('rescale', [True, False])
def test_generic_callable_runs_through_the_same_kernels(rescale):
    seen = {}

    def model(x, t):
        seen['t'] = t
        return 0 * x
    f, m = case('tiny_l2')
    meth = dlpm_amd.GenerativeLevyProcess(m['alpha'], DEV, m['T'], rescale_timesteps=rescale)
    x = torch.from_numpy(f['x_start']).to(DEV)
    out = meth.training_losses({'default': model}, x, noise=injected(f))
    want = np.sqrt((f['eps_t'].astype(np.float64) ** 2).reshape(m['B'], -1).mean(axis=1))
    np.testing.assert_allclose(out['losses'].cpu().numpy(), want, rtol=2e-6)
    if rescale:
        assert np.array_equal(seen['t'].cpu().numpy(), f['t_in'])
    else:
        assert seen['t'].dtype == torch.int64 and np.array_equal(seen['t'].cpu().numpy(), f['t'])


# ---------------------------------------------------------------- 10. labels follow their sample into every replica
def test_labels_are_repeated_per_replica():
    net = net_for('cond_l2')
    f, m = case('cond_l2')
    B, outer, inner = m['B'], 3, 2
    R = outer * inner
    x, y = torch.from_numpy(f['x_start']).to(DEV), torch.from_numpy(f['y'])
    g = torch.Generator().manual_seed(31)
    t = torch.randint(1, m['T'], [B], generator=g)
    a = 1 + torch.rand(outer * B, generator=g)
    z = torch.randn(R * B, 1, 32, 32, generator=g)
    med = method_for(m, DEV).training_losses({'default': net}, x, model_kwargs={'y': y}, noise={'t': t, 'a': a, 'z': z},
                                             loss_monte_carlo='median', monte_carlo_outer=outer, monte_carlo_inner=inner)
    flat = method_for(m, DEV).training_losses({'default': net}, x.repeat(R, 1, 1, 1), model_kwargs={'y': y.repeat(R)},
                                              noise={'t': t.repeat(R), 'a': a.repeat(inner), 'z': z})
    assert torch.equal(med['losses'], flat['losses'])
    other = method_for(m, DEV).training_losses({'default': net}, x, model_kwargs={'y': (y + 1) % 10}, noise={'t': t, 'a': a, 'z': z},
                                               loss_monte_carlo='median', monte_carlo_outer=outer, monte_carlo_inner=inner)
    assert not torch.equal(med['losses'], other['losses'])
