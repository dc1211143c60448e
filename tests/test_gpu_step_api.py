"""GPU tests of the step-level API: dlpm_anterior_f32 and dlpm_two_rv_elements_f32 against the reference's recorded
steps, and p_mean_variance / p_sample / ddim_sample / the progressive loops against the whole-trajectory entry points they are
the pieces of.  Smallest shapes that reach every path: D % 4 == 0 (16-byte accesses), D = 3 (scalar), per-element tables."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden
import dlpm_amd
from dlpm_amd import _lib
from oracle import process as P
from step_refs import F24_CASES, f24_case, two_rv_numpy
from test_gpu_sampler import Synth, _mlp, f12_dfn
from test_host_mirror import build_unet

pytestmark = pytest.mark.gpu
DEV = 'cuda'
STEPS = (1, 2, 17, 49)


def _process(sched, T, alpha, isotropic=True):
    """A DLPM on the GPU carrying exactly the schedule vectors given (a fixture's, or the oracle's): these tests are about the
    step arithmetic; the schedule has its own (tests/test_host_mirror.py)."""
    d = dlpm_amd.process.DLPM(alpha, DEV, T, isotropic=isotropic)
    for name, key in (('gammas', 'g'), ('bargammas', 'bg'), ('sigmas', 's'), ('barsigmas', 'bs')):
        if key in sched:
            setattr(d, name, torch.as_tensor(sched[key]).to(DEV).contiguous())
    d.constants = None
    return d


def _method(f, T, alpha, shape, **kw):
    """A method object whose process carries a fixture's schedule and the tables of its A."""
    m = dlpm_amd.GenerativeLevyProcess(alpha, DEV, T, rescale_timesteps=True, **kw)
    m.dlpm = _process(f, T, alpha)
    m.dlpm.sample_A(shape, T, A=torch.from_numpy(f['A']))
    m.dlpm.compute_Sigmas()
    return m


def _t_forms(t, B):
    return [t, torch.tensor(t), torch.full((B,), t, device=DEV)]


def _per_sample(v):
    """An isotropic [B, ...] result: a stride-0 view of [B]; returns the [B] values."""
    assert all(s == 0 for s, n in zip(v.stride()[1:], v.shape[1:]) if n > 1), v.stride()
    return v.reshape(v.shape[0], -1)[:, 0].cpu().numpy()


# ------------------------------------------------------------------------------ 1. the anterior moments
def test_anterior_against_reference_single_steps():
    """dlpm_anterior_f32 at [4,3,4,4] (the 16-byte path) against F4.  The variances contain only - * /, one correctly rounded
    operation each in the reference's order: bit for bit.  The means are held to the bounds test_update_against_reference_single_step
    applies to the same formulas.  t as an int, a 0-d tensor and a [B] tensor give the same bits."""
    f = golden('f4_single_step')
    d = _process(f, 50, 1.7)
    x, eps = torch.from_numpy(f['x']).to(DEV), torch.from_numpy(f['eps']).to(DEV)
    B = x.shape[0]
    d.sample_A(list(x.shape), 50, A=torch.from_numpy(f['A']))
    d.compute_Sigmas()
    for t in STEPS:
        outs = [d.anterior_mean_variance_dlpm(x, tt, eps) for tt in _t_forms(t, B)]
        mean, var = outs[0]
        assert all(torch.equal(mean, o[0]) and torch.equal(var, o[1]) for o in outs[1:])
        assert mean.shape == x.shape and var.shape == x.shape
        assert np.array_equal(_per_sample(var), f['dlpm_var_t%d' % t])
        np.testing.assert_allclose(mean.cpu().numpy(), f['dlpm_mean_t%d' % t], rtol=3e-7, atol=1e-6)
        m0, v0 = d.anterior_mean_variance_dlim(x, torch.full((B,), t, device=DEV), eps, eta=0.0)
        assert v0 == 0
        np.testing.assert_allclose(m0.cpu().numpy(), f['dlim0_t%d' % t], rtol=3e-7, atol=1e-6)
        outs = [d.anterior_mean_variance_dlim(x, tt, eps, eta=0.5) for tt in _t_forms(t, B)]
        m5, v5 = outs[0]
        assert all(torch.equal(m5, o[0]) and torch.equal(v5, o[1]) for o in outs[1:])
        assert np.array_equal(_per_sample(v5), f['dlim05_var_t%d' % t])
        np.testing.assert_allclose(m5.cpu().numpy(), f['dlim05_mean_t%d' % t], rtol=2e-6, atol=2e-6)
    # the raw entry point refuses what it cannot run, before any launch
    a = _lib.AnteriorArgs()
    with pytest.raises(ValueError):
        _lib.check(_lib.lib().dlpm_anterior_f32(C.byref(a), _lib.stream_ptr()))


@pytest.mark.parametrize('shape,isotropic', [((2, 1, 1, 3), True), ((3, 2, 4, 4), False), ((2, 1, 1, 3), False)],
                         ids=['scalar_path', 'per_element_vector', 'per_element_scalar'])
def test_anterior_scalar_path_and_per_element_tables_against_the_oracle(shape, isotropic):
    """D = 3 (no 16-byte access possible) and non-isotropic noise ([T,B,D] tables streamed with x) against oracle.process at the
    bounds of test_update_elementwise_tables_all_variants; the variances, - * / only, bit for bit."""
    T, alpha = 12, 1.7
    g, bg, s, bs = P.schedule(T, alpha)
    gen = torch.Generator().manual_seed(sum(shape) + int(isotropic))
    B = shape[0]
    A = torch.rand((T, B) if isotropic else (T,) + shape, generator=gen) * 3 + 0.2
    x, eps = (torch.randn(shape, generator=gen) for _ in range(2))
    Sig = P.sigma_table(A, g, s)
    d = _process(dict(g=g, bg=bg, s=s, bs=bs), T, alpha, isotropic=isotropic)
    d.sample_A(list(shape), T, A=A)
    d.compute_Sigmas()
    assert torch.equal(d.Sigmas.cpu(), Sig.view(T, B, 1, 1, 1).expand(T, *shape) if isotropic else Sig)
    xd, ed, z0 = x.to(DEV), eps.to(DEV), torch.zeros(shape)
    for t in (1, 2, 7, 11):
        _, want_mean, want_var = P.dlpm_step(x, eps, t, Sig, g, bs, z0)
        mean, var = d.anterior_mean_variance_dlpm(xd, t, ed)
        np.testing.assert_allclose(mean.cpu().numpy(), want_mean.numpy(), rtol=2e-6, atol=2e-6)
        assert torch.equal(var.cpu(), P._b(want_var, x).expand(shape))
        m0, _ = d.anterior_mean_variance_dlim(xd, t, ed, eta=0.0)
        np.testing.assert_allclose(m0.cpu().numpy(), P.dlim_step(x, eps, t, g, bs, eta=0.0).numpy(), rtol=2e-6, atol=2e-6)
        m5, v5 = d.anterior_mean_variance_dlim(xd, t, ed, eta=0.5)
        want = P.dlim_step(x, eps, t, g, bs, eta=0.5, alpha=alpha, A=A, z=z0)
        np.testing.assert_allclose(m5.cpu().numpy(), want.numpy(), rtol=5e-6, atol=5e-6)
        sig = 0.5 * bs[t - 1]
        assert torch.equal(v5.cpu(), P._b((0.0 if t == 1 else 1.0) * sig ** 2 * A[t], x).expand(shape))


# ------------------------------------------------------------------------------ 2. the tables
def test_compute_sigmas_bit_exact_and_tables_broadcast():
    f = golden('f3_sigma_tables')
    T, B = f['A'].shape
    shape = [B, 3, 2, 2]
    d = _process(f, T, 1.7)
    d.sample_A(shape, T, A=torch.from_numpy(f['A']))
    assert d.Sigmas is None
    d.compute_Sigmas()
    assert np.array_equal(d._Sigmas.cpu().numpy(), f['Sigmas'])
    assert tuple(d.A.shape) == tuple(d.Sigmas.shape) == (T, *shape) and d.A.stride()[2:] == (0, 0, 0)
    x = torch.ones(shape, device=DEV)
    for t in (0, 5, T - 1):
        assert np.array_equal((x * d.Sigmas[t]).cpu().numpy(), np.broadcast_to(f['Sigmas'][t].reshape(B, 1, 1, 1), shape))
        assert np.array_equal((x * d.A[t]).cpu().numpy(), np.broadcast_to(f['A'][t].reshape(B, 1, 1, 1), shape))
    g, bg, s, bs = d.get_schedule(shape)
    assert tuple(g.shape) == (T, 3, 2, 2) and g.stride()[1:] == (0, 0, 0) and d.update_constants(shape)[3].shape == bs.shape
    assert torch.equal((x * bs[torch.full((B,), 7, device=DEV)])[:, 0, 0, 0], d.barsigmas[7].expand(B))
    # drawn on the device: a function of (seed, global sample index) only, clamped as gen_a says
    d.gen_a.setParams(clamp_a=5.0)
    d.sample_A(shape, T, seed=3)
    whole = d._A.clone()
    d.sample_A([3, 3, 2, 2], T, seed=3, sample_offset=5)
    assert torch.equal(d._A, whole[:, 5:8]) and float(whole.max()) == 5.0 and float(whole.min()) > 0
    d.sample_A(shape, T, seed=4)
    assert not torch.equal(d._A, whole)
    a = d.get_one_rv_faster_sampling(shape, seed=3)
    assert tuple(a.shape) == tuple(shape) and a.stride()[1:] == (0, 0, 0) and float(a.min()) > 0 and float(a.max()) <= 5.0


# ------------------------------------------------------------------------------ 3. p_mean_variance
def test_p_mean_variance_every_mean_type_against_reference_single_steps():
    """p_mean_variance == the reference's (GenerativeLevyProcess.py:154-219) for EPSILON / START_X / Z / PREVIOUS_X x clip_denoised x
    denoised_fn at t in {1, 2, 17, 49} (F12): 'eps' bit for bit, as test_predict_kernel_every_mean_type_vs_reference_single_steps holds
    the kernel behind it; 'variance' bit for bit (- * / only); 'mean' at the bound of the same formula in test 1."""
    f = golden('f12_mean_types')
    x = torch.from_numpy(f['x']).to(DEV)
    out = torch.from_numpy(f['out']).to(DEV)
    B = x.shape[0]
    seen = {}

    def model(v, t, shift=0.0):
        seen['t'] = t
        return out + shift
    n = 0
    for mt in _lib.MEAN_TYPES:
        m = _method(f, 50, 1.7, list(x.shape), model_mean_type=mt)
        for t in STEPS:
            for clip in (0, 1):
                for fn in (0, 1):
                    key = '%s_t%d_clip%d_fn%d' % (mt, t, clip, fn)
                    r = m.p_mean_variance(model, x, torch.full((B,), t, device=DEV), clip_denoised=bool(clip),
                                          denoised_fn=f12_dfn if fn else None, model_kwargs=dict(shift=float(f['shift'])))
                    assert set(r) == {'eps', 'mean', 'variance'}
                    assert np.array_equal(r['eps'].cpu().numpy(), f['eps_' + key]), key
                    assert np.array_equal(_per_sample(r['variance']), f['var_' + key]), key
                    np.testing.assert_allclose(r['mean'].cpu().numpy(), f['mean_' + key], rtol=3e-7, atol=1e-6, err_msg=key)
                    n += 1
        assert torch.equal(seen['t'], torch.full((B,), 49, device=DEV).float() * (1.0 / 50))     # _scale_timesteps
        m.close()
    assert n == 4 * 4 * 2 * 2


# ------------------------------------------------------------------------------ 4. p_sample is the update
def test_p_sample_is_the_update_kernel_on_a_copy():
    f = golden('f4_single_step')
    x, eps = torch.from_numpy(f['x']).to(DEV), torch.from_numpy(f['eps']).to(DEV)
    B, D = x.shape[0], x[0].numel()
    m = _method(f, 50, 1.7, list(x.shape), seed=5)
    model = lambda v, t: eps          # noqa: E731
    z = torch.randn(x.shape, generator=torch.Generator().manual_seed(1))
    d = m.dlpm
    for t in STEPS:
        tt = torch.full((B,), t, device=DEV)
        x_before = x.clone()
        got = m.p_sample(model, x, tt, noise=z.to(DEV))['sample']
        assert torch.equal(x, x_before) and got.data_ptr() != x.data_ptr()
        var = torch.from_numpy(f['dlpm_var_t%d' % t]).view(-1, 1, 1, 1)
        want = torch.from_numpy(f['dlpm_mean_t%d' % t]) + (0.0 if t == 1 else 1.0) * torch.sqrt(var) * z
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=3e-7, atol=1e-6)
        got = m.ddim_sample(model, x, tt, eta=0.0)['sample']
        np.testing.assert_allclose(got.cpu().numpy(), f['dlim0_t%d' % t], rtol=3e-7, atol=1e-6)
        got = m.ddim_sample(model, x, tt, eta=0.5, noise=torch.zeros_like(x))['sample']
        np.testing.assert_allclose(got.cpu().numpy(), f['dlim05_mean_t%d' % t], rtol=2e-6, atol=2e-6)
        # Philox: the sampler's own counters under the key of the next call (no trajectory has begun on this object)
        seed, offset = m._philox_key()
        a = _lib.UpdateArgs()
        xd, td = x.clone(), torch.tensor([t], dtype=torch.int32, device=DEV)
        a.x_dev, a.eps_dev, a.t_dev = xd.data_ptr(), eps.data_ptr(), td.data_ptr()
        a.g_dev, a.bg_dev, a.bs_dev = d.gammas.data_ptr(), d.bargammas.data_ptr(), d.barsigmas.data_ptr()
        a.c_eps_dev, a.c_noise_dev, a.A_dev = d._c_eps.data_ptr(), d._c_noise.data_ptr(), d._A.data_ptr()
        a.B, a.D, a.T, a.alpha, a.seed, a.sample_offset = B, D, 50, 1.7, seed, offset
        _lib.check(_lib.lib().dlpm_update_f32(C.byref(a), _lib.stream_ptr()))
        got = m.p_sample(model, x, tt)['sample']
        assert torch.equal(got, xd) and (t == 1 or not torch.equal(got, m.p_sample(model, x, tt, noise=torch.zeros_like(x))['sample']))
    # without the tables of a trajectory of this shape the step methods say what is missing
    with pytest.raises(_lib.DlpmError, match='sample_A'):
        m.p_sample(model, x[:2], torch.full((2,), 3, device=DEV))
    m.close()


# ------------------------------------------------------------------------------ 5. the progressive loops against the reference
@pytest.mark.parametrize('name', ['f5_traj_synth_img', 'f5_traj_dlim_toy'])
def test_progressive_loop_identical_seeds_vs_reference(name):
    """The generators on the reference's CPU streams == the reference's recorded trajectory, at the bounds
    test_trajectory_identical_seeds_vs_reference applies to sample() on the same files."""
    f = golden(name)
    T, alpha, det, eta, ca, ce, clip = f['meta']
    T, shape = int(T), [int(v) for v in f['shape']]
    meth = dlpm_amd.GenerativeLevyProcess(float(alpha), DEV, T, rescale_timesteps=True, rng='reference', seed=0)
    meth.dlpm.gen_a.setParams(clamp_a=None if ca < 0 else float(ca))
    meth.dlpm.gen_eps.setParams(clamp_eps=None if ce < 0 else float(ce))
    model = Synth().to(DEV)
    if det:
        gen = meth.ddim_sample_loop_progressive(model, shape, clip_denoised=bool(clip), eta=float(eta))
    else:
        gen = meth.p_sample_loop_progressive(model, shape, clip_denoised=bool(clip))
    assert meth.calls == 0
    items = list(gen)
    assert len(items) == T and meth.calls == 1 and all(set(it) == {'sample'} for it in items)
    assert len({it['sample'].data_ptr() for it in items}) == T
    got = torch.stack([it['sample'] for it in items]).cpu().numpy()
    want = f['history']
    assert got.shape == want.shape
    scale = np.abs(want).max(axis=tuple(range(1, want.ndim)), keepdims=True) + 1e-6
    assert np.max(np.abs(got - want) / scale) < 5e-5
    fin = f['final']
    assert np.abs(got[-1] - fin).max() < 1e-4 * max(1.0, np.abs(fin).max())
    assert np.array_equal(meth.dlpm._A.cpu().numpy(), f['A']) and tuple(meth.dlpm.Sigmas.shape) == (T, *shape)


# ------------------------------------------------------------------------------ 6. a hand-written loop is the loop
T_HAND = 9


# per-element tables ([T,B,D], the generic path of the generators) and the input scaling of a scale_exploding process
KIND_KW = {'callable_noniso': dict(isotropic=False), 'unet_noniso': dict(isotropic=False),
           'callable_inscale': dict(scale='scale_exploding', input_scaling=True)}


def _net(kind):
    if kind == 'callable':
        return Synth().to(DEV), [3, 2, 4, 4]
    if kind == 'unet':
        return build_unet('tiny')[0], [2, 3, 16, 16]
    return _mlp(), [5, 1, 2]


@pytest.fixture(scope='module')
def nets():
    return {k: _net(k) for k in ('callable', 'unet', 'mlp')}


def _hand_loop(meth, model, shape, variant):
    if variant == 'p':
        gen, step = meth.p_sample_loop_progressive(model, shape), meth.p_sample
    else:
        eta = float(variant)
        gen = meth.ddim_sample_loop_progressive(model, shape, eta=eta)
        step = lambda *a: meth.ddim_sample(*a, eta=eta)          # noqa: E731
    x = next(gen)['sample']
    for i in range(T_HAND - 1, 0, -1):
        x = step(model, x, torch.full((shape[0],), i, device=DEV))['sample']
    return x


def _whole_loop(meth, model, shape, variant, **kw):
    if variant == 'p':
        return meth.p_sample_loop(model, shape, **kw)
    return meth.ddim_sample_loop(model, shape, eta=float(variant), **kw)


@pytest.mark.parametrize('variant', ['p', '0.0', '0.5'], ids=['p_sample', 'ddim_eta0', 'ddim_eta05'])
@pytest.mark.parametrize('kind', ['callable', 'unet', 'mlp', 'callable_noniso', 'unet_noniso', 'callable_inscale'])
def test_hand_written_loop_equals_the_loop(nets, kind, variant):
    """next(gen) then p_sample / ddim_sample by hand == p_sample_loop / ddim_sample_loop of an identically seeded twin, bit for
    bit: same key, same tables, same counters, whether the twin runs the Python loop (callable), the captured graph (tiny UNet)
    or the per-step MLP path (fused_mlp=False); with per-element noise tables and with input scaling too."""
    model, shape = nets[kind.split('_')[0]]
    kw = dict(rescale_timesteps=True, seed=21, fused_mlp=False, **KIND_KW.get(kind, {}))
    a, b = (dlpm_amd.GenerativeLevyProcess(1.7, DEV, T_HAND, **kw) for _ in range(2))
    got = _hand_loop(a, model, shape, variant)
    want = _whole_loop(b, model, shape, variant)
    assert torch.isfinite(want).all() and torch.equal(got, want)
    assert a.calls == b.calls == 1
    a.close()
    b.close()


def test_hand_written_loop_against_the_fused_toy_loop():
    """The one-launch toy loop sums its Linear layers in another order: the bound of test_fused_mlp_loop_matches_step_by_step."""
    model, shape = _mlp(), [37, 1, 2]
    a, b = (dlpm_amd.GenerativeLevyProcess(1.7, DEV, T_HAND, rescale_timesteps=True, seed=9, fused_mlp=True) for _ in range(2))
    got, want = _hand_loop(a, model, shape, 'p').cpu(), b.p_sample_loop(model, shape).cpu()
    assert (got - want).abs().max().item() < 2e-4 * max(1.0, want.abs().max().item())
    a.close()
    b.close()


# ------------------------------------------------------------------------------ 7. the native progressive loop
def test_native_progressive_loop_equals_the_history_and_pins_its_key(nets):
    model, shape = nets['unet']
    kw = dict(rescale_timesteps=True, seed=33)
    a, b = (dlpm_amd.GenerativeLevyProcess(1.7, DEV, T_HAND, **kw) for _ in range(2))
    x1, hist1 = b.p_sample_loop(model, shape, get_sample_history=True)
    x2 = b.p_sample_loop(model, shape)
    items = [it['sample'] for it in a.p_sample_loop_progressive(model, shape)]
    assert len(items) == T_HAND and len({v.data_ptr() for v in items}) == T_HAND
    assert torch.equal(torch.stack(items), hist1) and torch.equal(items[-1], x1)
    # second trajectory: a new key; three yields, the generator dropped, the rest by hand -- under the key the generator took
    gen = a.p_sample_loop_progressive(model, shape)
    x = [next(gen)['sample'] for _ in range(3)][-1]
    assert a.calls == 2
    del gen
    for i in range(T_HAND - 3, 0, -1):
        x = a.p_sample(model, x, torch.full((shape[0],), i, device=DEV))['sample']
    assert torch.equal(x, x2) and not torch.equal(x2, x1)
    # a generator whose sampler another loop has taken over says so instead of yielding that loop's state
    gen = a.ddim_sample_loop_progressive(model, shape, eta=0.5)
    first = next(gen)['sample']
    want = b.ddim_sample_loop(model, shape, eta=0.5, get_sample_history=True)[1]
    assert torch.equal(first, want[0]) and torch.equal(next(gen)['sample'], want[1])
    a.p_sample_loop(model, shape)
    with pytest.raises(_lib.DlpmError, match='another loop'):
        next(gen)
    a.close()
    b.close()


# ------------------------------------------------------------------------------ 8. the Proposition-8 elements
@pytest.mark.parametrize('tag', F24_CASES)
def test_two_rv_elements_against_the_reference_with_injected_draws(tag):
    """dlpm_two_rv_elements_f32 on the reference's recorded draws (F24).  The [B] outputs contain only + - * /: bit for bit,
    lambda = +inf and Sigma~ = 0 at t == 1 included.  x_t, eps_t, m~ pass through Sigma' ** (1/2): bit for bit where the recorded root
    is the correctly rounded one (the condition under which tests/test_gpu_loss.py holds the one-rv elements bit for bit), within
    its rtol 2e-6 elsewhere."""
    c = f24_case(golden('f24_two_rv'), tag)
    alpha = float(tag.split('_a')[1].replace('p', '.'))
    d = _process(c, 12, alpha)
    x0, z = torch.from_numpy(c['x0']).to(DEV), torch.from_numpy(c['z']).to(DEV)
    t = torch.from_numpy(c['t']).to(DEV)
    B = x0.shape[0]
    keys = ('x_t', 'eps_t', 'm_tilde', 'Sigma_tilde', 'lambda', 'Sigma_prime_t_1', 'Sigma_prime_t', 'Gamma_prime')
    a0 = torch.from_numpy(c['a0'])
    for a_form in (a0, a0.view(B, *([1] * (x0.dim() - 1))).expand(x0.shape)):          # [B], or the reference's expanded form
        got = dict(zip(keys, d.get_two_rv_loss_elements(t, x0, a_form, torch.from_numpy(c['a1']), z, return_constants=True)))
        for k in keys[3:]:
            assert got[k].shape == x0.shape and _per_sample(got[k]).tobytes() == c[k].tobytes(), k
        exact = c['sqrt_Sigma_prime_t'] == np.sqrt(c['Sigma_prime_t'].astype(np.float64)).astype(np.float32)
        for k in keys[:3]:
            g = got[k].cpu().numpy()
            assert np.array_equal(g[exact], c[k][exact]), k
            np.testing.assert_allclose(g[~exact], c[k][~exact], rtol=2e-6, err_msg=k)
    five = d.get_two_rv_loss_elements(t, x0, a0, torch.from_numpy(c['a1']), z)
    assert len(five) == 5 and all(torch.equal(u, got[k]) for u, k in zip(five, keys))
    one = c['t'] == 1
    assert np.isposinf(_per_sample(five[4])[one]).all() and (_per_sample(five[3])[one] == 0).all()
    # the one-line torch helpers on the same tensors: the reference's expressions on the device.  Products and sums are IEEE in
    # both; torch's device division is within 1 ulp (2^-23) of the correctly rounded one, which Gamma' = 1 - q turns into 2^-23 absolute
    tl, tail = t.long(), [1] * (x0.dim() - 1)
    a0z = torch.where((tl == 1).view(B, *tail), 0.0, a0.to(DEV).view(B, *tail)).expand(x0.shape)
    a1e = torch.from_numpy(c['a1']).to(DEV).view(B, *tail).expand(x0.shape)
    sp1, sp, gam = d.compute_two_rv_prime_constants(tl, a0z, a1e)
    assert sp1.shape == x0.shape
    np.testing.assert_allclose(sp1.cpu().numpy(), got['Sigma_prime_t_1'].cpu().numpy(), rtol=1.2e-7)
    np.testing.assert_allclose(sp.cpu().numpy(), got['Sigma_prime_t'].cpu().numpy(), rtol=2.4e-7)
    np.testing.assert_allclose(gam.cpu().numpy(), got['Gamma_prime'].cpu().numpy(), rtol=0, atol=2.4e-7)
    lam = d.compute_two_rv_lambda(tl, sp1)
    assert torch.isposinf(lam[torch.from_numpy(one).to(DEV)]).all()
    fin = torch.from_numpy(~one).to(DEV)
    np.testing.assert_allclose(lam[fin].cpu().numpy(), got['lambda'][fin].cpu().numpy(), rtol=3.6e-7)


@pytest.mark.parametrize('shape', [(3, 2, 4, 4), (2, 1, 1, 3)], ids=['vector', 'scalar'])
def test_two_rv_elements_per_element_draws_against_the_restatement(shape):
    """Non-isotropic noise: one (a0, a1) per element, every [n] output an array of x's shape.  Against the NumPy restatement
    (tests/step_refs.py: the same operations, each correctly rounded, the root included): bit for bit."""
    T, alpha = 12, 1.7
    g, bg, s, bs = (v.numpy() for v in P.schedule(T, alpha))
    gen = torch.Generator().manual_seed(sum(shape))
    x0, z = (torch.randn(shape, generator=gen) for _ in range(2))
    a0, a1 = (torch.rand(shape, generator=gen) * 3 + 0.2 for _ in range(2))
    t = torch.tensor([1, 5, 11][:shape[0]])
    d = _process(dict(g=g, bg=bg, s=s, bs=bs), T, alpha, isotropic=False)
    keys = ('x_t', 'eps_t', 'm_tilde', 'Sigma_tilde', 'lambda', 'Sigma_prime_t_1', 'Sigma_prime_t', 'Gamma_prime')
    got = dict(zip(keys, d.get_two_rv_loss_elements(t.to(DEV), x0.to(DEV), a0, a1, z.to(DEV), return_constants=True)))
    want = two_rv_numpy(x0.numpy(), t.numpy(), a0.numpy(), a1.numpy(), z.numpy(), g, bg, s, bs)
    for k in keys:
        assert got[k].shape == x0.shape and got[k].cpu().numpy().tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize('isotropic', [True, False])
def test_two_rv_elements_philox_draws(isotropic):
    """Draws made by the kernel: the same bits on two calls, other bits under another seed, shards compose, a0 == 0 exactly where
    t == 1, the clamp of gen_a holds, and the elements are what the restatement makes of the draws the kernel reports."""
    T, alpha, shape = 12, 1.7, (6, 2, 4, 4)
    sched = dict(zip(('g', 'bg', 's', 'bs'), (v.numpy() for v in P.schedule(T, alpha))))
    d = _process(sched, T, alpha, isotropic=isotropic)
    d.gen_a.setParams(clamp_a=4.0)
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(8)).to(DEV)
    t = torch.tensor([1, 2, 1, 7, 11, 1], device=DEV)
    a = d.get_two_rv_loss_elements(t, x0, seed=7, return_constants=True)
    b = d.get_two_rv_loss_elements(t, x0, seed=7, return_constants=True)
    c = d.get_two_rv_loss_elements(t, x0, seed=8, return_constants=True)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and not torch.equal(a[0], c[0]) and not torch.equal(a[6], c[6])
    lo = d.get_two_rv_loss_elements(t[:2], x0[:2], seed=7, return_constants=True)
    hi = d.get_two_rv_loss_elements(t[2:], x0[2:], seed=7, sample_offset=2, return_constants=True)
    assert all(torch.equal(torch.cat([u, v]), w) for u, v, w in zip(lo, hi, a))
    a0, a1 = d.get_two_rv_faster_sampling(x0, t, seed=7)
    assert a0.shape == x0.shape and a1.shape == x0.shape
    one = t == 1
    assert bool((a0[one] == 0).all()) and bool((a0[~one] > 0).all()) and bool((a1 > 0).all()) and float(torch.max(a0.max(), a1.max())) <= 4.0
    assert isotropic == all(s == 0 for s in a0.stride()[1:])
    assert not torch.equal(a0[~one], a1[~one]) and len(torch.unique(a1[:, 0, 0, 0])) > 1
    assert isotropic or len(torch.unique(a1[0])) > 1
    z = (a[0] - d.bargammas[t.long()].view(-1, 1, 1, 1) * x0) / torch.sqrt(a[6])          # recovered to rounding: only its scale matters
    assert 0.8 < float(z.std()) < 1.2 and abs(float(z.mean())) < 0.25
    assert bool(torch.isposinf(a[4][one]).all()) and bool((a[3][one] == 0).all()) and bool(torch.isfinite(a[4][~one]).all())
    # injected back, the reported draws give the same elements: the Philox path and the injected path are one computation
    pick = (lambda v: v) if not isotropic else (lambda v: v[:, 0, 0, 0])
    zero = torch.zeros_like(x0)
    inj = d.get_two_rv_loss_elements(t, x0, pick(a0), pick(a1), zero, return_constants=True)
    assert all(torch.equal(u, v) for u, v in zip(inj[3:], a[3:]))


# ------------------------------------------------------------------------------ 9, 10
def test_q_posterior_is_predict_eps_then_the_dlpm_moments():
    f = golden('f4_single_step')
    x_t, x_0 = torch.from_numpy(f['x']).to(DEV), torch.from_numpy(f['eps']).to(DEV) * 0.5
    B = x_t.shape[0]
    m = _method(f, 50, 1.7, list(x_t.shape))
    other = dlpm_amd.GenerativeLevyProcess(1.7, DEV, 50, rescale_timesteps=True)        # holds no tables: Sigmas is an argument
    other.dlpm = _process(f, 50, 1.7)
    for t in (1, 17, torch.full((B,), 49, device=DEV)):
        want = m.dlpm.anterior_mean_variance_dlpm(x_t, t, m.dlpm.predict_eps(x_t, t, x_0))
        for Sig in (m.dlpm.Sigmas, m.dlpm._Sigmas):                                     # [T, *shape] or [T,B]
            got = other.q_posterior_mean_variance(x_0, x_t, t, Sig)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[1].shape == x_t.shape
    assert other.dlpm.Sigmas is None


@pytest.mark.parametrize('kind', ['mlp', 'callable'])
def test_lim_sample_is_the_lim_path_of_sample(kind):
    model, shape = (_mlp(), [7, 1, 2]) if kind == 'mlp' else (Synth().to(DEV), [3, 2, 4, 4])
    kw = dict(rescale_timesteps=True, LIM=True, seed=3)
    for ddim in (False, True):
        a, b = (dlpm_amd.GenerativeLevyProcess(1.8, DEV, 10, **kw) for _ in range(2))
        want, want_hist = b.sample({'default': model}, shape, 10, deterministic=ddim, get_sample_history=True)
        got, hist = a.lim_sample(model, shape, ddim=ddim, get_sample_history=True)
        assert torch.isfinite(want).all() and torch.equal(got, want) and torch.equal(hist, want_hist) and a.calls == b.calls == 1
        assert torch.equal(a.lim_sample(model, shape, ddim=ddim), b.sample({'default': model}, shape, 10, deterministic=ddim))
        assert not torch.equal(got, a.lim_sample(model, shape, ddim=ddim))
        a.close()
        b.close()
    with pytest.raises(AssertionError):
        dlpm_amd.GenerativeLevyProcess(1.8, DEV, 10, rescale_timesteps=True).lim_sample(model, shape)


# ------------------------------------------------------------------------------ no host read: both kernels capture
def test_step_kernels_replay_from_a_captured_graph_and_read_t_on_the_device():
    """Neither entry point reads a host value or synchronises: the moments and the Proposition-8 elements capture into a
    torch.cuda.graph, and a replay after the DEVICE timesteps were overwritten gives the eager call's bits at the new timesteps."""
    f = golden('f4_single_step')
    d = _process(f, 50, 1.7)
    x, eps = torch.from_numpy(f['x']).to(DEV), torch.from_numpy(f['eps']).to(DEV)
    B = x.shape[0]
    d.sample_A(list(x.shape), 50, A=torch.from_numpy(f['A']))
    d.compute_Sigmas()
    t = torch.full((B,), 2, device=DEV)
    d.anterior_mean_variance_dlpm(x, t, eps), d.get_two_rv_loss_elements(t, x, seed=4)        # warm-up: code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mean, var = d.anterior_mean_variance_dlpm(x, t, eps)
        m5, v5 = d.anterior_mean_variance_dlim(x, t, eps, eta=0.5)
        two = d.get_two_rv_loss_elements(t, x, seed=4)
    t.copy_(torch.tensor([17, 1, 49, 17], device=DEV))
    g.replay()
    torch.cuda.synchronize()
    want = d.anterior_mean_variance_dlpm(x, 17, eps)
    assert torch.equal(mean, want[0]) and torch.equal(var, want[1])          # the step formulas use t[0]
    assert np.array_equal(_per_sample(var), f['dlpm_var_t17']) and np.array_equal(_per_sample(v5), f['dlim05_var_t17'])
    assert torch.equal(m5, d.anterior_mean_variance_dlim(x, 17, eps, eta=0.5)[0])
    assert all(torch.equal(u, v) for u, v in zip(two, d.get_two_rv_loss_elements(t, x, seed=4)))
    assert bool(torch.isposinf(two[4][1]).all()) and bool(torch.isfinite(two[4][0]).all())   # per-sample t: lambda = inf where t == 1
