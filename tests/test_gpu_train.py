"""Training of the toy net on the MI355X (include/dlpm_amd_train.h, dlpm_amd/training.py): the backward against float64 autograd
with torch's own fp32 autograd as the yardstick, the loss gradient, AdamW + EMA and the clip against the fp64 mirrors of
tests/train_refs.py (pinned on the CPU by tests/test_train_cpu.py), the parameter layout, one step as the composition of its parts,
reproducibility, resume, and a short run that learns."""
import ctypes as C

import numpy as np
import pytest
import torch

import dlpm_amd
from dlpm_amd import _lib, cli
import train_refs as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'

NETS = [(2, 4, 32), (1, 0, 64), (5, 1, 7)]          # (F, nblocks, TE): the shipped net and two that leave its sizes
ROW_CHUNK = 64                                     # rows per chunk of the weight-gradient reduction (mlp_train.hip: RC)
ROWS = [1, 3, 4, 5, 13, 260, ROW_CHUNK + 1]
# err_dev <= K * err_torch32 per tensor: the kernel's __expf SiLU and its summation order are not torch's.  K is the worst ratio
# measured on the GPU over NETS x ROWS (profiles/train/README.md), doubled and rounded up to a power of two.
K = 16.0
CEILING = 2e-5                                     # twice the forward's own contract (test_mlp_forward_matches_reference)


def stream():
    return _lib.stream_ptr()


def rel(a, b):
    """||a - b||_2 / ||b||_2 in fp64 (0 where both vanish)."""
    a, b = a.detach().cpu().double().reshape(-1), b.detach().cpu().double().reshape(-1)
    n = float(b.norm())
    d = float((a - b).norm())
    return d / n if n > 0 else d


def inputs(F, rows, seed):
    g = torch.Generator().manual_seed(seed)
    return 3 * torch.randn(rows, 1, F, generator=g), torch.rand(rows, generator=g), torch.randn(rows, 1, F, generator=g)


def dev_backward(net, x, t, dout, want_dx=True):
    """(flat gradient, dx) of dlpm_mlp_backward_f32; outputs and workspace start as NaN, so an element nobody wrote shows."""
    L = _lib.lib()
    h = net.native_handle()
    P, rows = L.dlpm_mlp_param_floats(h), x.shape[0]
    need = L.dlpm_mlp_backward_workspace_bytes(h, rows)
    ws = torch.full((need // 4,), float('nan'), dtype=torch.float32, device=DEV)
    grad = torch.full((P,), float('nan'), dtype=torch.float32, device=DEV)
    dx = torch.full(tuple(x.shape), float('nan'), dtype=torch.float32, device=DEV)
    xd, td, dd = x.to(DEV).contiguous(), t.to(DEV).contiguous(), dout.to(DEV).contiguous()
    _lib.check(L.dlpm_mlp_backward_f32(h, xd.data_ptr(), td.data_ptr(), dd.data_ptr(), rows, grad.data_ptr(),
                                       dx.data_ptr() if want_dx else None, ws.data_ptr(), need, stream()))
    return grad, dx


def split(net, flat):
    out, off = {}, 0
    for n, p in net.named_parameters():
        out[n] = flat[off:off + p.numel()].reshape(p.shape)
        off += p.numel()
    assert off == flat.numel()
    return out


_NETS = {}


def net_of(shape):
    if shape not in _NETS:
        _NETS[shape] = R.toy_net(*shape)
    return _NETS[shape]


_REFS = {}


def refs_of(shape, rows):
    """The fp64 and fp32 CPU autograd gradients at the seeded inputs, computed once per case."""
    key = (shape, rows)
    if key not in _REFS:
        x, t, dout = inputs(shape[0], rows, 1000 + rows)
        net = net_of(shape)
        _REFS[key] = (x, t, dout, R.autograd_grads(net, x, t, dout, torch.float64), R.autograd_grads(net, x, t, dout, torch.float32))
    return _REFS[key]


def judge(tag, got, got_dx, g64, dx64, g32, dx32):
    """Per tensor: print the three figures, then err_dev <= K * err_torch32 and err_dev <= CEILING."""
    worst = 0.0
    rows = [(n, got[n], g64[n], g32[n]) for n in g64] + [('dx', got_dx, dx64, dx32)]
    bad = []
    for n, a, r64, r32 in rows:
        assert torch.isfinite(a).all(), (tag, n)
        e_dev, e_32 = rel(a, r64), rel(r32, r64)
        ratio = e_dev / e_32 if e_32 > 0 else (0.0 if e_dev == 0 else float('inf'))
        worst = max(worst, ratio)
        print('%s %-40s err_dev %.3e err_torch32 %.3e ratio %.2f' % (tag, n, e_dev, e_32, ratio))
        if not (e_dev <= K * e_32 and e_dev <= CEILING):
            bad.append((n, e_dev, e_32))
    print('%s worst ratio %.2f' % (tag, worst))
    assert not bad, (tag, bad)


# ------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('shape', NETS)
def test_backward_against_float64_autograd(shape, rows):
    x, t, dout, (g64, dx64), (g32, dx32) = refs_of(shape, rows)
    net = net_of(shape)
    grad, dx = dev_backward(net, x, t, dout)
    judge('net %s rows %d' % (shape, rows), split(net, grad.cpu()), dx.cpu(), g64, dx64, g32, dx32)
    # without dx the parameter gradient is the same
    grad2, _ = dev_backward(net, x, t, dout, want_dx=False)
    assert torch.equal(grad, grad2)


@pytest.mark.parametrize('shape', NETS)
def test_backward_is_deterministic(shape):
    x, t, dout = inputs(shape[0], 260, 7)
    net = net_of(shape)
    a, adx = dev_backward(net, x, t, dout)
    b, bdx = dev_backward(net, x, t, dout)
    assert torch.equal(a, b) and torch.equal(adx, bdx)


@pytest.mark.parametrize('shape', NETS)
def test_ragged_last_quad_leaves_no_trace(shape):
    """rows = 5: one full wave and one with three padded rows.  The gradient equals the sum of the gradients of rows 0..3 and of row 4
    computed on their own, within the tolerance of the backward itself; dx of each row is the same bits in both."""
    x, t, dout, (g64, dx64), (g32, dx32) = refs_of(shape, 5)
    net = net_of(shape)
    g5, dx5 = dev_backward(net, x, t, dout)
    g4, dx4 = dev_backward(net, x[:4], t[:4], dout[:4])
    g1, dx1 = dev_backward(net, x[4:], t[4:], dout[4:])
    assert torch.equal(dx5, torch.cat([dx4, dx1]))
    whole, parts = split(net, g5.cpu()), split(net, (g4.double() + g1.double()).cpu())
    for n in g64:
        e = float((whole[n].double() - parts[n]).norm() / g64[n].norm())
        e_32 = rel(g32[n], g64[n])
        print('%s %-40s |g5 - (g4 + g1)| / |g64| %.3e err_torch32 %.3e' % (shape, n, e, e_32))
        assert e <= K * e_32 and e <= CEILING, (n, e, e_32)


# ------------------------------------------------------------------------------------------ loss gradient
def dev_terms(me, tg, B, R_, D, lploss):
    out = torch.empty(R_ * B, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().dlpm_loss_terms_f32(me.data_ptr(), tg.data_ptr(), out.data_ptr(), B, R_, D, lploss, B, 0, stream()))
    return out


def dev_reduce(terms, B, outer, inner, median):
    res = torch.empty(1, dtype=torch.float32, device=DEV)
    flag = torch.empty(1, dtype=torch.int32, device=DEV)
    idx = torch.empty(B, dtype=torch.int32, device=DEV) if median else None
    _lib.check(_lib.lib().dlpm_loss_reduce_f32(terms.data_ptr(), B, outer, inner, int(median), res.data_ptr(), flag.data_ptr(),
                                               _lib.ptr(idx), stream()))
    return res, idx


def dev_loss_grad(me, tg, terms, idx, B, outer, inner, D, lploss):
    out = torch.full_like(me, float('nan'))
    _lib.check(_lib.lib().dlpm_loss_grad_f32(me.data_ptr(), tg.data_ptr(), terms.data_ptr(), _lib.ptr(idx), out.data_ptr(), B, outer, inner,
                                             D, lploss, stream()))
    return out


@pytest.mark.parametrize('lploss', [2, 1, -1])
@pytest.mark.parametrize('median', [False, True])
@pytest.mark.parametrize('outer,inner', [(1, 1), (3, 2)])
@pytest.mark.parametrize('D', [2, 75])
@pytest.mark.parametrize('B', [1, 7])
def test_loss_grad_against_the_fp64_mirror(B, D, outer, inner, median, lploss):
    g = torch.Generator().manual_seed(B * 1000 + D * 10 + outer + lploss)
    rows = outer * inner * B
    me = (1.5 * torch.randn(rows, D, generator=g)).to(DEV)
    tg = torch.randn(rows, D, generator=g).to(DEV)
    if rows > 1:
        me[0] = tg[0]                                       # a row with model_eps == target
    terms = dev_terms(me, tg, B, outer * inner, D, lploss)
    _, idx = dev_reduce(terms, B, outer, inner, median)
    got = dev_loss_grad(me, tg, terms, idx, B, outer, inner, D, lploss).cpu()
    want = R.loss_grad_ref(me, tg, terms, idx, B, outer, inner, D, lploss)
    torch.testing.assert_close(got.double(), want, rtol=1e-6, atol=1e-9)
    if rows > 1:
        assert (got[0] == 0).all()                          # exact zeros, where torch's autograd gives NaN at lploss = 2
    if median:
        sel = idx.cpu().long()
        assert ((sel >= 0) & (sel < outer)).all()
        unselected = torch.arange(outer).reshape(outer, 1, 1) != sel.reshape(1, 1, B)
        assert (got.reshape(outer, inner, B, D)[unselected.expand(outer, inner, B)] == 0).all()
        assert outer == 1 or unselected.any()
    else:
        assert (got[-1] != 0).all()


# ------------------------------------------------------------------------------------------ AdamW + EMA, clip
N_VEC = 1031            # no multiple of any vector width
MUS = (0.9, 0.999)
TINY = 1.2e-38          # below the smallest normal fp32 the spacing of fp32 is absolute (1.4e-45): no relative bound can hold there


def dev_adamw(theta, g, m, v, shadows, lr, betas, eps, wd, step, coef):
    a = _lib.AdamwArgs()
    a.theta_dev, a.grad_dev, a.exp_avg_dev, a.exp_avg_sq_dev, a.n = theta.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), theta.numel()
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.step = lr, betas[0], betas[1], eps, wd, step
    a.coef_dev = _lib.ptr(coef)
    a.n_ema = len(shadows)
    for i, (s, mu) in enumerate(zip(shadows, MUS)):
        a.ema_dev[i], a.ema_mu[i] = s.data_ptr(), mu
    _lib.check(_lib.lib().dlpm_adamw_step_f32(C.byref(a), stream()))


@pytest.mark.parametrize('with_coef', [False, True])
def test_adamw_and_ema_against_the_fp64_mirror(with_coef):
    """Steps 1 and 2 from the zero state, then step 1000 from the state they left, each judged against the fp64 update of the fp32
    state the kernel was given.  Moments and shadows: rtol 2.4e-7 (two or three roundings; TINY absolute for the subnormal second
    moments of the 1e-20 gradients); theta: one ulp of theta plus eight of an update bounded by lr."""
    gen = torch.Generator().manual_seed(11)
    lr, betas, eps, wd = 5e-3, (0.9, 0.999), 1e-8, 0.01
    theta = torch.randn(N_VEC, generator=gen).to(DEV)
    m, v = torch.zeros(N_VEC, device=DEV), torch.zeros(N_VEC, device=DEV)
    shadows = [theta.clone(), (theta + 0.01).clone()]
    coef = torch.tensor([0.37], device=DEV) if with_coef else None
    for step in (1, 2, 1000):
        g = torch.randn(N_VEC, generator=gen)
        g[::13] = 0.0
        g[5::17] = 1e-20
        g = g.to(DEV)
        before = [a.clone() for a in (theta, m, v)] + [s.clone() for s in shadows]
        want_t, want_m, want_v, want_s = R.adamw_ref(before[0], g, before[1], before[2], lr, betas, eps, wd, step,
                                                     coef=None if coef is None else float(coef), shadows=before[3:], mus=MUS)
        dev_adamw(theta, g, m, v, shadows, lr, betas, eps, wd, step, coef)
        torch.testing.assert_close(m.cpu().double(), want_m, rtol=2.4e-7, atol=TINY)
        torch.testing.assert_close(v.cpu().double(), want_v, rtol=2.4e-7, atol=TINY)
        for s, w in zip(shadows, want_s):
            torch.testing.assert_close(s.cpu().double(), w, rtol=2.4e-7, atol=TINY)
        d = (theta.cpu().double() - want_t).abs()
        assert (d <= 1.2e-7 * want_t.abs() + 1e-6 * lr).all(), float(d.max())
        if step == 1:
            zero = (g == 0).cpu()
            assert (m.cpu()[zero] == 0).all() and (v.cpu()[zero] == 0).all()
            assert torch.equal(theta.cpu()[zero], (before[0].cpu().double()[zero] * (1 - lr * wd)).float())
    assert not torch.equal(shadows[0], shadows[1])


@pytest.mark.parametrize('max_norm', [0.5, 1e3])
def test_clip_coefficient(max_norm):
    g = torch.randn(N_VEC, generator=torch.Generator().manual_seed(12)).to(DEV)
    norm, coef = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    _lib.check(_lib.lib().dlpm_grad_clip_coef_f32(g.data_ptr(), N_VEC, max_norm, norm.data_ptr(), coef.data_ptr(), stream()))
    want_norm, want_coef = R.clip_ref(g, max_norm)
    assert abs(float(norm) - want_norm) <= 1e-6 * want_norm
    assert abs(float(coef) - want_coef) <= 1e-6 * want_coef
    if want_norm < max_norm:
        assert float(coef) == 1.0
    else:
        assert float(coef) < 1.0


# ------------------------------------------------------------------------------------------ layout
def method_of(p, seed=0):
    return dlpm_amd.init_method_by_parameter(dict(p, device=DEV), rng='philox', seed=seed)


@pytest.mark.parametrize('shape', NETS)
def test_export_import_layout(shape):
    L = _lib.lib()
    net = R.toy_net(*shape, seed=3)
    h = net.native_handle()
    P = L.dlpm_mlp_param_floats(h)
    want = torch.nn.utils.parameters_to_vector([p.detach() for p in net.parameters()])
    assert P == want.numel()
    flat = torch.full((P,), float('nan'), device=DEV)
    _lib.check(L.dlpm_mlp_export_params_f32(h, flat.data_ptr(), P, stream()))
    assert torch.equal(flat.cpu(), want)
    # import a perturbed vector: the forward is that of a fresh net given the same weights through load_state_dict
    new = want + 0.05 * torch.randn(P, generator=torch.Generator().manual_seed(4))
    new_dev = new.to(DEV)
    _lib.check(L.dlpm_mlp_import_params_f32(h, new_dev.data_ptr(), P, stream()))
    back = torch.empty(P, device=DEV)
    _lib.check(L.dlpm_mlp_export_params_f32(h, back.data_ptr(), P, stream()))
    assert torch.equal(back.cpu(), new)
    carrier = R.toy_net(*shape, seed=5)
    torch.nn.utils.vector_to_parameters(new.clone(), carrier.parameters())
    fresh = R.toy_net(*shape, seed=6)
    fresh.load_state_dict(carrier.state_dict())
    x, t, _ = inputs(shape[0], 37, 8)
    assert torch.equal(net(x.to(DEV), t.to(DEV)), fresh(x.to(DEV), t.to(DEV)))


def test_sample_after_sync_is_the_sample_of_a_fresh_net():
    """The fused sampling loop reads the float4 copies and the per-timestep table: after two training steps and sync() the samples
    are those of a fresh net given the trained weights through load_state_dict -- and so are they straight after a step, without
    sync(), when the samplers captured before the step have been dropped."""
    p = R.toy_config()
    net = R.toy_net(seed=2)
    method = method_of(p, seed=1)
    before = method.sample({'default': net}, [64, 1, 2], 100)         # a captured sampler on the handle, built before training
    tr = dlpm_amd.MLPTrainer(net, method, lr=5e-3, ema_rates=[0.9])
    x = dlpm_amd.get_dataset(p, DEV, 0)[0][:256]
    tr.step(x)
    tr.step(x)
    mid = method_of(p, seed=9).sample({'default': net}, [64, 1, 2], 100)
    tr.sync()
    fresh = dlpm_amd.MLPModel(p)
    fresh.load_state_dict(net.state_dict())
    assert torch.equal(torch.nn.utils.parameters_to_vector([q.detach() for q in net.parameters()]), tr.theta.cpu())
    got = method_of(p, seed=9).sample({'default': net}, [64, 1, 2], 100)
    want = method_of(p, seed=9).sample({'default': fresh}, [64, 1, 2], 100)
    assert torch.equal(got, want) and torch.equal(mid, want)
    assert not torch.equal(want, before) and torch.isfinite(want).all()
    assert torch.equal(net(x, torch.rand(256, device=DEV, generator=torch.Generator(DEV).manual_seed(1))),
                       fresh(x, torch.rand(256, device=DEV, generator=torch.Generator(DEV).manual_seed(1))))


# ------------------------------------------------------------------------------------------ one step is its parts
def by_hand(net, method, x, kw, noise, lr, betas, eps, weight_decay, mu, grad_clip, step):
    """The entry points in order on a net of one's own; returns (theta, m, v, shadow, loss)."""
    L = _lib.lib()
    h = net.native_handle()
    P = L.dlpm_mlp_param_floats(h)
    theta = torch.empty(P, device=DEV)
    _lib.check(L.dlpm_mlp_export_params_f32(h, theta.data_ptr(), P, stream()))
    m, v, shadow = torch.zeros(P, device=DEV), torch.zeros(P, device=DEV), theta.clone()
    B = x.shape[0]
    if method.LIM:
        r = method._lim_loss_terms(net, x, None, method._lim_check_args(net, x, None, noise), keep=True)
        out, target, x_in, tvec, lp, outer, inner, idx = r['output'], r['score'], r['x_t'], r['t'], 1, 1, 1, None
    else:
        lp, outer, inner = int(kw.get('lploss', 2)), kw.get('monte_carlo_outer', 1), kw.get('monte_carlo_inner', 1)
        r = method._loss_terms(net, x, lp, outer, inner, None, None, noise, keep=True)
        out, target, x_in, tvec = r['model_eps'], r['eps_t'], r['x_in'], r['tvec']
        idx = torch.empty(B, dtype=torch.int32, device=DEV) if kw.get('loss_monte_carlo') == 'median' else None
    loss = method._loss_reduce(r['losses'], B, outer, inner, 'median' if idx is not None else 'mean', False, median_index=idx)
    dmodel = dev_loss_grad(out, target, r['losses'], idx, B, outer, inner, x.shape[2], lp)
    rows = x_in.shape[0]
    need = L.dlpm_mlp_backward_workspace_bytes(h, rows)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    grad = torch.empty(P, device=DEV)
    _lib.check(L.dlpm_mlp_backward_f32(h, x_in.data_ptr(), tvec.data_ptr(), dmodel.data_ptr(), rows, grad.data_ptr(), None, ws.data_ptr(),
                                       need, stream()))
    coef = None
    if grad_clip is not None:
        norm, coef = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        _lib.check(L.dlpm_grad_clip_coef_f32(grad.data_ptr(), P, grad_clip, norm.data_ptr(), coef.data_ptr(), stream()))
    a = _lib.AdamwArgs()
    a.theta_dev, a.grad_dev, a.exp_avg_dev, a.exp_avg_sq_dev, a.n = theta.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), P
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.step = lr, betas[0], betas[1], eps, weight_decay, step
    a.coef_dev, a.n_ema = _lib.ptr(coef), 1
    a.ema_dev[0], a.ema_mu[0] = shadow.data_ptr(), mu
    _lib.check(L.dlpm_adamw_step_f32(C.byref(a), stream()))
    _lib.check(L.dlpm_mlp_import_params_f32(h, theta.data_ptr(), P, stream()))
    return theta, m, v, shadow, loss


STEP_CASES = {'dlpm_mean': ('dlpm', dict(lploss=2.0)),
              'dlpm_median_3x2': ('dlpm', dict(lploss=1.0, loss_monte_carlo='median', monte_carlo_outer=3, monte_carlo_inner=2)),
              'lim': ('lim', {})}


@pytest.mark.parametrize('B', [13, 1024])
@pytest.mark.parametrize('case', list(STEP_CASES))
def test_one_step_is_its_parts(case, B):
    name, kw = STEP_CASES[case]
    p = R.toy_config(method=name)
    g = torch.Generator().manual_seed(B + len(case))
    x = dlpm_amd.get_dataset(p, DEV, 0)[0][:B].contiguous()
    if name == 'lim':
        noise = {'t': (torch.rand(B, generator=g) * 0.9 + 0.05).to(DEV), 'e': torch.randn(B, 1, 2, generator=g).to(DEV)}
    else:
        R_ = kw.get('monte_carlo_outer', 1) * kw.get('monte_carlo_inner', 1)
        noise = {'t': torch.randint(1, 100, (B,), generator=g), 'a': torch.rand(kw.get('monte_carlo_outer', 1) * B, generator=g) + 0.2,
                 'z': torch.randn(R_ * B, 1, 2, generator=g)}
    hyper = dict(lr=5e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    clip = 0.05 if case == 'dlpm_mean' else None
    net_a, net_b = R.toy_net(seed=4), R.toy_net(seed=4)
    tr = dlpm_amd.MLPTrainer(net_a, method_of(p), ema_rates=[0.9], grad_clip=clip, **hyper)
    loss = tr.step(x, noise=noise, **kw)
    theta, m, v, shadow, want_loss = by_hand(net_b, method_of(p), x, kw, noise, mu=0.9, grad_clip=clip, step=1, **hyper)
    assert torch.equal(loss, want_loss) and torch.isfinite(loss) and int(tr.last_flag) == 0
    assert torch.equal(tr.theta, theta) and torch.equal(tr.exp_avg, m) and torch.equal(tr.exp_avg_sq, v) and torch.equal(tr.shadows[0], shadow)
    assert tr.step_count == 1 and (m != 0).float().mean() > 0.9 and not torch.equal(theta, shadow)
    if clip is not None:
        assert float(tr.clip_coef) < 1.0                                    # the clip was active
    probe = torch.rand(B, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    assert torch.equal(net_a(x, probe), net_b(x, probe))                    # model(x, t) sees the new weights


def test_two_trainers_from_the_same_seeds_agree():
    p = R.toy_config()
    data = dlpm_amd.get_dataset(p, DEV, 0)[0]
    finals = []
    for _ in range(2):
        tr = dlpm_amd.MLPTrainer(R.toy_net(seed=8), method_of(p, seed=5), lr=5e-3, ema_rates=[0.9, 0.999], grad_clip=1.0)
        for i in range(5):
            tr.step(data[i * 300:(i + 1) * 300 + 1])
        finals.append((tr.theta.clone(), tr.shadows[1].clone()))
    assert torch.equal(finals[0][0], finals[1][0]) and torch.equal(finals[0][1], finals[1][1])
    assert torch.isfinite(finals[0][0]).all()


# ------------------------------------------------------------------------------------------ the manager
def manager(p, data, seed_net, **kw):
    net = R.toy_net(seed=seed_net)
    return dlpm_amd.TrainingManager({'default': net}, data, method_of(p, seed=3), None, None, None, ema_rates=[0.9], p=p, batch_size=128,
                                    seed=3, **kw)


def test_resume_equals_the_uninterrupted_run(tmp_path):
    """2 steps, save, load into a fresh manager (another initialisation), 2 more steps == 4 steps straight: parameters, moments,
    shadow and step count, bit for bit.  The saved optimizer entry loads into a real torch.optim.AdamW."""
    p = R.toy_config()
    data = dlpm_amd.get_dataset(p, DEV, 0)[0][:300]                 # 3 batches per epoch, the last one short
    kw = dict(max_batch_per_epoch=2, grad_clip=1.0)
    straight = manager(p, data, 1)
    straight.train(2, **kw)
    first = manager(p, data, 1)
    first.train(1, **kw)
    path = str(tmp_path / 'ck.pt')
    first.save(path)
    second = manager(p, data, 2)
    second.load(path)
    assert (second.epochs, second.total_steps, second.trainer.step_count) == (1, 2, 2)
    second.train(2, **kw)
    a, b = straight.trainer, second.trainer
    assert (straight.epochs, straight.total_steps, a.step_count) == (second.epochs, second.total_steps, b.step_count) == (2, 4, 4)
    assert torch.equal(a.theta, b.theta) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert torch.equal(a.shadows[0], b.shadows[0])
    assert len(straight.epoch_losses) == 2 and straight.epoch_losses[1] == second.epoch_losses[-1]
    ck = dlpm_amd.checkpoint.read_checkpoint(path)
    assert {'epoch', 'steps', 'model_parameters', 'optimizer', 'learning_schedule', 'ema_models'} <= set(ck)
    assert set(ck['ema_models'][0]) == {n for n, _ in first.models['default'].named_parameters()}
    opt = torch.optim.AdamW(dlpm_amd.MLPModel(p).parameters(), lr=1.0)
    opt.load_state_dict(ck['optimizer'])
    assert opt.param_groups[0]['lr'] == 0.005 and len(opt.state) == 60
    assert all(float(s['step']) == 2.0 for s in opt.state.values())


def test_a_non_finite_loss_is_reported_once_per_epoch():
    p = R.toy_config()
    data = dlpm_amd.get_dataset(p, DEV, 0)[0][:256].clone()
    data[7, 0, 1] = float('nan')
    tm = manager(p, data, 1)
    with pytest.raises(FloatingPointError, match='nan in loss detected'):
        tm.train(1)


def held_out_loss(p, net, test):
    """evaluate_loss on 4096 test-stream samples under a fixed key: a fresh method object per evaluation."""
    ev = dlpm_amd.EvaluationManager(method_of(p, seed=123), None, None, verbose=False)
    return ev.evaluate_loss({'default': net}, test[:4096], 1024)


def test_it_learns():
    """2d_data as shipped (gmm_grid, alpha = 1.8, T = 100, B = 1024, lr = 0.005, lploss = 2), 100 steps.  The reference recipe (torch
    AdamW on the same architecture and objective) on the CPU for three seeds goes from 1.42-1.60 at step 0 to 0.706-0.738 at step 100:
    the start must be above 1.3 and the end, of the net and of its EMA (mu = 0.9), below 0.80 -- the reference's worst end value plus
    twice its spread across seeds."""
    p = dlpm_amd.load_config('2d_data')
    torch.manual_seed(0)
    net = dlpm_amd.MLPModel(p)
    train, test = dlpm_amd.get_dataset(p, DEV, 0)
    start = held_out_loss(p, net, test)
    tm = dlpm_amd.TrainingManager({'default': net}, dlpm_amd.ToyLoader(train, p['training']['batch_size']), method_of(p), None, None, None,
                                  ema_rates=[0.9], p=p)
    losses = tm.train(4, max_batch_per_epoch=25, lploss=2.0)
    assert tm.total_steps == 100 and len(losses) == 4
    tm.sync()
    end = held_out_loss(p, net, test)
    ema = held_out_loss(p, tm.ema_model(0), test)
    print('held-out loss: start %.4f, after 100 steps %.4f, EMA %.4f; epoch means %s' % (start, end, ema, ['%.4f' % v for v in losses]))
    assert start > 1.3
    assert end < 0.80
    assert ema < 0.80


def test_cli_trains_saves_and_evaluates(tmp_path, capsys):
    path = str(tmp_path / 'toy.pt')
    losses = cli.main(['--config', '2d_data', '--set_seed', '0', '--train', '1', '--max_batch_per_epoch', '20', '--ema_rates', '0.9',
                       '--save', path])
    assert len(losses) == 1 and np.isfinite(losses[0]) and 'epoch 1 loss' in capsys.readouterr().out
    for extra in ([], ['--ema_eval']):
        res = cli.main(['--config', '2d_data', '--set_seed', '0', '--checkpoint', path, '--generate', '512', '--eval_2d'] + extra)
        assert all(np.isfinite(float(res[k])) for k in ('wass', 'mmd', 'precision', 'recall', 'f_1_pr'))
        assert 'eval_2d wass' in capsys.readouterr().out
    # train and evaluate in one run
    res = cli.main(['--config', '2d_data', '--set_seed', '0', '--train', '1', '--max_batch_per_epoch', '2', '--generate', '512', '--eval_2d'])
    assert np.isfinite(float(res['mmd']))
