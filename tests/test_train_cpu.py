"""Training of the toy net, the part that needs no GPU: the header and its Python mirror, every refusal of
include/dlpm_amd_train.h before any launch, the host mirrors of tests/train_refs.py pinned against torch (autograd of the loss,
torch.optim.AdamW, clip_grad_norm_, oracle.nets.mlp_forward), the Python refusals and the optimizer entry of a checkpoint."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import dlpm_amd
from dlpm_amd import _lib, training
from oracle import nets
from test_host_mirror import build_unet
import train_refs as R

ERR_ARG, ERR_STATE, ERR_NOMEM = -1, -4, -5


# ------------------------------------------------------------------------------------------ refusals, before any launch
@pytest.fixture()
def unfinalized():
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.dlpm_mlp_create(2, 64, 4, 32, C.byref(h)))
    yield h
    L.dlpm_mlp_destroy(h)


def _host(n=64):
    """A host buffer standing for a device pointer: a refusal must come before anything touches it."""
    buf = np.zeros(n, dtype=np.float32)
    return buf, buf.ctypes.data


def test_layout_entry_points_refuse(unfinalized):
    L = _lib.lib()
    h = unfinalized
    assert L.dlpm_mlp_param_floats(None) < 0
    P = L.dlpm_mlp_param_floats(h)
    assert P == 55010 == sum(p.numel() for p in dlpm_amd.MLPModel(dlpm_amd.load_config('2d_data')).parameters())
    buf, ptr = _host()
    for fn in (L.dlpm_mlp_export_params_f32, L.dlpm_mlp_import_params_f32):
        assert fn(None, ptr, P, None) == ERR_ARG
        assert fn(h, None, P, None) == ERR_ARG
        assert fn(h, ptr, P - 1, None) == ERR_ARG
        assert fn(h, ptr, P, None) == ERR_STATE and b'finalize' in L.dlpm_last_error()
    for F, nb, TE in ((1, 0, 64), (5, 1, 7)):
        g = C.c_void_p()
        _lib.check(L.dlpm_mlp_create(F, 64, nb, TE, C.byref(g)))
        net = R.toy_net(F, nb, TE)
        assert L.dlpm_mlp_param_floats(g) == sum(p.numel() for p in net.parameters())
        L.dlpm_mlp_destroy(g)


def test_backward_refuses(unfinalized):
    L = _lib.lib()
    h = unfinalized
    buf, p = _host()
    assert L.dlpm_mlp_backward_workspace_bytes(None, 4) < 0 and L.dlpm_mlp_backward_workspace_bytes(h, 0) < 0
    need = L.dlpm_mlp_backward_workspace_bytes(h, 5)
    assert need > 0 and L.dlpm_mlp_backward_workspace_bytes(h, 65) > L.dlpm_mlp_backward_workspace_bytes(h, 64) > need
    ok = [h, p, p, p, 5, p, None, p, need, None]
    for i in (0, 1, 2, 3, 5, 7):
        a = list(ok)
        a[i] = None
        assert L.dlpm_mlp_backward_f32(*a) == ERR_ARG, i
    for rows in (0, -3):
        a = list(ok)
        a[4] = rows
        assert L.dlpm_mlp_backward_f32(*a) == ERR_ARG
    a = list(ok)
    a[8] = need - 1
    assert L.dlpm_mlp_backward_f32(*a) == ERR_NOMEM and b'workspace' in L.dlpm_last_error()
    assert L.dlpm_mlp_backward_f32(*ok) == ERR_STATE and b'finalize' in L.dlpm_last_error()


def test_loss_grad_refuses():
    L = _lib.lib()
    buf, p = _host()
    ok = [p, p, p, None, p, 4, 1, 1, 2, 2, None]
    for i in (0, 1, 2, 4):
        a = list(ok)
        a[i] = None
        assert L.dlpm_loss_grad_f32(*a) == ERR_ARG, i
    for i in (5, 6, 7, 8):
        a = list(ok)
        a[i] = 0
        assert L.dlpm_loss_grad_f32(*a) == ERR_ARG, i
    for lploss in (0, 3, -2):
        a = list(ok)
        a[9] = lploss
        assert L.dlpm_loss_grad_f32(*a) == ERR_ARG and b'lploss' in L.dlpm_last_error()
    a = list(ok)
    a[3], a[6] = p, 65
    assert L.dlpm_loss_grad_f32(*a) == ERR_ARG and b'64' in L.dlpm_last_error()


def test_clip_and_adamw_refuse():
    L = _lib.lib()
    buf, p = _host()
    assert L.dlpm_grad_clip_coef_f32(None, 4, 1.0, p, p, None) == ERR_ARG
    assert L.dlpm_grad_clip_coef_f32(p, 4, 1.0, None, p, None) == ERR_ARG
    assert L.dlpm_grad_clip_coef_f32(p, 4, 1.0, p, None, None) == ERR_ARG
    assert L.dlpm_grad_clip_coef_f32(p, 0, 1.0, p, p, None) == ERR_ARG
    assert L.dlpm_grad_clip_coef_f32(p, 4, 0.0, p, p, None) == ERR_ARG

    def args(**kw):
        a = _lib.AdamwArgs()
        a.theta_dev = a.grad_dev = a.exp_avg_dev = a.exp_avg_sq_dev = p
        a.n, a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.step, a.n_ema = 4, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert L.dlpm_adamw_step_f32(None, None) == ERR_ARG
    for bad in (dict(theta_dev=None), dict(grad_dev=None), dict(exp_avg_dev=None), dict(exp_avg_sq_dev=None), dict(n=0), dict(n_ema=9),
                dict(n_ema=-1), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(step=0), dict(step=-1), dict(n_ema=1),
                dict(lr=float('nan'))):
        assert L.dlpm_adamw_step_f32(C.byref(args(**bad)), None) == ERR_ARG, bad


# ------------------------------------------------------------------------------------------ the host mirrors, pinned
@pytest.mark.parametrize('shape', [(2, 4, 32), (1, 0, 64), (5, 1, 7)])
def test_forward_mirror_is_the_oracle_in_fp32(shape):
    """train_refs.mlp_forward in fp32 is oracle.nets.mlp_forward (which cannot run in fp64: it casts t); nblocks = 0 is beyond the
    oracle (it takes a max over the midblocks), so there only the two restated halves are compared."""
    F, nb, TE = shape
    net = R.toy_net(F, nb, TE)
    g = torch.Generator().manual_seed(3)
    x, t = 3 * torch.randn(9, 1, F, generator=g), torch.rand(9, generator=g)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    got = R.mlp_forward(sd, x, t)
    if nb > 0:
        assert torch.equal(got, nets.mlp_forward(sd, x, t))
    got64 = R.mlp_forward({k: v.double() for k, v in sd.items()}, x.double(), t.double())
    assert got64.dtype == torch.float64
    err = float((got.double() - got64).norm() / got64.norm())
    assert err < 1e-6, err


@pytest.mark.parametrize('lploss', [2, 1, -1])
@pytest.mark.parametrize('median', [False, True])
@pytest.mark.parametrize('outer,inner', [(1, 1), (3, 2)])
def test_loss_grad_mirror_against_autograd(lploss, median, outer, inner):
    B, D = 7, 6
    g = torch.Generator().manual_seed(10 * outer + lploss + 2)
    me = (1.5 * torch.randn(outer * inner * B, D, generator=g, dtype=torch.float64)).requires_grad_(True)
    tg = torch.randn(outer * inner * B, D, generator=g, dtype=torch.float64)
    terms = R.loss_terms(me, tg, lploss)
    loss, idx = R.loss_estimate(terms, B, outer, inner, median)
    loss.backward()
    got = R.loss_grad_ref(me, tg, terms, idx, B, outer, inner, D, lploss)
    torch.testing.assert_close(got, me.grad, rtol=1e-12, atol=0)
    if lploss == 1:
        assert ((me - tg).abs() > 1).any() and ((me - tg).abs() < 1).any()      # both branches of the smooth L1
    if median and outer > 1:
        assert (got.reshape(outer, inner, B, D) == 0).all(-1).any()              # unselected replicas get exact zeros


def test_adamw_mirror_against_torch():
    g = torch.Generator().manual_seed(5)
    n = 257
    theta0 = torch.randn(n, generator=g, dtype=torch.float64)
    lr, betas, eps, wd = 3e-3, (0.9, 0.999), 1e-8, 0.01
    p = theta0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    theta, m, v = theta0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    shadow = theta0.clone()
    for step in (1, 2, 3):
        grad = torch.randn(n, generator=g, dtype=torch.float64)
        p.grad = grad.clone()
        opt.step()
        theta, m, v, (shadow_new,) = R.adamw_ref(theta, grad, m, v, lr, betas, eps, wd, step, shadows=[shadow], mus=[0.9])
        assert torch.equal(shadow_new, (1. - 0.9) * theta + 0.9 * shadow)          # bem/utils_ema.py:27-28
        shadow = shadow_new
        st = opt.state[p]
        torch.testing.assert_close(theta, p.detach(), rtol=1e-12, atol=0)
        torch.testing.assert_close(m, st['exp_avg'], rtol=1e-12, atol=0)
        torch.testing.assert_close(v, st['exp_avg_sq'], rtol=1e-12, atol=0)
    t2 = R.adamw_ref(theta, grad, m, v, lr, betas, eps, wd, 4, coef=0.25)[0]
    torch.testing.assert_close(t2, R.adamw_ref(theta, 0.25 * grad, m, v, lr, betas, eps, wd, 4)[0], rtol=1e-15, atol=0)


@pytest.mark.parametrize('max_norm', [0.5, 1e3])
def test_clip_mirror_against_torch(max_norm):
    g = torch.Generator().manual_seed(6)
    parts = [torch.randn(s, generator=g, dtype=torch.float64).requires_grad_(True) for s in (5, 17, 3)]
    for q in parts:
        q.grad = torch.randn(q.shape, generator=g, dtype=torch.float64)
    flat = torch.cat([q.grad.clone() for q in parts])
    total = torch.nn.utils.clip_grad_norm_(parts, max_norm)
    norm, coef = R.clip_ref(flat, max_norm)
    assert abs(norm - float(total)) <= 1e-12 * norm
    torch.testing.assert_close(torch.cat([q.grad for q in parts]), flat * coef, rtol=1e-12, atol=0)
    assert (coef == 1.0) == (norm < max_norm)


# ------------------------------------------------------------------------------------------ Python refusals, checkpoints
def _method(p):
    p = dict(p, device='cpu')
    return dlpm_amd.init_method_by_parameter(p, rng='philox', seed=0)


def test_trainers_refuse_what_is_out_of_scope():
    p = R.toy_config()
    method = _method(p)
    unet = build_unet('tiny')[0]
    with pytest.raises(NotImplementedError, match='DESIGN'):
        training.MLPTrainer(unet, method, lr=1e-3)
    data = torch.zeros(8, 1, 2)
    with pytest.raises(NotImplementedError, match='DESIGN'):
        training.TrainingManager({'default': unet}, data, method, None, None, None, p=p, batch_size=4)
    net = dlpm_amd.MLPModel(p)
    with pytest.raises(NotImplementedError, match='AdamW'):
        training.TrainingManager({'default': net}, data, method, torch.optim.SGD(net.parameters(), lr=0.1), None, None, p=p, batch_size=4)
    with pytest.raises(NotImplementedError, match='steplr'):
        training.TrainingManager({'default': net}, data, method, None, 'linear', None, p=p, batch_size=4)
    with pytest.raises(ValueError, match='EMA'):
        training.MLPTrainer(net, method, lr=1e-3, ema_rates=[0.9] * 9)
    tm = training.TrainingManager({'default': net}, data, method, torch.optim.AdamW(net.parameters(), lr=0.02, betas=(0.8, 0.99)), 'steplr',
                                  None, p=p, batch_size=4)
    assert tm._opt == dict(lr=0.02, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.01) and tm.exists_ls() and tm.lr_step_size == 400
    tm = training.TrainingManager({'default': net}, data, method, None, None, None, p=p)
    assert tm._opt['lr'] == 0.005 and tm.batch_size == 1024 and not tm.exists_ls()
    ref = ['models', 'data', 'method', 'optimizers', 'learning_schedules', 'eval', 'logger', 'ema_rates', 'reset_models']
    assert list(inspect.signature(training.TrainingManager.__init__).parameters)[1:10] == ref


def test_checkpoint_optimizer_entry_loads_into_torch_adamw(tmp_path):
    """save_checkpoint with optimizers=: the stored entry is what torch.optim.AdamW.load_state_dict takes, over
    model.parameters() order; without it the file is what it was."""
    p = R.toy_config()
    net = dlpm_amd.MLPModel(p)
    names = [n for n, _ in net.named_parameters()]
    assert len(names) == 60
    opt = torch.optim.AdamW(net.parameters(), lr=0.005)
    for q in net.parameters():
        q.grad = torch.full_like(q, 0.5)
    opt.step()
    sd = opt.state_dict()
    path = dlpm_amd.checkpoint.save_checkpoint(str(tmp_path / 'a.pt'), {'default': net}, epoch=3, steps=7, optimizers={'default': sd},
                                               learning_schedules={'default': {'last_epoch': 7}})
    ck = dlpm_amd.checkpoint.read_checkpoint(path)
    assert set(ck) == {'epoch', 'steps', 'model_parameters', 'optimizer', 'learning_schedule'} and ck['learning_schedule'] == {'last_epoch': 7}
    fresh = torch.optim.AdamW(dlpm_amd.MLPModel(p).parameters(), lr=1.0)
    fresh.load_state_dict(ck['optimizer'])
    assert fresh.param_groups[0]['lr'] == 0.005 and len(fresh.state) == 60
    # the form MLPTrainer.state_dict() writes, from flat vectors in parameters_to_vector order
    shapes = [tuple(q.shape) for q in net.parameters()]
    flat_m = torch.nn.utils.parameters_to_vector([opt.state[q]['exp_avg'] for q in net.parameters()])
    flat_v = torch.nn.utils.parameters_to_vector([opt.state[q]['exp_avg_sq'] for q in net.parameters()])
    mine = training.optimizer_state_dict(names, shapes, flat_m, flat_v, 1, 0.005, (0.9, 0.999), 1e-8, 0.01)
    assert set(mine['param_groups'][0]) == set(sd['param_groups'][0]) and mine['param_groups'][0]['params'] == list(range(60))
    for i in range(60):
        assert float(mine['state'][i]['step']) == float(sd['state'][i]['step']) == 1.0
        assert torch.equal(mine['state'][i]['exp_avg'], sd['state'][i]['exp_avg'])
        assert torch.equal(mine['state'][i]['exp_avg_sq'], sd['state'][i]['exp_avg_sq'])
    again = torch.optim.AdamW(dlpm_amd.MLPModel(p).parameters(), lr=1.0)
    again.load_state_dict(mine)
    assert len(again.state) == 60 and again.param_groups[0]['betas'] == (0.9, 0.999)
    assert training.optimizer_state_dict(names, shapes, flat_m, flat_v, 0, 0.005, (0.9, 0.999), 1e-8, 0.01)['state'] == {}
    plain = dlpm_amd.checkpoint.read_checkpoint(dlpm_amd.checkpoint.save_checkpoint(str(tmp_path / 'b.pt'), {'default': net}))
    assert plain['optimizer'] is None and plain['learning_schedule'] is None and set(plain) == set(ck)
