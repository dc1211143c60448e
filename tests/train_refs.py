"""Host mirrors the training tests judge by (tests/test_train_cpu.py pins them on the CPU, tests/test_gpu_train.py uses them).

mlp_forward      the toy net's forward in whatever dtype its inputs have (oracle.nets.mlp_forward casts t to fp32, so it cannot be
                 the float64 reference); any nblocks >= 0
loss_terms / loss_estimate   compute_loss_terms and the estimator in torch ops, differentiable
loss_grad_ref    the closed form include/dlpm_amd_train.h states for dlpm_loss_grad_f32, in fp64
adamw_ref        torch.optim.AdamW's update with EMA shadows, in fp64
clip_ref         clip_grad_norm_'s norm and coefficient, in fp64
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

import dlpm_amd


def toy_config(nfeatures=2, nblocks=4, time_emb_size=32, method='dlpm'):
    p = copy.deepcopy(dlpm_amd.load_config('2d_data'))
    p['data']['nfeatures'] = nfeatures
    p['model']['nblocks'] = nblocks
    p['model']['time_emb_size'] = time_emb_size
    p['method'] = method
    return p


def toy_net(nfeatures=2, nblocks=4, time_emb_size=32, seed=1):
    """A seeded MLPModel whose LayerNorm weights and biases are not at their initial 1 and 0 (so that every term of the backward is
    exercised)."""
    torch.manual_seed(seed)
    net = dlpm_amd.MLPModel(toy_config(nfeatures, nblocks, time_emb_size))
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if 'group_norm' in name:
                p.add_(0.3 * torch.randn(p.shape, generator=g))
    return net


def _block(sd, pre, x, temb):
    nu = x.shape[-1]
    h = F.layer_norm(F.linear(x, sd[pre + 'mlp_1.1.weight'], sd[pre + 'mlp_1.1.bias']), [nu], sd[pre + 'group_norm1.weight'],
                     sd[pre + 'group_norm1.bias'])
    h = F.silu(h) + F.silu(F.linear(temb, sd[pre + 't_proj.1.weight'], sd[pre + 't_proj.1.bias']))
    h = F.layer_norm(F.linear(h, sd[pre + 'mlp_2.1.weight'], sd[pre + 'mlp_2.1.bias']), [nu], sd[pre + 'group_norm2.weight'],
                     sd[pre + 'group_norm2.bias'])
    return F.silu(h + x)


def mlp_forward(sd, x, t):
    """x [rows, 1, F], t [rows] -> [rows, 1, F], in the dtype of sd / x / t (all the same)."""
    temb = F.silu(F.linear(t.reshape(-1, 1, 1), sd['time_emb.weight'], sd['time_emb.bias']))
    temb = F.silu(F.linear(temb, sd['time_mlp.2.weight'], sd['time_mlp.2.bias']))
    nu = sd['linear_in.weight'].shape[0]
    h = F.silu(F.layer_norm(F.linear(x, sd['linear_in.weight'], sd['linear_in.bias']), [nu], sd['group_norm_in.weight'],
                            sd['group_norm_in.bias']))
    nb = len({k.split('.')[1] for k in sd if k.startswith('midblocks.')})
    for i in range(nb):
        h = _block(sd, 'midblocks.%d.' % i, h, temb)
    h = _block(sd, 'outblocks_mean.0.', h, temb)
    return F.linear(h, sd['outblocks_mean.1.weight'], sd['outblocks_mean.1.bias'])


def autograd_grads(net, x, t, dout, dtype):
    """d <dout, net(x, t)> / d(parameters) and / dx by torch autograd on the CPU in `dtype`: ({name: grad}, dx)."""
    params = {n: p.detach().to(dtype).clone().requires_grad_(True) for n, p in net.named_parameters()}
    first = {id(p): n for n, p in net.named_parameters()}
    sd = {k: params[first[id(v)]] for k, v in net.state_dict(keep_vars=True).items()}
    xx = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    out = mlp_forward(sd, xx, t.detach().cpu().to(dtype))
    (out * dout.detach().cpu().to(dtype)).sum().backward()
    return {n: p.grad for n, p in params.items()}, xx.grad


# ------------------------------------------------------------------------------------------ the loss
def loss_terms(model_eps, target, lploss):
    """compute_loss_terms (GenerativeLevyProcess.py:19-31) over [rows, ...] -> [rows]."""
    d = (model_eps - target).reshape(model_eps.shape[0], -1)
    if lploss == 2:
        return torch.sqrt((d * d).mean(1))
    if lploss == 1:
        return F.smooth_l1_loss(model_eps.reshape(d.shape), target.reshape(d.shape), beta=1.0, reduction='none').mean(1)
    assert lploss == -1
    return (d * d).mean(1)


def loss_estimate(terms, B, outer, inner, median):
    """The estimator (:667-677).  Returns (loss, median index [B] or None)."""
    if not median:
        return terms.mean(), None
    m = terms.reshape(outer, inner, B).mean(1).median(0)
    return m.values.mean(), m.indices


def loss_grad_ref(model_eps, target, terms, median_index, B, outer, inner, D, lploss):
    """fp64 [outer * inner * B, D] from the fp32 (or fp64) inputs; `terms` are the ones the derivative is taken at."""
    me = torch.as_tensor(model_eps).detach().cpu().double().reshape(outer * inner * B, D)
    tg = torch.as_tensor(target).detach().cpu().double().reshape(outer * inner * B, D)
    tm = torch.as_tensor(terms).detach().cpu().double().reshape(-1, 1)
    d = me - tg
    if lploss == 2:
        g = torch.where(tm == 0, torch.zeros_like(d), d / (D * torch.where(tm == 0, torch.ones_like(tm), tm)))
    elif lploss == 1:
        g = d.clamp(-1, 1) / D
    else:
        g = 2 * d / D
    if median_index is None:
        w = torch.full((outer * inner * B, 1), 1.0 / (outer * inner * B), dtype=torch.float64)
    else:
        mi = torch.as_tensor(median_index).detach().cpu().long()
        o = torch.arange(outer).reshape(outer, 1, 1).expand(outer, inner, B)
        w = ((o == mi.reshape(1, 1, B)).double() / (inner * B)).reshape(-1, 1)
    return g * w


# ------------------------------------------------------------------------------------------ the optimizer
def adamw_ref(theta, g, m, v, lr, betas, eps, weight_decay, step, coef=None, shadows=(), mus=()):
    """One torch.optim.AdamW step (decoupled decay first) in fp64 from the given state; returns (theta, m, v, [shadows])."""
    theta, g, m, v = (torch.as_tensor(a).detach().cpu().double() for a in (theta, g, m, v))
    if coef is not None:
        g = g * float(coef)
    b1, b2 = betas
    theta = theta * (1 - lr * weight_decay)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    theta = theta - (lr / bc1) * m / (v.sqrt() / np.sqrt(bc2) + eps)
    out = [(1 - mu) * theta + mu * torch.as_tensor(s).detach().cpu().double() for s, mu in zip(shadows, mus)]
    return theta, m, v, out


def clip_ref(g, max_norm):
    """(norm, coef) of torch.nn.utils.clip_grad_norm_ in fp64."""
    norm = float(torch.as_tensor(g).detach().cpu().double().pow(2).sum().sqrt())
    return norm, min(1.0, max_norm / (norm + 1e-6))
