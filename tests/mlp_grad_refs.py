"""What the tests of the toy net's gradients at any width share (tests/test_mlp_grad_cpu.py pins the mirror on the CPU,
tests/test_gpu_mlp_grad.py judges the kernels and the autograd bridge by it).

forward          mlp_general_refs.forward with the graph kept: the same functions (its _norm and _block) on tensors that are not
                 detached, so torch.autograd differentiates it; test_mlp_grad_cpu.py checks it returns mlp_general_refs.forward's bits
autograd_grads   d <dout, net(x, t)> / d(parameters) and / dx of that mirror on the CPU, in float64 (the reference) or float32 (the
                 yardstick)
module_forward   the same net through the MLPModel container's own torch modules, as the reference's Model.forward walks them
judge            per tensor err_dev <= K * err_torch32, the form of tests/test_gpu_train.py::judge
"""
import torch
import torch.nn.functional as F

import mlp_general_refs as G

ROW_CHUNK = 64      # rows per chunk of the weight pass: GEN_GRAD_RC, dlpm_amd/csrc/mlp_pack.h:102
MAX_SLOTS = 16      # gradient-sized partial buffers at most: GEN_GRAD_SLOTS, dlpm_amd/csrc/mlp_pack.h:103
ROWS = [1, 15, 16, 17, 33, 69, ROW_CHUNK + 1]


def forward(sd, x, t, group_norm=True, skip=True):
    """mlp_general_refs.forward on tensors as they are (one dtype, on the CPU), keeping the graph."""
    temb = F.silu(F.linear(t.reshape(-1, 1, 1), sd['time_emb.weight'], sd['time_emb.bias']))
    temb = F.silu(F.linear(temb, sd['time_mlp.2.weight'], sd['time_mlp.2.bias']))
    h = F.silu(G._norm(sd, 'group_norm_in', F.linear(x, sd['linear_in.weight'], sd['linear_in.bias']), group_norm))
    nb = len({k.split('.')[1] for k in sd if k.startswith('midblocks.')})
    for i in range(nb):
        h = G._block(sd, 'midblocks.%d.' % i, h, temb, group_norm, skip)
    h = G._block(sd, 'outblocks_mean.0.', h, temb, group_norm, skip)
    return F.linear(h, sd['outblocks_mean.1.weight'], sd['outblocks_mean.1.bias'])


def leaf_state(net, dtype):
    """({parameter name: leaf tensor in `dtype` on the CPU}, the state_dict over those leaves -- aliases share their leaf)."""
    params = {n: p.detach().cpu().to(dtype).clone().requires_grad_(True) for n, p in net.named_parameters()}
    first = {id(p): n for n, p in net.named_parameters()}
    sd = {k: params[first[id(v)]] for k, v in net.state_dict(keep_vars=True).items()}
    return params, sd


def autograd_grads(net, x, t, dout, dtype):
    """({name: grad}, dx) of <dout, net(x, t)> by torch.autograd over the mirror on the CPU in `dtype`."""
    params, sd = leaf_state(net, dtype)
    xx = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    out = forward(sd, xx, t.detach().cpu().to(dtype), net.group_norm, net.skip_connection)
    (out * dout.detach().cpu().to(dtype)).sum().backward()
    return {n: p.grad for n, p in params.items()}, xx.grad


def module_forward(net, x, t):
    """Model.forward (dlpm/models/Model.py:186-211, DiffusionBlocks.py:125-136) over the container's own modules, on the CPU."""
    temb = net.time_mlp(t.reshape(-1, 1, 1))
    h = net.inblock(x)

    def block(blk, v):
        y = F.silu(blk.mlp_1(v)) + blk.t_proj(temb)
        y = blk.mlp_2(y)
        return F.silu(y + v if net.skip_connection else y)

    for blk in net.midblocks:
        h = block(blk, h)
    return net.outblocks_mean[1](block(net.outblocks_mean[0], h))


def inputs(nfeatures, rows, seed):
    g = torch.Generator().manual_seed(seed)
    return 3 * torch.randn(rows, 1, nfeatures, generator=g), torch.rand(rows, generator=g), torch.randn(rows, 1, nfeatures, generator=g)


def rel(a, b):
    """||a - b||_2 / ||b||_2 in fp64 (the plain norm of the difference where b vanishes)."""
    a, b = a.detach().cpu().double().reshape(-1), b.detach().cpu().double().reshape(-1)
    n = float(b.norm())
    d = float((a - b).norm())
    return d / n if n > 0 else d


def split(net, flat):
    out, off = {}, 0
    for n, p in net.named_parameters():
        out[n] = flat[off:off + p.numel()].reshape(p.shape)
        off += p.numel()
    assert off == flat.numel()
    return out


def judge(tag, K, got, got_dx, g64, dx64, g32, dx32, lines=None):
    """Per tensor and for dx: print the three figures, then finite, err_dev <= K * err_torch32, and exactly 0 where the float64
    gradient is exactly 0.  Returns the worst ratio; `lines` collects the printed table."""
    worst, bad = 0.0, []
    rows = [(n, got[n], g64[n], g32[n]) for n in g64] + ([('dx', got_dx, dx64, dx32)] if got_dx is not None else [])
    for n, a, r64, r32 in rows:
        assert torch.isfinite(a).all(), (tag, n)
        if not r64.any():
            assert not a.any(), (tag, n, 'the float64 gradient is exactly 0')
        e_dev, e_32 = rel(a, r64), rel(r32, r64)
        ratio = e_dev / e_32 if e_32 > 0 else (0.0 if e_dev == 0 else float('inf'))
        worst = max(worst, ratio)
        line = '%s %-40s err_dev %.3e err_torch32 %.3e ratio %.2f' % (tag, n, e_dev, e_32, ratio)
        print(line)
        if lines is not None:
            lines.append(line)
        if not e_dev <= K * e_32:
            bad.append((n, e_dev, e_32))
    print('%s worst ratio %.2f' % (tag, worst))
    assert not bad, (tag, bad)
    return worst
