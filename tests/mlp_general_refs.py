"""What the tests of the general toy-net forward share (tests/test_mlp_general_cpu.py pins the mirror on the CPU,
tests/test_gpu_mlp_general.py judges the kernel by it).

CASES      the architectures (F, nblocks, TE, nunits, group_norm, skip[, kernel]) and what each exercises
config     the 2d_data config at one of them
seeded_net MLPModel under manual_seed, LayerNorm weights and biases perturbed as tests/train_refs.py::toy_net does
forward    MLPModel.forward as plain torch functions of the state_dict, in the dtype asked for (fp32 or fp64), with or without
           LayerNorm and skip; oracle.nets.mlp_forward and train_refs.mlp_forward assume both
"""
import copy
import hashlib

import torch
import torch.nn.functional as F

import dlpm_amd

# (F, nblocks, TE, nunits, group_norm, skip, kernel)
CASES = {
    'u16_te7_nomid': (2, 0, 7, 16, True, True, 'auto'),        # one column tile, odd TE, no mid block
    'u72': (2, 1, 32, 72, True, True, 'auto'),                 # not a multiple of 16: LayerNorm over a padded tile
    'u80_noln': (3, 1, 48, 80, False, True, 'auto'),           # not a multiple of 32, no LayerNorm
    'u64_te96_noskip': (5, 1, 96, 64, True, False, 'auto'),    # the lane kernel's width, but TE > 64 and no skip
    'u128': (2, 1, 32, 128, True, True, 'auto'),               # first width beyond 64
    'u264_te130_plain': (2, 1, 130, 264, False, False, 'auto'),  # ragged TE and width across several K steps, both switches off
    'u1024': (1, 1, 32, 1024, True, True, 'auto'),             # the cap
    'shipped_general': (2, 4, 32, 64, True, True, 'general'),  # the shipped net on the new kernel
}


def config(nfeatures, nblocks, time_emb_size, nunits, group_norm=True, skip=True, method='dlpm'):
    p = copy.deepcopy(dlpm_amd.load_config('2d_data'))
    p['data']['nfeatures'] = nfeatures
    p['model'].update(nblocks=nblocks, time_emb_size=time_emb_size, nunits=nunits, group_norm=group_norm, skip_connection=skip)
    p['method'] = method
    return p


def perturb_norms_(net, seed):
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if 'group_norm' in name:
                p.add_(0.3 * torch.randn(p.shape, generator=g))
    return net


def seeded_net(case, seed=1, perturb=True, **kw):
    """The MLPModel of CASES[case] under manual_seed(seed); with `perturb` its LayerNorm weights and biases leave 1 and 0."""
    nf, nb, te, nu, gn, skip, kernel = CASES[case]
    torch.manual_seed(seed)
    net = dlpm_amd.MLPModel(config(nf, nb, te, nu, gn, skip), kernel=kw.pop('kernel', kernel), **kw)
    return perturb_norms_(net, seed) if perturb else net


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _norm(sd, pre, x, group_norm):
    return F.layer_norm(x, [x.shape[-1]], sd[pre + '.weight'], sd[pre + '.bias']) if group_norm else x


def _block(sd, pre, x, temb, group_norm, skip):
    h = F.silu(_norm(sd, pre + 'group_norm1', F.linear(x, sd[pre + 'mlp_1.1.weight'], sd[pre + 'mlp_1.1.bias']), group_norm))
    h = h + F.silu(F.linear(temb, sd[pre + 't_proj.1.weight'], sd[pre + 't_proj.1.bias']))
    h = _norm(sd, pre + 'group_norm2', F.linear(h, sd[pre + 'mlp_2.1.weight'], sd[pre + 'mlp_2.1.bias']), group_norm)
    if skip:
        h = h + x
    return F.silu(h)


def forward(sd, x, t, group_norm=True, skip=True, dtype=torch.float32):
    """x [rows, 1, F], t [rows] -> [rows, 1, F] in `dtype`; `sd` is the state_dict (any float dtype, cast here)."""
    sd = {k: v.detach().cpu().to(dtype) for k, v in sd.items()}
    x, t = x.detach().cpu().to(dtype), t.detach().cpu().to(dtype)
    temb = F.silu(F.linear(t.reshape(-1, 1, 1), sd['time_emb.weight'], sd['time_emb.bias']))
    temb = F.silu(F.linear(temb, sd['time_mlp.2.weight'], sd['time_mlp.2.bias']))
    h = F.silu(_norm(sd, 'group_norm_in', F.linear(x, sd['linear_in.weight'], sd['linear_in.bias']), group_norm))
    nb = len({k.split('.')[1] for k in sd if k.startswith('midblocks.')})
    for i in range(nb):
        h = _block(sd, 'midblocks.%d.' % i, h, temb, group_norm, skip)
    h = _block(sd, 'outblocks_mean.0.', h, temb, group_norm, skip)
    return F.linear(h, sd['outblocks_mean.1.weight'], sd['outblocks_mean.1.bias'])


def rel_l2(got, want):
    got, want = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    return float((got - want).norm() / want.norm())
