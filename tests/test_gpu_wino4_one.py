"""3x3 stride-1 convolutions on 4x4-pixel tensors through the one-tile F(4x4,3x3) kernel (conv_wino4.hip: k_conv3x3_wino4_one, 16 whole
images x 64 channels per workgroup, the K loop split over two groups of four waves; force_direct bit 9 = value 512 of dlpm_conv2d_f32,
with bit 3) against F.conv2d in float64 and against the forced 8-wave F(4x4) kernel on blocks of 16 one-tile images (bit 3 alone)."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest
import torch

from dlpm_amd import _lib
from test_gpu_kernels import DEV, L, ref_conv, run_conv, st

pytestmark = pytest.mark.gpu

F4, ONE = 8, 8 | 512


def conv(x0, w, bias=None, x1=None, coef=None, silu=False, res=None, force=ONE, stats=False):
    Cout, Cin = w.shape[:2]
    # behind the helper's own scratch: the F(4x4,3x3) copy and the one-tile copy, 36 floats per filter each, and their paddings
    return run_conv(x0, w, bias, x1, 1, 0, coef, silu, res, force_direct=force, scratch_extra=72 * Cout * Cin + 8192, stats=stats)


def forced_f4(x0, w, bias=None, x1=None, coef=None, silu=False, res=None):
    """The same convolution on the 8-wave F(4x4) kernel (bit 3 alone).  On blocks of 16 one-tile images that kernel exists for the
    128-channel n-tile only (the narrow shapes' raw buffer does not hold 16 6x6 patches: bit 3 is an error there), so a 64-channel
    layer rides in a 128-channel launch with every filter, bias and residual channel twice; a wave's 16 output channels do not depend
    on the others, and the first Cout channels are the layer's."""
    Cout = w.shape[0]
    if Cout % 128 == 0:
        return conv(x0, w, bias, x1, coef, silu, res, force=F4)
    twice = lambda v: None if v is None else torch.cat([v, v], 0 if v.dim() != 4 or v is w else 1)
    return conv(x0, twice(w), twice(bias), x1, coef, silu, twice(res), force=F4)[:, :Cout].contiguous()


def make(name, B, C0, C1, Cout, use_bias, act, use_res, H=4):
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    Cin = C0 + C1
    x0 = torch.randn(B, C0, H, H, generator=g)
    x1 = torch.randn(B, C1, H, H, generator=g) if C1 else None
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    bias = torch.randn(Cout, generator=g) if use_bias else None
    # coefficients with a non-zero shift: silu(0 A + B) != 0, so a border that is zeroed BEFORE the activation shows
    coef = (1 + 0.3 * torch.randn(B, Cin, generator=g), 0.5 + 0.3 * torch.randn(B, Cin, generator=g)) if act else None
    res = torch.randn(B, Cout, H, H, generator=g) if use_res else None
    return x0, w, bias, x1, coef, act, res


CASES = [
    # name, B, C0, C1, Cout, bias, coefficients + SiLU, residual
    ('one_image', 1, 16, 0, 64, False, False, False),             # one phase per K half, 15 absent images in the block
    ('ragged_two_blocks', 19, 32, 0, 128, True, False, False),    # second block ragged, two n-tiles
    ('concat_gn_silu_res', 3, 8, 24, 64, False, True, True),      # concat boundary inside half 0; border zero AFTER the activation
    ('long_k', 2, 256, 256, 64, False, False, False),             # 32 phases per half, ring wrap
    ('cifar_shape', 17, 256, 0, 256, False, True, True),          # the step's own layer at a small batch
]
# max |kernel - fp64 reference| measured on MI355X (profiles/wino4_one/test_gpu_wino4_one.txt), for the record -- the bound below is
# relative to the 8-wave kernel's error in the same run: (one-tile kernel, forced 8-wave F(4x4) kernel)
ONE_MEASURED = {'one_image': (1.61e-06, 2.02e-06),
                'ragged_two_blocks': (3.28e-06, 4.59e-06),
                'concat_gn_silu_res': (2.03e-06, 2.74e-06),
                'long_k': (7.39e-06, 1.22e-05),
                'cifar_shape': (5.36e-06, 8.23e-06)}


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_one_tile_against_fp64_and_the_forced_f4_kernel(case):
    """Error against the float64 convolution <= 1.5x the forced 8-wave F(4x4) kernel's on the same inputs (the project's rule for a
    replacement kernel; the one-tile kernel halves that kernel's accumulation chains), never above 2e-5 (test_conv_winograd_f4's cap);
    and at least one bit differs from the 8-wave kernel's output, i.e. the new kernel ran."""
    name = case[0]
    x0, w, bias, x1, coef, act, res = make(*case)
    want = ref_conv(x0, w, bias, x1, 1, 0, coef, act, res)
    new = conv(x0, w, bias, x1, coef, act, res, force=ONE)
    old = forced_f4(x0, w, bias, x1, coef, act, res)
    assert new.shape == want.shape == old.shape
    e_new, e_old = (new - want).abs().max().item(), (old - want).abs().max().item()
    print('%s: one-tile err %.2e, 8-wave F(4x4) err %.2e' % (name, e_new, e_old))
    assert e_new <= 1.5 * e_old and e_new < 2e-5, (name, e_new, e_old)
    assert not torch.equal(new, old), 'the one-tile kernel did not run (identical to the 8-wave kernel)'


def test_one_tile_batch_independence():
    """Image k convolved alone is bit-identical to image k inside the batch (second block ragged)."""
    x0, w, bias, x1, coef, act, res = make(*CASES[1])
    full = conv(x0, w, bias)
    for k in (0, 15, 16, 18):
        one = conv(x0[k:k + 1], w, bias)
        assert torch.equal(one[0], full[k]), k


@pytest.mark.parametrize('Cin,H', [(24, 4), (16, 8)], ids=['cin24', '8x8_image'])
def test_bit_9_is_an_error_where_the_kernel_does_not_take_the_geometry(Cin, H):
    """Cin = 24 (an odd number of 8-channel chunks) and 8x8 images: the bit asks for its kernel, never a silent fall-back."""
    x0, w, bias, x1, coef, act, res = make('unsupported', 2, Cin, 0, 128, True, False, False, H=H)
    with pytest.raises(_lib.DlpmError, match='one-tile'):
        conv(x0, w, bias, force=ONE)
    old = conv(x0, w, bias, force=F4)          # (the F(4x4) kernel of bit 3 takes both)
    assert (old - ref_conv(x0, w, bias, None, 1, 0)).abs().max().item() < 2e-5


@pytest.mark.parametrize('B', [3, 19])
def test_one_tile_statistics_partials(B):
    """One (mean, M2) partial per image and channel, [B][1][Cout]: against the float64 mean and centred sum of squares of the kernel's
    own output, and dlpm_groupnorm_coeffs_from_stats_f32 on them against the float64 GroupNorm of that output.  Tolerances of
    tests/test_gpu_gn_stats.py."""
    x0, w, bias, x1, coef, act, res = make('one_stats', B, 32, 32, 128, True, True, True)
    out, part, px = conv(x0, w, bias, x1, coef, act, res, stats=True)
    assert px == 16
    Cout = 128
    p = part.view(B, 1, Cout, 2).double()
    assert bool(torch.isfinite(p).all())
    o = out.double()
    want_m = o.mean(dim=(2, 3))
    want_M2 = ((o - want_m[:, :, None, None]) ** 2).sum(dim=(2, 3))
    assert (p[:, 0, :, 0] - want_m).abs().max() < 1e-5
    assert ((p[:, 0, :, 1] - want_M2).abs() / (1 + want_M2)).max() < 1e-5
    assert torch.equal(out, conv(x0, w, bias, x1, coef, act, res))      # the statistics epilogue leaves the output's bits alone
    # the consumer: GroupNorm coefficients from these partials
    g = torch.Generator().manual_seed(77)
    gamma, beta = 1 + 0.2 * torch.randn(Cout, generator=g), 0.2 * torch.randn(Cout, generator=g)
    groups = 32
    cA, cB = torch.empty(B, Cout, device=DEV), torch.empty(B, Cout, device=DEV)
    pd, gd, bd = part[:2 * B * Cout].to(DEV).contiguous(), gamma.to(DEV), beta.to(DEV)
    _lib.check(L().dlpm_groupnorm_coeffs_from_stats_f32(pd.data_ptr(), None, Cout, 0, B, 1, 1, 16, groups, gd.data_ptr(), bd.data_ptr(),
                                                        None, 0, 0, cA.data_ptr(), cB.data_ptr(), st()))
    torch.cuda.synchronize()
    og = o.view(B, groups, -1)
    mu, var = og.mean(dim=2), og.var(dim=2, unbiased=False)
    rstd = (1.0 / torch.sqrt(var + 1e-5)).repeat_interleave(Cout // groups, dim=1)
    mu = mu.repeat_interleave(Cout // groups, dim=1)
    wantA = rstd * gamma.double()
    wantB = beta.double() - mu * wantA
    assert (cA.cpu().double() - wantA).abs().max() < 1e-5 * wantA.abs().max()
    assert (cB.cpu().double() - wantB).abs().max() < 1e-5 * (1 + wantB.abs().max())


_NET_SCRIPT = r"""
import ctypes as C, hashlib, sys, torch
sys.path.insert(0, sys.argv[1])
import dlpm_amd
from dlpm_amd import _lib
from oracle import nets
torch.manual_seed(31)
net = dlpm_amd.UNetModel(3, 128, 3, 1, [2], channel_mult=[1, 2], num_heads=4, use_scale_shift_norm=True)
dlpm_amd.rerandomize_(net, 32)
net.set_conv_policy('auto', 1024)   # the flagship's declaration: AUTO takes the one-tile shape under a declared batch that fills the chip
g = torch.Generator().manual_seed(33)
x, t = torch.randn(3, 3, 8, 8, generator=g), torch.rand(3, generator=g)
sd = {k: v.detach() for k, v in net.state_dict().items()}
with torch.no_grad():
    want = nets.unet_forward(sd, x, t, 4)
got = net(x.to('cuda'), t.to('cuda')).cpu()
L = _lib.lib()
_lib.check(L.dlpm_prof_enable(1))
again = net(x.to('cuda'), t.to('cuda')).cpu()
buf = C.create_string_buffer(1 << 16)
_lib.check(L.dlpm_prof_report(buf, len(buf)))
_lib.check(L.dlpm_prof_enable(0))
assert torch.equal(again, got)
classes = sorted({ln.split()[0].split(':')[0] for ln in buf.value.decode().strip().splitlines()})
print('NETERR %.6g' % (got - want).abs().max().item())
print('NETDIGEST ' + hashlib.sha256(got.numpy().tobytes()).hexdigest())
print('NETCLASSES ' + ','.join(classes))
# the sampler on the CIFAR architecture (test_host_mirror.UNETS['cifar']: levels of 32, 16, 8 and 4 pixels; its head carries the update,
# which the two-chain step needs)
torch.manual_seed(1234)
net = dlpm_amd.UNetModel(3, 128, 3, 2, [4, 8, 16], channel_mult=[1, 2, 2, 2], num_heads=4, use_scale_shift_norm=True)
dlpm_amd.rerandomize_(net, 4321)
net.set_conv_policy('auto', 1024)
m = dlpm_amd.GenerativeLevyProcess(1.7, 'cuda', 4, rescale_timesteps=True, seed=42, use_graph=True)
xs = m.sample({'default': net}, [4, 3, 32, 32], 4, clamp_a=10.0, clamp_eps=50.0).cpu()
(ent,) = m._samplers.values()
print('CHAINS %d' % L.dlpm_sampler_chains(ent['h']))
m.close()
assert bool(torch.isfinite(xs).all())
print('STATEDIGEST ' + hashlib.sha256(xs.numpy().tobytes()).hexdigest())
"""


def _child(env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-c', _NET_SCRIPT, root], env=dict(os.environ, **env), cwd=root, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return {ln.split()[0]: ln.split()[1] for ln in r.stdout.splitlines() if ln.split() and ln.split()[0].isupper()}


@pytest.fixture(scope='module')
def net_runs():
    return {(one, chains): _child({'DLPM_WINO4_ONE': one, 'DLPM_SAMPLER_CHAINS': chains}) for one, chains in (('1', '2'), ('0', '2'), ('1', '1'))}


def test_one_tile_through_the_net(net_runs):
    """The mc = 128 [1, 2] net of test_subpixel_through_the_net on 8x8 images (its second level is 4x4 pixels x 256 channels) with the
    route on (default; a declared batch of 1024) and off (DLPM_WINO4_ONE=0, read once per process: one child each): both within that test's 1e-5 of the oracle,
    not the same bits, and the launches report under their own profile class exactly when the route is on."""
    on, off = net_runs[('1', '2')], net_runs[('0', '2')]
    print('UNet mc=128 [1,2] 8x8 B=3: max |hip - oracle| one-tile route on %s, off %s' % (on['NETERR'], off['NETERR']))
    assert float(on['NETERR']) < 1e-5 and float(off['NETERR']) < 1e-5
    assert on['NETDIGEST'] != off['NETDIGEST']
    assert 'conv3x3_wino4_one' in on['NETCLASSES'].split(',') and 'conv3x3_wino4_one' not in off['NETCLASSES'].split(',')


def test_one_tile_sampler_state_is_the_same_on_one_chain_and_two(net_runs):
    """Three reverse steps (T = 4) of the CIFAR architecture, B = 4, the route on: the two half-batch chains give the bits of the
    one-chain step."""
    two, one = net_runs[('1', '2')], net_runs[('1', '1')]
    assert (two['CHAINS'], one['CHAINS']) == ('2', '1')
    assert two['STATEDIGEST'] == one['STATEDIGEST']
    assert two['NETDIGEST'] == one['NETDIGEST']
