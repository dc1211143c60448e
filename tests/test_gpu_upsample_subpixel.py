"""The nearest-x2 Upsample convolutions as four parity-class Winograd F(4x4,2x2) convolutions on the low-res image
(conv_wino4.hip: k_conv3x3_wino4sp, force_direct bit 8 = value 256 of dlpm_conv2d_f32) against F.interpolate + F.conv2d in
float64 and against the kernel it replaces (bit 3 alone: the UPS instantiation of k_conv3x3_wino4)."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest
import torch

from dlpm_amd import _lib
from oracle import nets
from test_gpu_kernels import DEV, L, nchw, nhwc, ref_conv, st

pytestmark = pytest.mark.gpu

F4, SP = 8, 8 | 256


def run_conv(x0, w, bias=None, x1=None, coef=None, silu=False, res=None, force=SP, stats=False):
    """Upsampling 3x3 convolution of NCHW cpu tensors through dlpm_conv2d_f32 (or dlpm_conv2d_stats_f32); NCHW cpu output
    (and the statistics partials [B][nt][Cout][2] with their pixel count)."""
    B, C0, Hin, Win = x0.shape
    Cout, Cin = w.shape[:2]
    a = _lib.ConvArgs()
    keep = []

    def dev(t):
        t = t.to(DEV).contiguous()
        keep.append(t)
        return t.data_ptr()
    a.src0, a.C0 = dev(nhwc(x0)), C0
    if x1 is not None:
        a.src1, a.C1 = dev(nhwc(x1)), x1.shape[1]
    a.B, a.Hin, a.Win, a.Hout, a.Wout = B, Hin, Win, 2 * Hin, 2 * Win
    a.ksize, a.stride, a.upsample = 3, 1, 1
    a.weight = dev(w)
    if bias is not None:
        a.bias = dev(bias)
    if coef is not None:
        a.coefA, a.coefB = dev(coef[0]), dev(coef[1])
    a.act_silu = int(silu)
    if res is not None:
        a.res0, a.R0 = dev(nhwc(res)), Cout
    out = torch.empty(B, 2 * Hin, 2 * Win, Cout, device=DEV)
    a.out, a.Cout, a.force_direct = out.data_ptr(), Cout, force
    # direct + fragment + F(2x2) + F(4x4,3x3) + sub-pixel copies: 9 + 9 + 16 + 36 + 104 floats per filter, and their paddings
    scratch = torch.empty(200 * Cout * Cin + 64 * 1024 * (1 + Cout // 32), device=DEV)
    a.scratch_floats = scratch.numel()
    if not stats:
        _lib.check(L().dlpm_conv2d_f32(C.byref(a), scratch.data_ptr(), st()))
        torch.cuda.synchronize()
        return nchw(out).cpu()
    fn = L().dlpm_conv2d_stats_f32
    part = torch.full((B * (4 * Hin * Win // 64) * Cout * 2,), float('nan'), device=DEV)
    px = C.c_int32(0)
    _lib.check(fn(C.byref(a), scratch.data_ptr(), part.data_ptr(), C.byref(px), st()))
    torch.cuda.synchronize()
    nt = 4 * Hin * Win // px.value
    return nchw(out).cpu(), part[:B * nt * Cout * 2].view(B, nt, Cout, 2).cpu(), px.value


def make(name, B, C0, C1, Hlo, Wlo, Cout, act, use_res):
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    Cin = C0 + C1
    x0 = torch.randn(B, C0, Hlo, Wlo, generator=g)
    x1 = torch.randn(B, C1, Hlo, Wlo, generator=g) if C1 else None
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    bias = torch.randn(Cout, generator=g)
    coef = (1 + 0.3 * torch.randn(B, Cin, generator=g), 0.3 * torch.randn(B, Cin, generator=g)) if act else None
    res = torch.randn(B, Cout, 2 * Hlo, 2 * Wlo, generator=g) if use_res else None
    return x0, w, bias, x1, coef, act, res


CASES = [
    # name, B, C0, C1, low-res H, W, Cout, coef + silu, res
    ('sp_16to32_one_image', 1, 16, 0, 16, 16, 128, False, False),          # one image per block, all four classes, two phases
    ('sp_8to16_four_images_ragged', 5, 32, 0, 8, 8, 256, False, False),    # four images per block, ragged last block, two n-tiles
    ('sp_16x8_concat_gn_silu_res', 2, 24, 8, 16, 8, 128, True, True),      # non-square, concat boundary inside a phase, padding after SiLU
    ('sp_long_k', 1, 256, 256, 8, 8, 128, False, False),                   # K = 512
]
# max |kernel - fp64 reference| measured on MI355X (profiles/wino4_subpixel/kernels_subpixel.txt), for the record -- the bound below is
# relative to the UPS kernel's error in the same run: (sub-pixel kernel, UPS kernel)
SP_MEASURED = {'sp_16to32_one_image': (4.23e-06, 4.77e-06),
               'sp_8to16_four_images_ragged': (6.14e-06, 5.45e-06),
               'sp_16x8_concat_gn_silu_res': (5.13e-06, 4.05e-06),
               'sp_long_k': (1.59e-05, 1.86e-05)}


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_subpixel_against_fp64_and_the_kernel_it_replaces(case):
    """Error against the float64 convolution <= 1.5x the UPS kernel's on the same inputs (the project's rule for a replacement
    kernel), never above 2e-5 (test_conv_winograd_f4's cap); and at least one bit differs from the UPS kernel's output, i.e.
    the new kernel ran."""
    name = case[0]
    x0, w, bias, x1, coef, act, res = make(*case)
    want = ref_conv(x0, w, bias, x1, 1, 1, coef, act, res)
    new = run_conv(x0, w, bias, x1, coef, act, res, force=SP)
    old = run_conv(x0, w, bias, x1, coef, act, res, force=F4)
    assert new.shape == want.shape
    e_new, e_old = (new - want).abs().max().item(), (old - want).abs().max().item()
    print('%s: sub-pixel err %.2e, UPS kernel err %.2e' % (name, e_new, e_old))
    assert e_new <= 1.5 * e_old and e_new < 2e-5, (name, e_new, e_old)
    assert not torch.equal(new, old), 'the sub-pixel kernel did not run (identical to the UPS kernel)'


def test_subpixel_does_not_take_4x4_images():
    """Sixteen one-tile low-res images per block did not ship: bit 8 (value 256) is an error there, never a silent fall-back."""
    x0, w, bias, x1, coef, act, res = make('sp_4to8', 19, 32, 0, 4, 4, 128, False, False)
    with pytest.raises(_lib.DlpmError, match='sub-pixel'):
        run_conv(x0, w, bias, force=SP)
    old = run_conv(x0, w, bias, force=F4)
    assert (old - ref_conv(x0, w, bias, None, 1, 1)).abs().max().item() < 2e-5


def test_subpixel_batch_independence():
    """Image k convolved alone is bit-identical to image k inside the batch (four images per block, ragged last block)."""
    x0, w, bias, x1, coef, act, res = make(*CASES[1])
    full = run_conv(x0, w, bias)
    for k in (1, 4):
        one = run_conv(x0[k:k + 1], w, bias)
        assert torch.equal(one[0], full[k]), k


@pytest.mark.parametrize('shape', [(2, 16, 16, 16), (5, 32, 8, 8), (1, 16, 32, 16), (1, 16, 16, 32)],
                         ids=['block_class', 'image_class', 'two_block_rows', 'two_block_columns'])
def test_subpixel_statistics_partials(shape):
    """Every (mean, M2) partial against the mean and centred sum of squares of ITS OWN pixels of the kernel's output, which pins
    the slot order stated in conv.h: [image][block of 16x16 low-res pixels, row-major][class 2 a + b] of 256 outputs, or -- four
    whole 8x8 low-res images per block -- [image][class] of 64; class (a, b) = output pixels (2 i + a, 2 j + b).  Then the
    partials merged in index order as k_gn_coeffs_stats merges partials of equal count (gn_stats.h) against the whole image.
    Tolerances of the fused blocks' statistics tests in test_gpu_kernels.py."""
    B, Cin, Hlo, Wlo = shape
    x0, w, bias, x1, coef, act, res = make('sp_stats', B, Cin, 0, Hlo, Wlo, 128, True, True)
    out, part, px = run_conv(x0, w, bias, None, coef, act, res, stats=True)
    nt = part.shape[1]
    assert px == (256 if Hlo * Wlo >= 256 else 64) and nt * px == 4 * Hlo * Wlo and bool(torch.isfinite(part).all())
    p, o = part.double(), out.double()

    def check(got, sub):
        want_m = sub.mean(dim=(2, 3))
        want_M2 = ((sub - want_m[:, :, None, None]) ** 2).sum(dim=(2, 3))
        assert (got[0] - want_m).abs().max() < 1e-5
        assert ((got[1] - want_M2).abs() / (1 + want_M2)).max() < 1e-5
    bs = 32 if px == 256 else 2 * Hlo          # output pixels per block side (px = 64: the whole image)
    k = 0
    for by in range(2 * Hlo // bs):
        for bx in range(2 * Wlo // bs):
            blk = o[:, :, by * bs:(by + 1) * bs, bx * bs:(bx + 1) * bs]
            for a in (0, 1):
                for b in (0, 1):
                    check((p[:, k, :, 0], p[:, k, :, 1]), blk[:, :, a::2, b::2])
                    k += 1
    assert k == nt
    m, M2, na = p[:, 0, :, 0].clone(), p[:, 0, :, 1].clone(), float(px)
    for k in range(1, nt):
        d, N = p[:, k, :, 0] - m, na + px
        m += d * (px / N)
        M2 += p[:, k, :, 1] + d * d * (na * px / N)
        na = N
    check((m, M2), o)


def test_subpixel_through_the_net():
    """A small UNet whose Upsample convolution (256 -> 256, 8x8 -> 16x16) takes the sub-pixel kernel, against the oracle; the
    launch reports under its own profile class."""
    import dlpm_amd
    torch.manual_seed(31)
    net = dlpm_amd.UNetModel(3, 128, 3, 1, [2], channel_mult=[1, 2], num_heads=4, use_scale_shift_norm=True)
    dlpm_amd.rerandomize_(net, 32)
    g = torch.Generator().manual_seed(33)
    x, t = torch.randn(3, 3, 16, 16, generator=g), torch.rand(3, generator=g)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    with torch.no_grad():
        want = nets.unet_forward(sd, x, t, 4)
    got = net(x.to(DEV), t.to(DEV)).cpu()
    _lib.check(L().dlpm_prof_enable(1))
    try:
        again = net(x.to(DEV), t.to(DEV)).cpu()
        buf = C.create_string_buffer(1 << 16)
        _lib.check(L().dlpm_prof_report(buf, len(buf)))
    finally:
        _lib.check(L().dlpm_prof_enable(0))
    err = (got - want).abs().max().item()
    print('UNet mc=128 [1,2] 16x16 B=3: max |hip - oracle| = %.3g (|y| max %.3g)' % (err, want.abs().max().item()))
    assert err < 1e-5
    assert torch.equal(again, got)
    classes = [ln.split()[0].split(':')[0] for ln in buf.value.decode().strip().splitlines()]
    assert 'conv3x3_wino4sp' in classes, classes


_NET_DIGEST_SCRIPT = r"""
import hashlib, sys, torch
sys.path.insert(0, sys.argv[1])
import dlpm_amd
p = dlpm_amd.load_config('cifar10')
torch.manual_seed(1234)
net = dlpm_amd.rerandomize_(dlpm_amd.init_model_by_parameter(p), 4321).to('cuda')
g = torch.Generator().manual_seed(5)
x = torch.randn(5, 3, 32, 32, generator=g).cuda()
t = torch.rand(5, generator=g).cuda()
print(hashlib.sha256(net(x, t).cpu().numpy().tobytes()).hexdigest())
"""


def test_switch_off_is_the_parent_commits_forward_bit_for_bit():
    """DLPM_WINO4_SUBPIX=0 (read once per process: one child each) puts the Upsample convolutions back on the UPS kernel: the
    CIFAR net's forward (B = 5) then has the digest recorded from the commit before this kernel existed
    (tests/golden/upsample_subpixel_parent_digest.txt: this child script run against that commit's library on MI355X); with
    the switch on (default) the Upsample layers that take the new kernel round differently.
    The digest pins the whole forward, so a later change that deliberately rounds ANY of its kernels differently has to
    re-record it: `DLPM_WINO4_SUBPIX=0 python tests/test_gpu_upsample_subpixel.py` on MI355X rewrites the file -- from a tree
    in which the switch-off path itself is untouched, which is what the digest stands for from then on."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'tests', 'golden', 'upsample_subpixel_parent_digest.txt')) as f:
        parent = f.read().split()[0]
    out = {}
    for sw in ('0', '1'):
        e = dict(os.environ, DLPM_WINO4_SUBPIX=sw)
        r = subprocess.run([sys.executable, '-c', _NET_DIGEST_SCRIPT, root], env=e, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        out[sw] = r.stdout.strip().splitlines()[-1]
    assert len(parent) == 64 and out['0'] == parent, (out, parent)
    assert out['1'] != parent


if __name__ == '__main__':      # re-record the digest (see the test above)
    assert os.environ.get('DLPM_WINO4_SUBPIX') == '0', 'record with DLPM_WINO4_SUBPIX=0'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-c', _NET_DIGEST_SCRIPT, root], capture_output=True, text=True, timeout=900, check=True)
    with open(os.path.join(root, 'tests', 'golden', 'upsample_subpixel_parent_digest.txt'), 'w') as f:
        f.write(r.stdout.strip().splitlines()[-1] + '\n')
