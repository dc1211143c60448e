"""Parity of each HIP kernel, called through the C ABI, against the oracle (CPU) on seeded inputs.

fp32 tolerances are written at each assert.  Marked gpu: runs on the MI355X box only."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from dlpm_amd import _lib
from oracle import nets, process as P

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def L():
    return _lib.lib()


def st():
    return _lib.stream_ptr()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def run_conv(x0, w, bias=None, x1=None, stride=1, ups=0, coef=None, silu=False, res=None, in_nchw=False,
             out_nchw=False, force_direct=False, scratch_extra=0, stats=False):
    """x0/x1: NCHW cpu tensors; returns NCHW cpu output of the HIP conv.  res: the residual, or a pair (res0, res1) = the two halves
    of a residual concat.  stats=True: the launch through dlpm_conv2d_stats_f32; returns (output, the WHOLE statistics buffer --
    2 B (Hout Wout / 64) Cout floats, the upper bound a caller allocates, pre-filled with NaN -- as a flat cpu tensor, pixels per partial)."""
    B, C0, Hin, Win = x0.shape
    Cout, Cin, ks, _ = w.shape
    Hi, Wi = (Hin * 2, Win * 2) if ups else (Hin, Win)
    pad = ks // 2
    Hout, Wout = (Hi + 2 * pad - ks) // stride + 1, (Wi + 2 * pad - ks) // stride + 1
    a = _lib.ConvArgs()
    keep = []

    def dev(t):
        t = t.to(DEV).contiguous()
        keep.append(t)
        return t.data_ptr()
    a.src0 = dev(x0 if in_nchw else nhwc(x0))
    a.C0 = C0
    if x1 is not None:
        a.src1, a.C1 = dev(nhwc(x1)), x1.shape[1]
    a.B, a.Hin, a.Win, a.Hout, a.Wout = B, Hin, Win, Hout, Wout
    a.ksize, a.stride, a.upsample = ks, stride, ups
    a.weight = dev(w)
    if bias is not None:
        a.bias = dev(bias)
    if coef is not None:
        a.coefA, a.coefB = dev(coef[0]), dev(coef[1])
    a.act_silu = int(silu)
    if isinstance(res, tuple):
        a.res0, a.res1, a.R0 = dev(nhwc(res[0])), dev(nhwc(res[1])), res[0].shape[1]
    elif res is not None:
        a.res0, a.R0 = dev(nhwc(res)), Cout
    out = torch.empty((B, Cout, Hout, Wout) if out_nchw else (B, Hout, Wout, Cout), device=DEV)
    a.out, a.Cout = out.data_ptr(), Cout
    a.in_nchw, a.out_nchw, a.force_direct = int(in_nchw), int(out_nchw), int(force_direct)
    scratch = torch.empty(9 * w.numel() + 16 * 1024 * (1 + Cout // 32) + scratch_extra, device=DEV)
    a.scratch_floats = scratch.numel()
    if stats:
        part = torch.full((2 * B * max(1, Hout * Wout // 64) * Cout,), float('nan'), device=DEV)
        px = C.c_int32(0)
        _lib.check(L().dlpm_conv2d_stats_f32(C.byref(a), scratch.data_ptr(), part.data_ptr(), C.byref(px), st()))
        torch.cuda.synchronize()
        return (out if out_nchw else nchw(out)).cpu(), part.cpu(), px.value
    _lib.check(L().dlpm_conv2d_f32(C.byref(a), scratch.data_ptr(), st()))
    torch.cuda.synchronize()
    return (out if out_nchw else nchw(out)).cpu()


def ref_conv(x0, w, bias=None, x1=None, stride=1, ups=0, coef=None, silu=False, res=None):
    x = x0 if x1 is None else torch.cat([x0, x1], 1)
    if coef is not None:
        x = x * coef[0][:, :, None, None] + coef[1][:, :, None, None]
    if silu:
        x = nets.silu(x)
    if ups:
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    y = F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), stride=stride, padding=w.shape[2] // 2)
    if res is not None:
        y = y + res.double()
    return y.float()


def conv_tol(w, Cin):
    # fp32 accumulation over K = taps*Cin terms of O(1) magnitude: error ~ sqrt(K) * 1e-7 * |terms|
    return 3e-6 * math.sqrt(w.shape[2] * w.shape[3] * Cin)


CONV_CASES = [
    # name, B, C0, C1, H, Cout, ks, stride, ups, coef, silu, res
    ('igemm_3x3_128', 2, 128, 0, 8, 128, 3, 1, 0, False, False, False),
    ('igemm_3x3_fused_gn_silu_res', 3, 64, 0, 8, 64, 3, 1, 0, True, True, True),
    ('igemm_3x3_concat', 2, 64, 32, 8, 64, 3, 1, 0, True, True, False),
    ('igemm_1x1_concat_skip', 2, 64, 32, 4, 32, 1, 1, 0, False, False, False),
    ('igemm_3x3_stride2', 2, 32, 0, 16, 32, 3, 2, 0, False, False, False),
    ('igemm_3x3_upsample', 2, 64, 0, 4, 64, 3, 1, 1, False, False, False),
    ('igemm_cout_256_tail', 1, 128, 0, 4, 256, 3, 1, 0, False, False, True),
    ('igemm_cout_96', 2, 32, 0, 8, 96, 1, 1, 0, True, False, False),
    ('igemm_1x1_qkv_16x16', 3, 64, 0, 16, 192, 1, 1, 0, True, False, False),
    ('igemm_1x1_proj_res_4x4', 5, 64, 0, 4, 64, 1, 1, 0, False, False, True),
    ('igemm_1x1_skip_concat_32x32', 1, 64, 64, 32, 128, 1, 1, 0, False, False, False),
    ('igemm_linear_silu', 37, 128, 0, 1, 96, 1, 1, 0, False, True, False),
    ('igemm_ragged_m', 3, 32, 0, 4, 32, 3, 1, 0, False, True, False),     # M = 48 < one 128-pixel tile
    ('igemm_32x32_rows', 1, 32, 0, 32, 64, 3, 1, 0, True, True, True),
    ('igemm_halo_32x32_concat_res', 2, 64, 32, 32, 128, 3, 1, 0, True, True, True),
    ('igemm_halo_16x16', 3, 64, 0, 16, 64, 3, 1, 0, True, True, False),
    ('igemm_halo_16x16_noact_cout32', 2, 32, 0, 16, 32, 3, 1, 0, False, False, True),
    ('igemm_halo_64x64', 1, 32, 0, 64, 32, 3, 1, 0, True, True, False),
    ('igemm_halo_upsample_16to32', 2, 64, 0, 16, 128, 3, 1, 1, False, False, False),
    ('igemm_halo_upsample_4to8_multiimage', 3, 32, 0, 4, 64, 3, 1, 1, False, False, True),
    ('igemm_halo_upsample_8to16_coef', 2, 32, 0, 8, 32, 3, 1, 1, True, True, False),
    ('direct_odd_channels', 2, 24, 0, 8, 40, 3, 1, 0, True, True, True),
    ('direct_concat_1x1', 2, 8, 16, 4, 8, 1, 1, 0, False, False, False),
    ('direct_stride2', 2, 8, 0, 8, 8, 3, 2, 0, False, False, False),
    ('direct_upsample', 2, 8, 0, 4, 8, 3, 1, 1, False, False, False),
]


@pytest.mark.parametrize('case', CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv(case):
    name, B, C0, C1, H, Cout, ks, stride, ups, use_coef, silu, use_res = case
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    Cin = C0 + C1
    x0 = torch.randn(B, C0, H, H, generator=g)
    x1 = torch.randn(B, C1, H, H, generator=g) if C1 else None
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / math.sqrt(Cin * ks * ks)
    bias = torch.randn(Cout, generator=g)
    coef = (1 + 0.3 * torch.randn(B, Cin, generator=g), 0.3 * torch.randn(B, Cin, generator=g)) if use_coef else None
    Ho = (H * (2 if ups else 1) + 2 * (ks // 2) - ks) // stride + 1
    res = torch.randn(B, Cout, Ho, Ho, generator=g) if use_res else None
    want = ref_conv(x0, w, bias, x1, stride, ups, coef, silu, res)
    got = run_conv(x0, w, bias, x1, stride, ups, coef, silu, res)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() < conv_tol(w, Cin), name
    if 'igemm' in name and ks == 3 and stride == 1:
        # force_direct bit 1: no Winograd -- the same shape through the implicit-GEMM halo kernel (where the shape
        # qualified for F(2x2,3x3) the run above took the Winograd kernel)
        got_h = run_conv(x0, w, bias, x1, stride, ups, coef, silu, res, force_direct=2)
        assert (got_h - want).abs().max().item() < conv_tol(w, Cin), name + ' (implicit GEMM)'
        print('%s: winograd/auto err %.2e, implicit-GEMM err %.2e, tol %.2e' % (
            name, (got - want).abs().max().item(), (got_h - want).abs().max().item(), conv_tol(w, Cin)))
    if 'igemm' in name and ks == 1:
        # force_direct bit 2 asked for the weight-streaming 1x1 kernel, which was measured slower and removed: an error, not a fall-back
        with pytest.raises(_lib.DlpmError, match=r'dlpm status -3\]'):   # DLPM_ERR_UNSUPPORTED
            run_conv(x0, w, bias, x1, stride, ups, coef, silu, res, force_direct=4)
    if 'igemm' in name:  # same shape through the direct kernel: the two kernels agree with each other
        got_d = run_conv(x0, w, bias, x1, stride, ups, coef, silu, res, force_direct=True)
        assert (got_d - want).abs().max().item() < conv_tol(w, Cin), name + ' (direct)'


WINO4_CASES = [
    # name, B, C0, C1, H (input), Cout, ups, coef+silu, res   -- F(4x4,3x3) kernel (force_direct bit 3)
    ('f4_16x16_block', 2, 128, 0, 16, 128, 0, False, False),
    ('f4_32x32_four_blocks_gn_silu_res', 2, 64, 0, 32, 128, 0, True, True),
    ('f4_concat_cout256', 1, 64, 32, 16, 256, 0, True, False),
    ('f4_8x8_four_images', 5, 32, 0, 8, 128, 0, True, True),          # B not a multiple of the 4 images per block
    ('f4_4x4_sixteen_images', 19, 32, 32, 4, 128, 0, False, True),
    ('f4_upsample_8to16', 2, 32, 0, 8, 128, 1, False, False),
    ('f4_upsample_16to32_coef_res', 1, 64, 0, 16, 128, 1, True, True),
    ('f4_upsample_2to4_multiimage', 18, 32, 0, 2, 128, 1, False, False),
    ('f4_64x64', 1, 32, 0, 64, 128, 0, True, False),
    ('f4_long_k', 1, 256, 256, 8, 128, 0, True, True),
]


# max |F(4x4) kernel - fp64 reference| measured on MI355X.  Round 4 (interpolation points {0, +-11/16, +-3/2, inf}, profiles/r04/
# kernels_f4_points.txt); with rounds 1-3's {0, +-1, +-2, inf} the same cases measured 1.0-4.5e-5 (F4_MEASURED_LAVIN_POINTS, kept
# for the record: the F4_POINTS_LAVIN build reproduces them bit for bit).
F4_MEASURED = {'f4_16x16_block': 9.30e-06,
               'f4_32x32_four_blocks_gn_silu_res': 3.99e-06,
               'f4_concat_cout256': 4.23e-06,
               'f4_8x8_four_images': 3.10e-06,
               'f4_4x4_sixteen_images': 5.74e-06,
               'f4_upsample_8to16': 5.28e-06,
               'f4_upsample_16to32_coef_res': 5.96e-06,
               'f4_upsample_2to4_multiimage': 4.14e-06,
               'f4_64x64': 3.34e-06,
               'f4_long_k': 8.94e-06}
F4_MEASURED_LAVIN_POINTS = {'f4_16x16_block': 4.49e-05, 'f4_32x32_four_blocks_gn_silu_res': 1.57e-05, 'f4_concat_cout256': 1.7e-05,
                            'f4_8x8_four_images': 9.95e-06, 'f4_4x4_sixteen_images': 2.72e-05, 'f4_upsample_8to16': 3.65e-05,
                            'f4_upsample_16to32_coef_res': 2.12e-05, 'f4_upsample_2to4_multiimage': 2e-05, 'f4_64x64': 1.7e-05,
                            'f4_long_k': 2.42e-05}


@pytest.mark.parametrize('case', WINO4_CASES, ids=[c[0] for c in WINO4_CASES])
def test_conv_winograd_f4(case):
    """F(4x4,3x3): same convolution, products accumulated in the Winograd domain (partial sums larger than the result).  Bound =
    twice the error measured on MI355X for each case (F4_MEASURED, O(1) outputs: 3-9e-6 with the round-4 interpolation points),
    never above 2e-5 -- a fifth of the path's 1e-4 budget."""
    name, B, C0, C1, H, Cout, ups, act, use_res = case
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    Cin = C0 + C1
    x0 = torch.randn(B, C0, H, H, generator=g)
    x1 = torch.randn(B, C1, H, H, generator=g) if C1 else None
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    bias = torch.randn(Cout, generator=g)
    coef = (1 + 0.3 * torch.randn(B, Cin, generator=g), 0.3 * torch.randn(B, Cin, generator=g)) if act else None
    Ho = H * (2 if ups else 1)
    res = torch.randn(B, Cout, Ho, Ho, generator=g) if use_res else None
    want = ref_conv(x0, w, bias, x1, 1, ups, coef, act, res)
    got = run_conv(x0, w, bias, x1, 1, ups, coef, act, res, force_direct=8)
    got2 = run_conv(x0, w, bias, x1, 1, ups, coef, act, res)
    assert got.shape == want.shape
    e4, e2 = (got - want).abs().max().item(), (got2 - want).abs().max().item()
    tol = min(2e-5, 2 * F4_MEASURED[name])
    print('%s: F(4x4) err %.2e, default path err %.2e, tol %.2e' % (name, e4, e2, tol))
    assert e4 < tol, name
    assert not torch.equal(got, got2), 'the F(4x4) kernel did not run (identical to the default path)'


# Round 5: the same kernel with 4 / 2 waves per workgroup for 64- / 32-channel n-tiles (Cout a multiple of 32 but not of 128: the
# MNIST-sized nets' 32x32 and 16x16 levels).  Same arithmetic per output as the 8-wave shape; measured on MI355X
# (profiles/r05/kernels_f4_narrow.txt), bound = twice the measurement like F4_MEASURED.
WINO4_NARROW_CASES = [
    # name, B, C0, C1, H (input), Cout, ups, coef+silu, res
    ('f4n_c64_16x16_gn_silu_res', 3, 64, 0, 16, 64, 0, True, True),
    ('f4n_c64_concat_16x16', 2, 64, 64, 16, 64, 0, True, False),
    ('f4n_c64_8x8_four_images', 5, 64, 0, 8, 64, 0, True, True),
    ('f4n_c64_upsample_8to16', 2, 64, 0, 8, 64, 1, False, False),
    ('f4n_c64_upsample_16to32', 1, 64, 0, 16, 64, 1, False, False),
    ('f4n_c32_32x32_gn_silu_res', 2, 32, 0, 32, 32, 0, True, True),
    ('f4n_c32_concat96_32x32', 1, 64, 32, 32, 32, 0, True, False),
    ('f4n_c32_16x16', 3, 32, 0, 16, 32, 0, False, False),
    ('f4n_c32_8x8_four_images', 6, 32, 0, 8, 32, 0, True, True),
    ('f4n_c96_16x16_three_ntiles', 2, 32, 0, 16, 96, 0, True, True),
    ('f4n_c192_16x16_three_ntiles', 1, 64, 0, 16, 192, 0, False, True),
]
F4N_MEASURED = {'f4n_c64_16x16_gn_silu_res': 4.17e-06,
                'f4n_c64_concat_16x16': 5.02e-06,
                'f4n_c64_8x8_four_images': 3.58e-06,
                'f4n_c64_upsample_8to16': 6.44e-06,
                'f4n_c64_upsample_16to32': 8.76e-06,
                'f4n_c32_32x32_gn_silu_res': 2.98e-06,
                'f4n_c32_concat96_32x32': 4.83e-06,
                'f4n_c32_16x16': 4.77e-06,
                'f4n_c32_8x8_four_images': 2.74e-06,
                'f4n_c96_16x16_three_ntiles': 3.22e-06,
                'f4n_c192_16x16_three_ntiles': 6.20e-06}


@pytest.mark.parametrize('case', WINO4_NARROW_CASES, ids=[c[0] for c in WINO4_NARROW_CASES])
def test_conv_winograd_f4_narrow(case):
    """F(4x4,3x3) on 64- / 32-channel n-tiles (4 / 2 waves per workgroup) against the fp64 convolution."""
    name, B, C0, C1, H, Cout, ups, act, use_res = case
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    Cin = C0 + C1
    x0 = torch.randn(B, C0, H, H, generator=g)
    x1 = torch.randn(B, C1, H, H, generator=g) if C1 else None
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    bias = torch.randn(Cout, generator=g)
    coef = (1 + 0.3 * torch.randn(B, Cin, generator=g), 0.3 * torch.randn(B, Cin, generator=g)) if act else None
    Ho = H * (2 if ups else 1)
    res = torch.randn(B, Cout, Ho, Ho, generator=g) if use_res else None
    want = ref_conv(x0, w, bias, x1, 1, ups, coef, act, res)
    got = run_conv(x0, w, bias, x1, 1, ups, coef, act, res, force_direct=8)
    got2 = run_conv(x0, w, bias, x1, 1, ups, coef, act, res)
    assert got.shape == want.shape
    e4, e2 = (got - want).abs().max().item(), (got2 - want).abs().max().item()
    tol = min(2e-5, 2 * F4N_MEASURED[name])
    print('%s: F(4x4) narrow err %.2e, default path err %.2e, tol %.2e' % (name, e4, e2, tol))
    assert e4 < tol, name
    assert not torch.equal(got, got2), 'the F(4x4) kernel did not run (identical to the default path)'


def test_conv_winograd_f4_narrow_batch_independence():
    """The MNIST config's own launch shape (B = 256, 32x32, 32 -> 32 channels, GN + SiLU, residual): every image of the batch is
    bit-identical to the same image convolved alone (blocks never span images at 32x32), and matches fp64."""
    B, Cc, H = 256, 32, 32
    g = torch.Generator(device=DEV).manual_seed(12)
    x = torch.randn(B, H, H, Cc, device=DEV, generator=g)
    w = torch.randn(Cc, Cc, 3, 3, device=DEV, generator=g) / math.sqrt(Cc * 9)
    bias = torch.randn(Cc, device=DEV, generator=g)
    cA = 1 + 0.3 * torch.randn(B, Cc, device=DEV, generator=g)
    cB = 0.3 * torch.randn(B, Cc, device=DEV, generator=g)
    res = torch.randn(B, H, H, Cc, device=DEV, generator=g)
    scratch = torch.empty(9 * w.numel() + 16 * 1024 * (1 + Cc // 32), device=DEV)

    def conv(sl):
        n = sl.stop - sl.start
        out = torch.empty(n, H, H, Cc, device=DEV)
        a = _lib.ConvArgs()
        xs, As, Bs, rs = x[sl].contiguous(), cA[sl].contiguous(), cB[sl].contiguous(), res[sl].contiguous()
        a.src0, a.C0, a.B, a.Hin, a.Win, a.Hout, a.Wout = xs.data_ptr(), Cc, n, H, H, H, H
        a.ksize, a.stride, a.weight, a.bias = 3, 1, w.data_ptr(), bias.data_ptr()
        a.coefA, a.coefB, a.act_silu = As.data_ptr(), Bs.data_ptr(), 1
        a.res0, a.R0, a.out, a.Cout = rs.data_ptr(), Cc, out.data_ptr(), Cc
        a.force_direct, a.scratch_floats = 8, scratch.numel()
        _lib.check(L().dlpm_conv2d_f32(C.byref(a), scratch.data_ptr(), st()))
        torch.cuda.synchronize()
        return out

    full = conv(slice(0, B))
    assert torch.isfinite(full).all()
    for b in (0, 129, 255):
        one = conv(slice(b, b + 1))
        assert torch.equal(one[0], full[b]), 'image %d depends on its batch' % b
        xb = nchw(x[b:b + 1]).cpu()
        want = ref_conv(xb, w.cpu(), bias.cpu(), coef=(cA[b:b + 1].cpu(), cB[b:b + 1].cpu()), silu=True, res=nchw(res[b:b + 1]).cpu())
        assert (nchw(full[b:b + 1]).cpu() - want).abs().max().item() < 2e-5


def test_conv_winograd_f4_full_size_batch_independence():
    """BASELINE size (CIFAR step: B = 1024, 32x32, 128 -> 128 channels, GN+SiLU, residual) through a size-independent
    property: the F(4x4) kernel's blocks never span images here, so every image of the big batch must come out
    bit-identical to the same image convolved alone, and the result must match the fp64 reference on those images."""
    B, Cc, H = 1024, 128, 32
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(B, H, H, Cc, device=DEV, generator=g)                      # NHWC
    w = torch.randn(Cc, Cc, 3, 3, device=DEV, generator=g) / math.sqrt(Cc * 9)
    bias = torch.randn(Cc, device=DEV, generator=g)
    cA = 1 + 0.3 * torch.randn(B, Cc, device=DEV, generator=g)
    cB = 0.3 * torch.randn(B, Cc, device=DEV, generator=g)
    res = torch.randn(B, H, H, Cc, device=DEV, generator=g)
    scratch = torch.empty(9 * w.numel() + 16 * 1024 * (1 + Cc // 32), device=DEV)

    def conv(sl):
        n = sl.stop - sl.start
        out = torch.empty(n, H, H, Cc, device=DEV)
        a = _lib.ConvArgs()
        xs, As, Bs, rs = x[sl].contiguous(), cA[sl].contiguous(), cB[sl].contiguous(), res[sl].contiguous()
        a.src0, a.C0, a.B, a.Hin, a.Win, a.Hout, a.Wout = xs.data_ptr(), Cc, n, H, H, H, H
        a.ksize, a.stride, a.weight, a.bias = 3, 1, w.data_ptr(), bias.data_ptr()
        a.coefA, a.coefB, a.act_silu = As.data_ptr(), Bs.data_ptr(), 1
        a.res0, a.R0, a.out, a.Cout = rs.data_ptr(), Cc, out.data_ptr(), Cc
        a.force_direct, a.scratch_floats = 8, scratch.numel()
        _lib.check(L().dlpm_conv2d_f32(C.byref(a), scratch.data_ptr(), st()))
        torch.cuda.synchronize()
        return out

    full = conv(slice(0, B))
    assert torch.isfinite(full).all()
    for b in (0, 517, 1023):
        one = conv(slice(b, b + 1))
        assert torch.equal(one[0], full[b]), 'image %d depends on its batch' % b
        xb = nchw(x[b:b + 1]).cpu()
        want = ref_conv(xb, w.cpu(), bias.cpu(), coef=(cA[b:b + 1].cpu(), cB[b:b + 1].cpu()), silu=True, res=nchw(res[b:b + 1]).cpu())
        assert (nchw(full[b:b + 1]).cpu() - want).abs().max().item() < 1e-4   # measured ~2e-5 (f4_32x32 case)


@pytest.mark.parametrize('H', [8, 4])
def test_conv_winograd_f2_small_launch_shape_is_bit_identical(H):
    """64-channel F(2x2) layers on 8x8 / 4x4 tensors: small batches take the 4-wave 32-tile x 64-channel workgroup shape,
    large ones the 8-wave 64-tile shape (wino_small_launch).  Same arithmetic per output: the first images of a large
    batch must equal, bit for bit, the same images convolved as a small batch -- and match the fp64 reference."""
    Cc, Bbig, Bsmall = 64, 2048, 6
    g = torch.Generator(device=DEV).manual_seed(H)
    x = torch.randn(Bbig, H, H, Cc, device=DEV, generator=g)
    w = torch.randn(Cc, Cc, 3, 3, device=DEV, generator=g) / math.sqrt(Cc * 9)
    bias = torch.randn(Cc, device=DEV, generator=g)
    cA = 1 + 0.3 * torch.randn(Bbig, Cc, device=DEV, generator=g)
    cB = 0.3 * torch.randn(Bbig, Cc, device=DEV, generator=g)
    res = torch.randn(Bbig, H, H, Cc, device=DEV, generator=g)
    scratch = torch.empty(90 * w.numel() + 64 * 1024 * (1 + Cc // 32), device=DEV)

    def conv(n):
        out = torch.empty(n, H, H, Cc, device=DEV)
        a = _lib.ConvArgs()
        xs, As, Bs, rs = x[:n].contiguous(), cA[:n].contiguous(), cB[:n].contiguous(), res[:n].contiguous()
        a.src0, a.C0, a.B, a.Hin, a.Win, a.Hout, a.Wout = xs.data_ptr(), Cc, n, H, H, H, H
        a.ksize, a.stride, a.weight, a.bias = 3, 1, w.data_ptr(), bias.data_ptr()
        a.coefA, a.coefB, a.act_silu = As.data_ptr(), Bs.data_ptr(), 1
        a.res0, a.R0, a.out, a.Cout = rs.data_ptr(), Cc, out.data_ptr(), Cc
        a.force_direct, a.scratch_floats = 0, scratch.numel()
        _lib.check(L().dlpm_conv2d_f32(C.byref(a), scratch.data_ptr(), st()))
        torch.cuda.synchronize()
        return out
    big, small = conv(Bbig), conv(Bsmall)
    assert torch.equal(small, big[:Bsmall])
    want = ref_conv(nchw(x[:Bsmall]).cpu(), w.cpu(), bias.cpu(), coef=(cA[:Bsmall].cpu(), cB[:Bsmall].cpu()), silu=True,
                    res=nchw(res[:Bsmall]).cpu())
    assert (nchw(small).cpu() - want).abs().max().item() < conv_tol(w, Cc)


def test_conv_boundary_layouts():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 8, 8, generator=g)
    w = torch.randn(32, 3, 3, 3, generator=g) / 5
    b = torch.randn(32, generator=g)
    got = run_conv(x, w, b, in_nchw=True)          # stem: reads the caller's NCHW state
    assert (got - ref_conv(x, w, b)).abs().max().item() < 1e-5
    h = torch.randn(2, 32, 8, 8, generator=g)
    w2 = torch.randn(3, 32, 3, 3, generator=g) / 17
    b2 = torch.randn(3, generator=g)
    coef = (1 + 0.3 * torch.randn(2, 32, generator=g), 0.3 * torch.randn(2, 32, generator=g))
    got = run_conv(h, w2, b2, coef=coef, silu=True, out_nchw=True)   # head: writes NCHW eps (MFMA kernel, 32-wide N tile)
    assert (got - ref_conv(h, w2, b2, coef=coef, silu=True)).abs().max().item() < 2e-5
    got = run_conv(h, w2, b2, coef=coef, silu=True, out_nchw=True, force_direct=True)
    assert (got - ref_conv(h, w2, b2, coef=coef, silu=True)).abs().max().item() < 2e-5
    got = run_conv(x, w, b, in_nchw=True, force_direct=True)
    assert (got - ref_conv(x, w, b)).abs().max().item() < 1e-5


@pytest.mark.parametrize('B,Cin,H,Cout', [(3, 3, 32, 128), (2, 1, 32, 32), (1, 3, 64, 128), (2, 3, 16, 64)])
def test_stem_conv_kernels(B, Cin, H, Cout):
    """The stem (unet.py:347: reads the caller's NCHW state, Cin = image channels): whole rows of one image per block through
    LDS where the image is a multiple of 1024 pixels (CIFAR / MNIST / CelebA shapes), the register-weight kernel otherwise."""
    g = torch.Generator().manual_seed(B * 10 + Cin + H)
    x = torch.randn(B, Cin, H, H, generator=g) * 2
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    b = torch.randn(Cout, generator=g)
    got = run_conv(x, w, b, in_nchw=True)
    assert (got - ref_conv(x, w, b)).abs().max().item() < 1e-5


@pytest.mark.parametrize('B,C,H,Cout,nchw', [(3, 64, 16, 3, True), (2, 32, 32, 3, True), (2, 128, 32, 1, True), (1, 32, 64, 4, False)])
def test_head_conv_kernel(B, C, H, Cout, nchw):
    """The dedicated head kernel (Cout <= 4, fused GN affine + SiLU, NCHW out) against the fp64 reference and against
    the MFMA path it replaces (force_direct bit 1 keeps the launch on the old path)."""
    g = torch.Generator().manual_seed(B * 100 + C + H)
    h = torch.randn(B, C, H, H, generator=g)
    w = torch.randn(Cout, C, 3, 3, generator=g) / math.sqrt(9 * C)
    b = torch.randn(Cout, generator=g)
    coef = (1 + 0.3 * torch.randn(B, C, generator=g), 0.3 * torch.randn(B, C, generator=g))
    want = ref_conv(h, w, b, coef=coef, silu=True)
    # (room for the fragment copy in front of the head copy: without it the entry leaves the head copy out -- at C = 128, Cout = 1 -- and the
    # launch runs the halo kernel a second time; tests/test_gpu_conv_tiles.py asserts the kernel taken)
    room = (C // 32 * 144 + 2) * 256 + 36 * C
    got = run_conv(h, w, b, coef=coef, silu=True, out_nchw=nchw, scratch_extra=room)
    old = run_conv(h, w, b, coef=coef, silu=True, out_nchw=nchw, force_direct=2)
    assert (got - want).abs().max().item() < conv_tol(w, C)
    assert (old - want).abs().max().item() < conv_tol(w, C)
    got2 = run_conv(h, w, b, out_nchw=nchw, scratch_extra=room)                     # no activation
    assert (got2 - ref_conv(h, w, b)).abs().max().item() < conv_tol(w, C)


@pytest.mark.parametrize('B,C,H,Cout,nchw', [(3, 64, 16, 3, True), (2, 32, 32, 3, True), (2, 128, 32, 1, True), (1, 32, 64, 2, False),
                                             (5, 128, 32, 3, True), (2, 128, 64, 3, True)])   # last: the CelebA-64 head (TH = 2 gather tiles)
def test_head_conv_as_gemm_plus_gather(B, C, H, Cout, nchw):
    """The head (unet.py:435) as a 1x1 GEMM onto its 9 Cout tap channels (fused GN affine + SiLU) + the 9-point gather
    (force_direct bit 32), against the fp64 reference and next to the dedicated VALU kernel it replaces in the UNet plan."""
    g = torch.Generator().manual_seed(B * 100 + C + H + 7)
    h = torch.randn(B, C, H, H, generator=g)
    w = torch.randn(Cout, C, 3, 3, generator=g) / math.sqrt(9 * C)
    b = torch.randn(Cout, generator=g)
    coef = (1 + 0.3 * torch.randn(B, C, generator=g), 0.3 * torch.randn(B, C, generator=g))
    extra = 32 * C + B * H * H * 32
    want = ref_conv(h, w, b, coef=coef, silu=True)
    got = run_conv(h, w, b, coef=coef, silu=True, out_nchw=nchw, force_direct=32, scratch_extra=extra)
    old = run_conv(h, w, b, coef=coef, silu=True, out_nchw=nchw)
    e_new, e_old = (got - want).abs().max().item(), (old - want).abs().max().item()
    print('head %dx%d C%d -> %d: GEMM + gather err %.2e, VALU kernel err %.2e, tol %.2e' % (H, H, C, Cout, e_new, e_old, conv_tol(w, C)))
    if H % 32 == 0 and C <= 128:
        # round 4: the ONE-PASS head kernel (force_direct bit 64; head_fused.hip): the tap channels never leave the CU.  Its default
        # form runs the GEMM on the bf16 pipe (exact three-plane split, six products); bit 128 keeps it on the fp32 MFMA
        extra = max(extra, 80 * C + 4096)
        one = run_conv(h, w, b, coef=coef, silu=True, out_nchw=nchw, force_direct=64, scratch_extra=extra)
        one32 = run_conv(h, w, b, coef=coef, silu=True, out_nchw=nchw, force_direct=64 | 128, scratch_extra=extra)
        e_one, e_one32 = (one - want).abs().max().item(), (one32 - want).abs().max().item()
        print('    one-pass head kernel err %.2e (bf16 x 3), %.2e (fp32 MFMA)' % (e_one, e_one32))
        assert e_one < conv_tol(w, C) and e_one32 < conv_tol(w, C)
        assert e_one <= 1.5 * e_one32 + 1e-7              # the split is exact to 2^-24 per product: no worse than the fp32 form
        # a launch WITHOUT bias (valid for dlpm_conv2d_f32): the kernel's unconditional dummy load must not leak into the sums
        # (round 4 seeded the accumulators with W'[0] there -- ADVICE r04)
        nb = run_conv(h, w, None, coef=coef, silu=True, out_nchw=nchw, force_direct=64, scratch_extra=extra)
        assert (nb - ref_conv(h, w, None, coef=coef, silu=True)).abs().max().item() < conv_tol(w, C)
    assert e_new < conv_tol(w, C) and e_old < conv_tol(w, C)
    got2 = run_conv(h, w, None, out_nchw=nchw, force_direct=32, scratch_extra=extra)       # no activation, no bias
    assert (got2 - ref_conv(h, w, None)).abs().max().item() < conv_tol(w, C)


@pytest.mark.parametrize('C,Cout,H,f32', [(32, 3, 32, False), (64, 2, 32, False), (96, 1, 32, True), (32, 3, 64, False)])
def test_head_one_pass_walks_many_images(C, Cout, H, f32):
    """The one-pass head kernel is PERSISTENT: two workgroups per CU walk the images (head_fused.hip), carrying the next image's
    GroupNorm coefficients and two tiles of read-ahead across image boundaries.  A batch of more images than workgroups (every
    workgroup walks two or three, the last ones one fewer), per-image coefficients that differ wildly between neighbours, every channel
    count the kernel instantiates (32 / 64 / 96; 128 is the bench's) and both picture widths: every image against the fp64 reference."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * ncu * 2 + 37 if H == 32 else 2 * ncu + 5
    g = torch.Generator().manual_seed(C + Cout + H)
    h = torch.randn(B, C, H, H, generator=g)
    w = torch.randn(Cout, C, 3, 3, generator=g) / math.sqrt(9 * C)
    b = torch.randn(Cout, generator=g)
    coef = ((1 + 0.3 * torch.randn(B, C, generator=g)) * (1 + (torch.arange(B) % 3)[:, None].float()), 0.3 * torch.randn(B, C, generator=g))
    want = ref_conv(h, w, b, coef=coef, silu=True)
    got = run_conv(h, w, b, coef=coef, silu=True, out_nchw=True, force_direct=64 | (128 if f32 else 0), scratch_extra=80 * C + 4096)
    err = (got - want).abs().amax(dim=(1, 2, 3))
    print('one-pass head, %d images of %dx%d, C%d -> %d (%s): max err %.2e (image %d), tol %.2e'
          % (B, H, H, C, Cout, 'fp32 MFMA' if f32 else 'bf16 x 3', err.max().item(), int(err.argmax()), conv_tol(w, C)))
    assert err.max().item() < conv_tol(w, C)              # (observed 1.9e-6 .. 2.9e-6)


def test_linear_as_conv():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(37, 128, generator=g)
    w = torch.randn(512, 128, generator=g) / 11
    b = torch.randn(512, generator=g)
    got = run_conv(x[:, :, None, None], w[:, :, None, None], b, silu=True)
    want = F.linear(nets.silu(x).double(), w.double(), b.double()).float()
    assert (got[:, :, 0, 0] - want).abs().max().item() < 2e-5


@pytest.mark.parametrize('C,hw', [(32, 8), (96, 4), (128, 8), (384, 4)])
def test_groupnorm_coeffs_against_reference_fixture(C, hw):
    f = golden('f7_layers')
    tag = 'gn_C%d_hw%d' % (C, hw)
    x = torch.from_numpy(f[tag + '_x'])
    B = x.shape[0]
    xd = nhwc(x).to(DEV)
    gam, bet = torch.from_numpy(f[tag + '_w']).to(DEV), torch.from_numpy(f[tag + '_b']).to(DEV)
    cA, cB = torch.empty(B, C, device=DEV), torch.empty(B, C, device=DEV)
    _lib.check(L().dlpm_groupnorm_coeffs_f32(xd.data_ptr(), None, C, 0, B, hw * hw, 32, gam.data_ptr(), bet.data_ptr(),
                                            None, 0, 0, cA.data_ptr(), cB.data_ptr(), st()))
    y = x * cA.cpu()[:, :, None, None] + cB.cpu()[:, :, None, None]
    # GroupNorm output is O(1); fp32 statistics over (C/32)*hw*hw elements
    np.testing.assert_allclose(y.numpy(), f[tag + '_y'], atol=3e-6)
    # scale/shift folded in, virtual concat split at a point that cuts a group when C/32 does not divide it
    ss = torch.cat([torch.from_numpy(f[tag + '_sc']).reshape(B, C), torch.from_numpy(f[tag + '_sh']).reshape(B, C)], 1)
    ss_pad = torch.zeros(B, 2 * C + 7)
    ss_pad[:, 5:5 + 2 * C] = ss
    ssd = ss_pad.to(DEV)
    c0 = 64 if C == 96 else (256 if C == 384 else C // 2)
    x0, x1 = nhwc(x[:, :c0]).to(DEV), nhwc(x[:, c0:]).to(DEV)
    _lib.check(L().dlpm_groupnorm_coeffs_f32(x0.data_ptr(), x1.data_ptr(), c0, C - c0, B, hw * hw, 32, gam.data_ptr(),
                                            bet.data_ptr(), ssd.data_ptr(), 2 * C + 7, 5, cA.data_ptr(), cB.data_ptr(), st()))
    y = nets.silu(x * cA.cpu()[:, :, None, None] + cB.cpu()[:, :, None, None])
    np.testing.assert_allclose(y.numpy(), f[tag + '_y_ss_silu'], atol=4e-6)


def test_groupnorm_scalar_kernel_odd_channels():
    """C = 30 (not a multiple of 4) takes the scalar kernel; checked against the oracle."""
    g = torch.Generator().manual_seed(8)
    x = torch.randn(3, 30, 5, 5, generator=g) * 1.5 + 0.3
    gam, bet = 1 + 0.2 * torch.randn(30, generator=g), 0.2 * torch.randn(30, generator=g)
    want = nets.group_norm(x, gam, bet)
    xd, gd, bd = nhwc(x).to(DEV), gam.to(DEV), bet.to(DEV)
    cA, cB = torch.empty(3, 30, device=DEV), torch.empty(3, 30, device=DEV)
    _lib.check(L().dlpm_groupnorm_coeffs_f32(xd.data_ptr(), None, 30, 0, 3, 25, 30, gd.data_ptr(), bd.data_ptr(),
                                            None, 0, 0, cA.data_ptr(), cB.data_ptr(), st()))
    y = x * cA.cpu()[:, :, None, None] + cB.cpu()[:, :, None, None]
    np.testing.assert_allclose(y.numpy(), want.numpy(), atol=3e-6)


@pytest.mark.parametrize('ch,T', [(16, 64), (64, 16), (16, 256), (64, 64)])
def test_attention_against_reference_fixture(ch, T):
    f = golden('f7_layers')
    qkv = torch.from_numpy(f['qkv_ch%d_T%d_in' % (ch, T)])      # [N = b*heads, 3ch, T], b = 1, heads = 3
    heads = qkv.shape[0]
    Cc = heads * ch
    # [heads, 3ch, T] -> NHWC [1, T, heads*3ch] (head-major channels)
    x = qkv.permute(2, 0, 1).reshape(1, T, heads * 3 * ch).contiguous().to(DEV)
    out = torch.empty(1, T, Cc, device=DEV)
    _lib.check(L().dlpm_attention_f32(x.data_ptr(), out.data_ptr(), 1, T, Cc, heads, st()))
    got = out.cpu().reshape(T, heads, ch).permute(1, 2, 0)       # [heads, ch, T]
    np.testing.assert_allclose(got.numpy(), f['qkv_ch%d_T%d_out' % (ch, T)], atol=3e-6)


def test_attention_batched_heads():
    g = torch.Generator().manual_seed(6)
    B, heads, ch, T = 5, 4, 16, 64
    qkv = torch.randn(B * heads, 3 * ch, T, generator=g)
    want = nets.qkv_attention(qkv).reshape(B, heads * ch, T)
    x = qkv.reshape(B, heads * 3 * ch, T).permute(0, 2, 1).contiguous().to(DEV)
    out = torch.empty(B, T, heads * ch, device=DEV)
    _lib.check(L().dlpm_attention_f32(x.data_ptr(), out.data_ptr(), B, T, heads * ch, heads, st()))
    np.testing.assert_allclose(out.cpu().permute(0, 2, 1).numpy(), want.numpy(), atol=3e-6)


def test_timestep_embedding():
    f = golden('f7_layers')
    t = torch.from_numpy(f['temb_t']).to(DEV)
    for dim in (32, 128):
        e = torch.empty(t.numel(), dim, device=DEV)
        _lib.check(L().dlpm_timestep_embedding_f32(t.data_ptr(), e.data_ptr(), t.numel(), dim, st()))
        # arguments up to 17 rad: sin/cos abs error ~ ulp(arg)
        np.testing.assert_allclose(e.cpu().numpy(), f['temb_dim%d' % dim], atol=2e-6)


def test_layout_roundtrip():
    x = torch.randn(3, 5, 4, 6)
    xd = x.to(DEV)
    a, b = torch.empty(3, 4, 6, 5, device=DEV), torch.empty_like(xd)
    _lib.check(L().dlpm_nchw_to_nhwc_f32(xd.data_ptr(), a.data_ptr(), 3, 5, 4, 6, st()))
    _lib.check(L().dlpm_nhwc_to_nchw_f32(a.data_ptr(), b.data_ptr(), 3, 5, 4, 6, st()))
    assert torch.equal(a.cpu(), nhwc(x)) and torch.equal(b.cpu(), x)


# ------------------------------------------------------------------------------ noise / tables / update
def test_coeff_tables_bit_exact():
    f = golden('f3_sigma_tables')
    A, g, s, bs = (torch.from_numpy(f[k]).to(DEV) for k in ['A', 'g', 's', 'bs'])
    T, B = A.shape
    ce, cn, sig = torch.empty_like(A), torch.empty_like(A), torch.empty_like(A)
    _lib.check(L().dlpm_coeff_tables_f32(A.data_ptr(), g.data_ptr(), s.data_ptr(), bs.data_ptr(), T, B, ce.data_ptr(),
                                        cn.data_ptr(), sig.data_ptr(), st()))
    assert np.array_equal(sig.cpu().numpy(), f['Sigmas'])                       # same fp32 op order: bit-exact
    Gam, var = f['Gamma_1_to_T'], f['var_1_to_T']
    assert np.array_equal(ce.cpu().numpy()[1:], (f['bs'][1:, None] * Gam).astype(np.float32))
    want_cn = np.sqrt(var)
    want_cn[0] = 0.0                                                             # t == 1: no noise
    np.testing.assert_allclose(cn.cpu().numpy()[1:], want_cn, rtol=1.2e-7)


def _update(x, eps, z, t, tabs, flags=0, eta=0.0, alpha=1.7, seed=0, offset=0):
    g, bg, bs, ce, cn, A = tabs
    T, B = A.shape
    a = _lib.UpdateArgs()
    xd = x.to(DEV).contiguous()
    ed = eps.to(DEV).contiguous()
    zd = z.to(DEV).contiguous() if z is not None else None
    td = torch.tensor([t], dtype=torch.int32, device=DEV)
    a.x_dev, a.eps_dev, a.z_dev, a.t_dev = xd.data_ptr(), ed.data_ptr(), zd.data_ptr() if zd is not None else None, td.data_ptr()
    a.g_dev, a.bg_dev, a.bs_dev = g.data_ptr(), bg.data_ptr(), bs.data_ptr()
    a.c_eps_dev, a.c_noise_dev, a.A_dev = ce.data_ptr(), cn.data_ptr(), A.data_ptr()
    a.B, a.D, a.T, a.flags, a.dlim_eta, a.alpha = B, x[0].numel(), T, flags, eta, alpha
    a.seed, a.sample_offset = seed, offset
    _lib.check(L().dlpm_update_f32(C.byref(a), st()))
    torch.cuda.synchronize()
    return xd.cpu(), td.cpu().item()


def _tables(f):
    A, g, bg, s, bs = (torch.from_numpy(f[k]).to(DEV) for k in ['A', 'g', 'bg', 's', 'bs'])
    T, B = A.shape
    ce, cn = torch.empty_like(A), torch.empty_like(A)
    _lib.check(L().dlpm_coeff_tables_f32(A.data_ptr(), g.data_ptr(), s.data_ptr(), bs.data_ptr(), T, B, ce.data_ptr(),
                                        cn.data_ptr(), None, st()))
    return g, bg, bs, ce, cn, A


def test_update_against_reference_single_step():
    f = golden('f4_single_step')
    tabs = _tables(f)
    x, eps = torch.from_numpy(f['x']), torch.from_numpy(f['eps'])
    z = torch.randn(x.shape, generator=torch.Generator().manual_seed(1))
    for t in (1, 2, 17, 49):
        mean = torch.from_numpy(f['dlpm_mean_t%d' % t])
        var = torch.from_numpy(f['dlpm_var_t%d' % t]).view(-1, 1, 1, 1)
        want = mean + (0.0 if t == 1 else 1.0) * torch.sqrt(var) * z
        got, _ = _update(x, eps, z, t, tabs)
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=3e-7, atol=1e-6)   # same op order, 1-2 ulp
        got, tn = _update(x, eps, None, t, tabs, flags=_lib.UPD_DLIM | _lib.UPD_ADVANCE)
        assert tn == t - 1
        np.testing.assert_allclose(got.numpy(), f['dlim0_t%d' % t], rtol=3e-7, atol=1e-6)
        z0 = torch.zeros_like(x)
        got, _ = _update(x, eps, z0, t, tabs, flags=_lib.UPD_DLIM, eta=0.5)
        np.testing.assert_allclose(got.numpy(), f['dlim05_mean_t%d' % t], rtol=2e-6, atol=2e-6)
        # clip branch: eps' then the DLPM mean
        e2 = torch.from_numpy(f['eps_from_clipped_xstart_t%d' % t])
        Sig = P.sigma_table(tabs[5].cpu(), tabs[0].cpu(), torch.from_numpy(f['s']))
        want, _, _ = P.dlpm_step(x, e2, t, Sig, tabs[0].cpu(), tabs[2].cpu(), z)
        got, _ = _update(x, eps, z, t, tabs, flags=_lib.UPD_CLIP)
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-6, atol=2e-6)


@pytest.mark.parametrize('shape', [(3, 2, 4, 4), (2, 1, 1, 3)])       # D % 4 == 0 (vector path) and D = 3 (scalar path)
def test_update_elementwise_tables_all_variants(shape):
    """DLPM_UPD_ELEMENTWISE (non-isotropic noise): per-element [T,B,D] tables through the update kernel, every variant
    (stochastic, clip, DLIM eta = 0, DLIM eta > 0 with noise, history row) against the oracle's formulas."""
    T, alpha = 12, 1.7
    g_, bg_, s_, bs_ = P.schedule(T, alpha)
    gen = torch.Generator().manual_seed(sum(shape))
    B, D = shape[0], int(np.prod(shape[1:]))
    A = torch.rand((T,) + shape, generator=gen) * 3 + 0.2
    x, eps, z = (torch.randn(shape, generator=gen) for _ in range(3))
    Sig = P.sigma_table(A, g_, s_)
    Ad = A.reshape(T, B * D).to(DEV).contiguous()
    g, bg, s, bs = (v.to(DEV) for v in (g_, bg_, s_, bs_))
    ce, cn = torch.empty_like(Ad), torch.empty_like(Ad)
    _lib.check(L().dlpm_coeff_tables_f32(Ad.data_ptr(), g.data_ptr(), s.data_ptr(), bs.data_ptr(), T, B * D, ce.data_ptr(),
                                        cn.data_ptr(), None, st()))

    def run(t, flags, eta=0.0, hist=None):
        a = _lib.UpdateArgs()
        xd, ed, zd = x.to(DEV).contiguous(), eps.to(DEV).contiguous(), z.to(DEV).contiguous()
        td = torch.tensor([t], dtype=torch.int32, device=DEV)
        a.x_dev, a.eps_dev, a.z_dev, a.t_dev = xd.data_ptr(), ed.data_ptr(), zd.data_ptr(), td.data_ptr()
        a.g_dev, a.bg_dev, a.bs_dev = g.data_ptr(), bg.data_ptr(), bs.data_ptr()
        a.c_eps_dev, a.c_noise_dev, a.A_dev = ce.data_ptr(), cn.data_ptr(), Ad.data_ptr()
        a.B, a.D, a.T, a.flags, a.dlim_eta, a.alpha = B, D, T, flags | _lib.UPD_ELEMENTWISE, eta, alpha
        cell = None
        if hist is not None:
            cell = torch.tensor([hist.data_ptr()], dtype=torch.int64, device=DEV)
            a.hist_pp = cell.data_ptr()
        _lib.check(L().dlpm_update_f32(C.byref(a), st()))
        torch.cuda.synchronize()
        return xd.cpu()

    for t in (1, 2, 7, 11):
        want, _, _ = P.dlpm_step(x, eps, t, Sig, g_, bs_, z)
        np.testing.assert_allclose(run(t, 0).numpy(), want.numpy(), rtol=2e-6, atol=2e-6)
        e2 = P.clipped_eps(x, eps, t, bg_, bs_)
        want, _, _ = P.dlpm_step(x, e2, t, Sig, g_, bs_, z)
        np.testing.assert_allclose(run(t, _lib.UPD_CLIP).numpy(), want.numpy(), rtol=3e-6, atol=3e-6)
        want = P.dlim_step(x, eps, t, g_, bs_, eta=0.0)
        np.testing.assert_allclose(run(t, _lib.UPD_DLIM).numpy(), want.numpy(), rtol=2e-6, atol=2e-6)
        want = P.dlim_step(x, eps, t, g_, bs_, eta=0.5, alpha=alpha, A=A, z=z)
        np.testing.assert_allclose(run(t, _lib.UPD_DLIM, eta=0.5).numpy(), want.numpy(), rtol=5e-6, atol=5e-6)
    hist = torch.zeros((T,) + shape, device=DEV)
    got = run(5, 0, hist=hist)
    assert torch.equal(hist[T - 5].cpu(), got) and float(hist.abs().sum()) == float(got.abs().sum())


def test_update_scalar_path_toy_shape():
    """D = 2 (toy data) takes the non-vectorised path."""
    f = golden('f5_traj_synth_toy')
    T, alpha = int(f['meta'][0]), float(f['meta'][1])
    g, bg, s, bs = P.schedule(T, alpha)
    ff = dict(A=f['A'], g=g.numpy(), bg=bg.numpy(), s=s.numpy(), bs=bs.numpy())
    tabs = _tables(ff)
    hist, z = torch.from_numpy(f['history']), torch.from_numpy(f['z'])
    for k, t in [(0, T - 1), (40, T - 41), (98, 1)]:
        x = hist[k]
        eps = 0.5 * x + float(t) * (1.0 / T)
        got, _ = _update(x, eps, z[k], t, tabs)
        want = hist[k + 1]
        assert (got - want).abs().max().item() <= 2e-6 * max(1.0, want.abs().max().item())


def test_philox_noise_statistics_and_sharding():
    B, D, T, alpha = 4096, 64, 8, 1.7
    A = torch.empty(T, B, device=DEV)
    _lib.check(L().dlpm_skewed_levy_philox_f32(A.data_ptr(), T, B, alpha, -1.0, 123, 0, st()))
    a = A.cpu().numpy().ravel().astype(np.float64)
    assert np.all(a > 0) and np.all(np.isfinite(a))
    import scipy.stats
    scale = 2 * np.cos(np.pi * alpha / 4) ** (2 / alpha)
    qs = np.array([0.1, 0.25, 0.5, 0.75, 0.9])
    want_q = scipy.stats.levy_stable.ppf(qs, alpha / 2, 1, loc=0, scale=scale)
    # (= [1.18521284, 1.37370291, 1.75562623, 2.67362479, 5.30812354] with scipy 1.15.3)
    got_q = np.quantile(a, qs)
    # 32768 draws: quantile standard error ~ sqrt(q(1-q)/n)/pdf ~ 1-2 %
    np.testing.assert_allclose(got_q, want_q, rtol=0.06)
    # clamp and the alpha == 2 constant
    _lib.check(L().dlpm_skewed_levy_philox_f32(A.data_ptr(), T, B, alpha, 10.0, 123, 0, st()))
    assert A.max().item() <= 10.0 and A.min().item() >= 0.0
    _lib.check(L().dlpm_skewed_levy_philox_f32(A.data_ptr(), T, B, 2.0, -1.0, 123, 0, st()))
    assert torch.all(A == 2.0).item()
    # sharding invariance: rows [b0, b1) drawn with sample_offset = b0 equal the slice of the full draw
    full = torch.empty(T, B, device=DEV)
    _lib.check(L().dlpm_skewed_levy_philox_f32(full.data_ptr(), T, B, alpha, -1.0, 9, 0, st()))
    part = torch.empty(T, B // 4, device=DEV)
    _lib.check(L().dlpm_skewed_levy_philox_f32(part.data_ptr(), T, B // 4, alpha, -1.0, 9, B // 2, st()))
    assert torch.equal(part.cpu(), full.cpu()[:, B // 2:B // 2 + B // 4])
    # x_T init: z statistics (alpha = 2 -> a0 = 2, x = bs * sqrt(2) z)
    x = torch.empty(B, D, device=DEV)
    _lib.check(L().dlpm_init_state_philox_f32(x.data_ptr(), B, D, 2.0, -1.0, 1.0, 5, 0, st()))
    zz = (x.cpu().numpy().ravel() / math.sqrt(2.0)).astype(np.float64)
    n = zz.size
    assert abs(zz.mean()) < 5 / math.sqrt(n) and abs(zz.var() - 1) < 5 * math.sqrt(2 / n)
    assert abs((zz ** 4).mean() - 3) < 0.1 and scipy.stats.kstest(zz[:20000], 'norm').pvalue > 1e-4
    xs = torch.empty(B // 2, D, device=DEV)
    _lib.check(L().dlpm_init_state_philox_f32(xs.data_ptr(), B // 2, D, 2.0, -1.0, 1.0, 5, B // 2, st()))
    assert torch.equal(xs.cpu(), x.cpu()[B // 2:])


def test_update_philox_is_linear_and_shard_invariant_at_full_size():
    """BASELINE config 3 size (B=1024, D=3072): properties that need no oracle at this size.
    x' = (x - c_eps eps)/g + c_noise z(seed, sample, t): affine in (x, eps) for fixed noise."""
    B, D, T, alpha = 1024, 3072, 1000, 1.7
    g, bg, s, bs = (v.to(DEV) for v in P.schedule(T, alpha))
    A = torch.empty(T, B, device=DEV)
    _lib.check(L().dlpm_skewed_levy_philox_f32(A.data_ptr(), T, B, alpha, 10.0, 7, 0, st()))
    ce, cn = torch.empty_like(A), torch.empty_like(A)
    _lib.check(L().dlpm_coeff_tables_f32(A.data_ptr(), g.data_ptr(), s.data_ptr(), bs.data_ptr(), T, B, ce.data_ptr(),
                                        cn.data_ptr(), None, st()))
    tabs = (g, bg, bs, ce, cn, A)
    gen = torch.Generator().manual_seed(3)
    x, e = torch.randn(B, D, generator=gen), torch.randn(B, D, generator=gen)
    t = 500
    zero = torch.zeros(B, D)
    n0, _ = _update(zero, zero, None, t, tabs, seed=11)          # pure noise term
    full, _ = _update(x, e, None, t, tabs, seed=11)
    det, _ = _update(x, e, zero, t, tabs, seed=11)               # injected z = 0: deterministic part
    assert (full - (det + n0)).abs().max().item() <= 1e-5 * full.abs().max().item()
    # noise term has the right per-sample scale
    ratio = n0.std(dim=1) / cn[t].cpu()
    assert (ratio - 1).abs().max().item() < 0.08
    # shard invariance: the second half processed alone with sample_offset = B/2
    tabs_h = (g, bg, bs, ce[:, B // 2:].contiguous(), cn[:, B // 2:].contiguous(), A[:, B // 2:].contiguous())
    half, _ = _update(x[B // 2:], e[B // 2:], None, t, tabs_h, seed=11, offset=B // 2)
    assert torch.equal(half, full[B // 2:])
    # a different seed or step gives different noise
    other, _ = _update(zero, zero, None, t, tabs, seed=12)
    assert not torch.equal(other, n0)


def test_postprocess_matches_generation_manager_fixture():
    f = golden('f8_generation_manager')
    for tag, clamp, aff in (('img', 1.0, 1), ('toy', 6.0, 0)):
        x = torch.from_numpy(f[tag + '_x']).to(DEV)
        o = torch.empty_like(x)
        _lib.check(L().dlpm_postprocess_f32(x.data_ptr(), o.data_ptr(), x.numel(), clamp, aff, st()))
        assert np.array_equal(o.cpu().numpy(), f[tag + '_samples'])


def test_groupnorm_large_offset_is_stable():
    """|mean| >> std (offset 100, std 0.05): the one-pass shifted statistics must not cancel."""
    g = torch.Generator().manual_seed(9)
    C, hw, B = 128, 16, 2
    x = 100.0 + 0.05 * torch.randn(B, C, hw, hw, generator=g) + 0.3 * torch.randn(B, C, 1, 1, generator=g)
    gam, bet = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    want = torch.nn.functional.group_norm(x.double(), 32, gam.double(), bet.double(), 1e-5).float()
    xd, gd, bd = nhwc(x).to(DEV), gam.to(DEV), bet.to(DEV)
    cA, cB = torch.empty(B, C, device=DEV), torch.empty(B, C, device=DEV)
    _lib.check(L().dlpm_groupnorm_coeffs_f32(xd.data_ptr(), None, C, 0, B, hw * hw, 32, gd.data_ptr(), bd.data_ptr(),
                                            None, 0, 0, cA.data_ptr(), cB.data_ptr(), st()))
    y = (x.double() * cA.cpu().double()[:, :, None, None] + cB.cpu().double()[:, :, None, None]).float()
    # x*A + B with |x| = 100, A ~ 3: the affine form itself carries ~100*3*6e-8 = 2e-5 of rounding in B
    assert (y - want).abs().max().item() < 2e-4


SPLIT_CASES = [
    # name, B, C0, C1, H, Cout, coef, silu, res     (shapes of the UNet's 1x1 convolutions, small batches)
    ('qkv_8x8', 4, 256, 0, 8, 768, True, False, False),
    ('proj_res_8x8', 4, 256, 0, 8, 256, False, False, True),
    ('skip_concat_32x32', 1, 128, 128, 32, 128, False, False, False),
    ('skip_concat_256_128', 2, 256, 128, 16, 256, False, False, False),
    ('gn_silu_128', 2, 128, 0, 8, 128, True, True, False),
    ('long_k_512', 2, 256, 256, 8, 256, False, False, True),
    ('ragged_qkv_4x4_b3', 3, 256, 0, 4, 768, True, False, False),       # M = 48: one partial tile, 3 samples of 8 in its table
    ('ragged_proj_res_8x8_b3', 3, 256, 0, 8, 256, False, False, True),  # M = 192: a full and a half tile
    ('xcd_mapped_qkv_8x8_b16', 16, 256, 0, 8, 384, True, False, False),  # 8 pixel tiles x 3 channel tiles
    # round 5, k_conv_split_pipe's loop tails: a 32-channel pair = 2 k-steps, the loop is unrolled by 4 with a guarded tail
    ('pipe_one_pair_k32', 2, 32, 0, 8, 128, True, True, False),          # 2 k-steps: prologue + tail only (clamped prologue loads)
    ('pipe_three_pairs_concat_64_32', 2, 64, 32, 16, 128, True, False, True),   # 6 k-steps: the tail trip is half a trip
    ('pipe_five_pairs_k160', 1, 160, 0, 8, 256, False, False, False),    # 10 k-steps: one steady trip + a whole + half tail
    ('pipe_seven_pairs_k224_ragged', 3, 128, 96, 4, 128, True, False, True),    # 14 k-steps, M = 48
]


@pytest.mark.parametrize('case', SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_conv1x1_bf16_split_gemm_is_fp32_grade(case):
    """conv_split.hip (force_direct bit 4): fp32 operands cut exactly into three bf16 planes, six partial products per
    multiply, fp32 accumulation on the bf16 matrix pipe.  Judged against float64 next to the fp32 MFMA kernel on the same
    inputs: its error may not exceed 1.5x the fp32 kernel's (+ one ulp of slack), and both stay inside the fp32
    accumulation bound.  Operands span 12 binades, with exact zeros and tiny (1e-30) magnitudes mixed in."""
    name, B, C0, C1, H, Cout, use_coef, silu, use_res = case
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    Cin = C0 + C1
    scale = lambda *s: torch.exp2(torch.randint(-6, 7, s, generator=g).float())
    x0 = torch.randn(B, C0, H, H, generator=g) * scale(B, C0, H, H)
    x0[0, :8, 0, 0] = 0.0
    x0[0, 8:16, 0, 0] = 1e-30
    x1 = torch.randn(B, C1, H, H, generator=g) if C1 else None
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / math.sqrt(Cin) * scale(Cout, Cin, 1, 1) / 8
    w[0, :4] = 0.0
    bias = torch.randn(Cout, generator=g)
    coef = (1 + 0.3 * torch.randn(B, Cin, generator=g), 0.3 * torch.randn(B, Cin, generator=g)) if use_coef else None
    res = torch.randn(B, Cout, H, H, generator=g) if use_res else None
    x = x0 if x1 is None else torch.cat([x0, x1], 1)
    if coef is not None:
        x = x * coef[0][:, :, None, None] + coef[1][:, :, None, None]
    if silu:
        x = nets.silu(x)
    want = F.conv2d(x.double(), w.double(), bias.double())
    if res is not None:
        want = want + res.double()
    mag = F.conv2d(x.double().abs(), w.double().abs()).max().item()   # sum |a||b|: what fp32 accumulation errors scale with
    got32 = run_conv(x0, w, bias, x1, 1, 0, coef, silu, res).double()
    got16 = run_conv(x0, w, bias, x1, 1, 0, coef, silu, res, force_direct=16).double()
    e32, e16 = (got32 - want).abs().max().item(), (got16 - want).abs().max().item()
    print('%s: fp32 MFMA err %.2e, bf16x3 err %.2e (sum|a||b| max %.1f, Cin %d)' % (name, e32, e16, mag, Cin))
    assert e16 <= 1.5 * e32 + 1.2e-7 * mag, name
    assert e16 < 3e-7 * math.sqrt(Cin) * mag, name
    assert not torch.equal(got16, got32) or e16 == 0.0   # the split kernel really ran (different rounding order)


_PIPE_DIGEST_SCRIPT = r"""
import hashlib, sys, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_kernels as T
h = hashlib.sha256()
for name, B, C0, C1, H, Cout, use_coef, silu, use_res in T.SPLIT_CASES:
    g = torch.Generator().manual_seed(len(name))
    x0 = torch.randn(B, C0, H, H, generator=g)
    x1 = torch.randn(B, C1, H, H, generator=g) if C1 else None
    w = torch.randn(Cout, C0 + C1, 1, 1, generator=g) / (C0 + C1) ** 0.5
    bias = torch.randn(Cout, generator=g)
    coef = (1 + 0.3 * torch.randn(B, C0 + C1, generator=g), 0.3 * torch.randn(B, C0 + C1, generator=g)) if use_coef else None
    res = torch.randn(B, Cout, H, H, generator=g) if use_res else None
    h.update(T.run_conv(x0, w, bias, x1, 1, 0, coef, silu, res, force_direct=16).numpy().tobytes())
print(h.hexdigest())
"""


def test_pipelined_split_gemm_is_bit_identical_to_the_two_barrier_kernel():
    """k_conv_split_pipe (round 5: one k-step per LDS stage, one barrier per k-step) accumulates every output in the order of
    k_conv_split<8, 1, 1>: every SPLIT_CASES shape -- ragged tiles, every loop-tail length, concat, GroupNorm table, residual --
    must come out bit for bit the same from both.  DLPM_SPLIT_PIPE is read once per process: two child processes, one digest each."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for pipe in ('1', '0'):
        e = dict(os.environ, DLPM_SPLIT_PIPE=pipe)
        r = subprocess.run([sys.executable, '-c', _PIPE_DIGEST_SCRIPT, root], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out[pipe] = r.stdout.strip().splitlines()[-1]
    assert len(out['1']) == 64 and out['1'] == out['0'], out


_WHOLE_IMAGE_DIGEST_SCRIPT = r"""
import hashlib, sys, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_kernels as T
import dlpm_amd
h = hashlib.sha256()
for name, B, C0, C1, use_coef, use_res in T.WHOLE_IMAGE_CASES:
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x0 = torch.randn(B, C0, 32, 32, generator=g)
    x1 = torch.randn(B, C1, 32, 32, generator=g) if C1 else None
    w = torch.randn(32, C0 + C1, 3, 3, generator=g) / (9 * (C0 + C1)) ** 0.5
    bias = torch.randn(32, generator=g)
    coef = (1 + 0.3 * torch.randn(B, C0 + C1, generator=g), 0.3 * torch.randn(B, C0 + C1, generator=g)) if use_coef else None
    res = torch.randn(B, 32, 32, 32, generator=g) if use_res else None
    got = T.run_conv(x0, w, bias, x1, 1, 0, coef, use_coef, res, force_direct=8)
    want = T.ref_conv(x0, w, bias, x1, 1, 0, coef, use_coef, res)
    assert (got - want).abs().max().item() < 2e-5, name
    h.update(got.numpy().tobytes())
# ... and inside the MNIST-sized net, where the kernel also emits the GroupNorm statistics its consumers normalise with
p = dlpm_amd.load_config('mnist')
torch.manual_seed(1234)
net = dlpm_amd.rerandomize_(dlpm_amd.init_model_by_parameter(p), 4321).to('cuda')
g = torch.Generator().manual_seed(5)
x = torch.randn(5, 1, 32, 32, generator=g).cuda()
t = torch.rand(5, generator=g).cuda()
h.update(net(x, t).cpu().numpy().tobytes())
print(h.hexdigest())
"""

WHOLE_IMAGE_CASES = [
    # name, B, C0, C1, coef + silu, res   -- 32 output channels on 32x32 images: k_conv3x3_wino4_img
    ('img_32_gn_silu_res', 3, 32, 0, True, True),
    ('img_32_plain', 1, 32, 0, False, False),
    ('img_concat_64_32_gn_silu', 2, 64, 32, True, False),
    ('img_concat_32_32_gn_silu', 2, 32, 32, True, False),
    ('img_96_gn_silu_res', 1, 96, 0, True, True),
]


def test_conv_winograd_f4_whole_image_is_bit_identical():
    """Round 6: k_conv3x3_wino4_img (one workgroup per 32x32 image, 8 MFMA waves, phases run one after the other) is a re-scheduling of the
    2 + 2-wave 16-tile shape's arithmetic -- same staged values, same transform expressions, same k order per accumulator, same epilogue
    and statistics partials: every case (against fp64 inside the child, 2e-5) and the whole MNIST-sized UNet forward must come out bit
    for bit the same with DLPM_WINO4_IMG=1 (default) and =0.  Read once per process: two child processes, one digest each."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for img in ('1', '0'):
        e = dict(os.environ, DLPM_WINO4_IMG=img)
        r = subprocess.run([sys.executable, '-c', _WHOLE_IMAGE_DIGEST_SCRIPT, root], env=e, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        out[img] = r.stdout.strip().splitlines()[-1]
    assert len(out['1']) == 64 and out['1'] == out['0'], out


_MNIST_NET_DIGEST_SCRIPT = r"""
import hashlib, sys, torch
sys.path.insert(0, sys.argv[1])
import dlpm_amd
p = dlpm_amd.load_config('mnist')
torch.manual_seed(1234)
net = dlpm_amd.rerandomize_(dlpm_amd.init_model_by_parameter(p), 4321).to('cuda')
g = torch.Generator().manual_seed(5)
x = torch.randn(5, 1, 32, 32, generator=g).cuda()
t = torch.rand(5, generator=g).cuda()
h = hashlib.sha256()
h.update(net(x, t).cpu().numpy().tobytes())
h.update(net(x[1:3], t[1:3]).cpu().numpy().tobytes())
print(h.hexdigest())
"""


def test_resblock_whole_image_is_bit_identical_to_the_separate_launches():
    """Round 6: k_resblock_wino4_img (a whole 32-channel ResBlock of a 32x32 image in one launch: GroupNorm-1 from the producers'
    statistics, conv1, GroupNorm-2 with scale-shift inside the workgroup, conv2 over the activated intermediate, skip, statistics)
    evaluates the expressions of the launches it replaces (conv -> k_gn_coeffs_stats -> conv; gn_stats.h is shared): the whole
    MNIST-sized UNet forward -- five such blocks, identity and 1x1-convolution skips, concat inputs, sources with 1 and 4 statistics
    partials -- must come out bit for bit the same with DLPM_RES_IMG=1 (default) and =0.  Two child processes, one digest each."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for v in ('1', '0'):
        e = dict(os.environ, DLPM_RES_IMG=v, DLPM_RES_IMG16='0')   # (the 16x16 shape splits K over wave pairs: its own rounding, off in both)
        r = subprocess.run([sys.executable, '-c', _MNIST_NET_DIGEST_SCRIPT, root], env=e, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        out[v] = r.stdout.strip().splitlines()[-1]
    assert len(out['1']) == 64 and out['1'] == out['0'], out


SPLIT3_CASES = [
    # name, B, C0, C1, H, Cout, stride, coef+silu, res
    ('down_16_to_8', 3, 128, 0, 16, 128, 2, False, False),
    ('down_8_to_4_256', 2, 256, 0, 8, 256, 2, False, False),
    ('down_32_to_16_stats_tile', 1, 128, 0, 32, 128, 2, False, False),      # 256 output pixels per image: whole 128-pixel tiles
    ('s1_4x4_gn_silu_res', 5, 128, 0, 4, 128, 1, True, True),               # ragged: 80 output pixels
    ('s1_8x8_concat', 2, 128, 64, 8, 256, 1, True, False),
    ('down_odd_input_7_to_4', 2, 64, 0, 7, 128, 2, False, False),
]


@pytest.mark.parametrize('case', SPLIT3_CASES, ids=[c[0] for c in SPLIT3_CASES])
def test_conv3x3_bf16_split_implicit_gemm(case):
    """The 3x3 (padding 1, stride 1 / 2) form of conv_split.hip -- what the UNet's stride-2 downsampling convolutions take
    (unet.py:96, Downsample.op): judged against float64 beside the fp32 implicit-GEMM kernel, like the 1x1 form."""
    name, B, C0, C1, H, Cout, stride, act, use_res = case
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    Cin = C0 + C1
    x0 = torch.randn(B, C0, H, H, generator=g)
    x1 = torch.randn(B, C1, H, H, generator=g) if C1 else None
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    bias = torch.randn(Cout, generator=g)
    coef = (1 + 0.3 * torch.randn(B, Cin, generator=g), 0.3 * torch.randn(B, Cin, generator=g)) if act else None
    Ho = (H - 1) // stride + 1
    res = torch.randn(B, Cout, Ho, Ho, generator=g) if use_res else None
    want = ref_conv(x0, w, bias, x1, stride, 0, coef, act, res).double()
    x = x0 if x1 is None else torch.cat([x0, x1], 1)
    if coef is not None:
        x = x * coef[0][:, :, None, None] + coef[1][:, :, None, None]
    if act:
        x = nets.silu(x)
    want = F.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=1)
    if res is not None:
        want = want + res.double()
    mag = F.conv2d(x.double().abs(), w.double().abs(), stride=stride, padding=1).max().item()
    got32 = run_conv(x0, w, bias, x1, stride, 0, coef, act, res, force_direct=2).double()
    got16 = run_conv(x0, w, bias, x1, stride, 0, coef, act, res, force_direct=16).double()
    e32, e16 = (got32 - want).abs().max().item(), (got16 - want).abs().max().item()
    print('%s: fp32 implicit GEMM err %.2e, bf16x3 err %.2e (sum|a||b| max %.1f)' % (name, e32, e16, mag))
    assert e16 <= 1.5 * e32 + 1.2e-7 * mag, name
    assert e16 < conv_tol(w, Cin), name
    assert not torch.equal(got16, got32)


# ---------------------------------------------------------------- round 4: whole blocks of small images in one launch (block_small.hip)
@pytest.mark.parametrize('cin,hs', [(64, 8), (64, 4), (128, 8), (128, 4)])
def test_fused_small_resblock_vs_reference(cin, hs):
    """k_resblock_small (GroupNorm + SiLU + conv3x3 + GroupNorm x (1 + scale) + shift + SiLU + conv3x3 + skip in ONE launch, one
    workgroup per image) against the reference's ResBlock (unet.py:105-196) on the F13 fixtures -- 64 -> 64 with the identity
    skip, 128 (= concat 64 | 64) -> 64 with the 1x1 skip convolution, 8x8 and 4x4 -- and bit-independence of the batch."""
    import small_block_weights as sbw
    from test_gpu_fused_blocks import image, launch_res      # (the launch every whole-block test shares)
    from oracle import nets
    f = golden('f13_small_blocks')
    tag = 'res_c%d_h%d_' % (cin, hs)
    sd = sbw.res_state(cin, hs)
    assert sbw.digest(sd) == bytes(f[tag + 'digest']).hex()
    x, emb, want = torch.from_numpy(f[tag + 'x']), torch.from_numpy(f[tag + 'emb']), f[tag + 'y']
    ss = torch.nn.functional.linear(nets.silu(emb), sd['emb_layers.1.weight'], sd['emb_layers.1.bias'])   # the block's emb_layers (host)

    def run(xb, ssb):
        r = launch_res('res_small', sd, xb, ssb, 64, cin - 64)
        return image(r), r['stats'].view(-1, 64, 2)

    got, stats = run(x, ss)
    err = (got.numpy() - want).__abs__().max()
    print('fused ResBlock %d -> 64 at %dx%d: max |hip - reference| = %.3g (|y| max %.3g)' % (cin, hs, hs, err, np.abs(want).max()))
    assert err < 2e-5 * max(1.0, np.abs(want).max())
    # per-image statistics of the output (what a GroupNorm consumer reads): mean and centred sum of squares per channel
    g64 = got.double()
    assert (stats[..., 0].double() - g64.mean(dim=(2, 3))).abs().max() < 1e-5
    m2 = ((g64 - g64.mean(dim=(2, 3), keepdim=True)) ** 2).sum(dim=(2, 3))
    assert ((stats[..., 1].double() - m2).abs() / (1 + m2)).max() < 1e-5
    # a sample's bits do not depend on the batch it travels in
    big = torch.cat([x[2:3], x, x[0:1]])
    gb, _ = run(big, torch.cat([ss[2:3], ss, ss[0:1]]))
    assert torch.equal(gb[1:4], got) and torch.equal(gb[0], got[2]) and torch.equal(gb[4], got[0])


@pytest.mark.parametrize('cin', [64, 128, 96])
def test_whole_image_resblock_16x16_vs_reference(cin):
    """Round 6: k_resblock_wino4_img16 (a whole 64-channel ResBlock of a 16x16 image in one launch: the intermediate stays in LDS, the K loop is
    split over wave pairs) against the reference's ResBlock (unet.py:105-196) on the F14 fixtures -- 64 -> 64 with the identity skip, 128
    (= 64 | 64) and 96 (= 64 | 32) -> 64 with the 1x1 skip convolution -- its per-image statistics, and bit-independence of the batch."""
    import small_block_weights as sbw
    from test_gpu_fused_blocks import image, launch_res      # (the launch every whole-block test shares)
    from oracle import nets
    f = golden('f14_blocks16')
    tag = 'res_c%d_o64_h16_' % cin
    sd = sbw.res_fine_state(cin, 64, 16)
    assert sbw.digest(sd) == bytes(f[tag + 'digest']).hex()
    x, emb = sbw.res_fine_input(cin, 16, 2)
    assert sbw.input_digest(x, emb) == bytes(f[tag + 'xdigest']).hex()
    want = f[tag + 'y']
    ss = torch.nn.functional.linear(nets.silu(emb), sd['emb_layers.1.weight'], sd['emb_layers.1.bias'])

    def run(xb, ssb):
        r = launch_res('res_img16', sd, xb, ssb, 64, cin - 64)
        return image(r), r['stats'].view(-1, 64, 2)

    got, stats = run(x, ss)
    err = np.abs(got.numpy() - want).max()
    print('whole-image ResBlock %d -> 64 at 16x16: max |hip - reference| = %.3g (|y| max %.3g)' % (cin, err, np.abs(want).max()))
    assert err < 2e-5 * max(1.0, np.abs(want).max())
    g64 = got.double()
    assert (stats[..., 0].double() - g64.mean(dim=(2, 3))).abs().max() < 1e-5
    m2 = ((g64 - g64.mean(dim=(2, 3), keepdim=True)) ** 2).sum(dim=(2, 3))
    assert ((stats[..., 1].double() - m2).abs() / (1 + m2)).max() < 1e-5
    big = torch.cat([x[1:2], x, 0.5 * x[0:1]])
    gb, _ = run(big, torch.cat([ss[1:2], ss, ss[0:1] + 0.1]))
    assert torch.equal(gb[1:3], got) and torch.equal(gb[0], got[1])


@pytest.mark.parametrize('cin', [32, 64, 96])
def test_whole_image_resblock_vs_reference(cin):
    """Round 6: k_resblock_wino4_img (a whole 32-channel ResBlock of a 32x32 image in one launch, Winograd F(4x4,3x3) inside) against the
    reference's ResBlock (unet.py:105-196) on the F14 fixtures -- 32 -> 32 with the identity skip, 64 (= concat 32 | 32) and 96 (= 64 | 32)
    -> 32 with the 1x1 skip convolution -- the quadrant statistics it emits, and bit-independence of the batch."""
    import small_block_weights as sbw
    from test_gpu_fused_blocks import image, launch_res      # (the launch every whole-block test shares)
    from oracle import nets
    f = golden('f14_blocks16')
    tag = 'res_c%d_o32_h32_' % cin
    sd = sbw.res_fine_state(cin, 32, 32)
    assert sbw.digest(sd) == bytes(f[tag + 'digest']).hex()
    x, emb = sbw.res_fine_input(cin, 32, 1)
    assert sbw.input_digest(x, emb) == bytes(f[tag + 'xdigest']).hex()
    want = f[tag + 'y']
    ss = torch.nn.functional.linear(nets.silu(emb), sd['emb_layers.1.weight'], sd['emb_layers.1.bias'])   # the block's emb_layers (host)
    c0 = {32: 32, 64: 32, 96: 64}[cin]

    def run(xb, ssb):
        r = launch_res('res_img32', sd, xb, ssb, c0, cin - c0)
        return image(r), r['stats'].view(-1, 4, 32, 2)

    got, stats = run(x, ss)
    err = np.abs(got.numpy() - want).max()
    print('whole-image ResBlock %d -> 32 at 32x32: max |hip - reference| = %.3g (|y| max %.3g)' % (cin, err, np.abs(want).max()))
    assert err < 2e-5 * max(1.0, np.abs(want).max())
    # statistics partials: (mean, centred sum of squares) of each 16x16 quadrant (row-major) per channel
    g64 = got.double()
    for q in range(4):
        blk = g64[:, :, 16 * (q // 2):16 * (q // 2) + 16, 16 * (q % 2):16 * (q % 2) + 16]
        assert (stats[:, q, :, 0].double() - blk.mean(dim=(2, 3))).abs().max() < 1e-5
        m2 = ((blk - blk.mean(dim=(2, 3), keepdim=True)) ** 2).sum(dim=(2, 3))
        assert ((stats[:, q, :, 1].double() - m2).abs() / (1 + m2)).max() < 1e-5
    # a sample's bits do not depend on the batch it travels in (other images: the same one scaled, with its own emb row)
    big = torch.cat([0.5 * x, x, 2.0 * x])
    gb, _ = run(big, torch.cat([ss + 0.1, ss, ss - 0.1]))
    assert torch.equal(gb[1:2], got)


def test_fused_attention_block_16x16_vs_reference():
    """Round 6: k_attnblock16 (GroupNorm -> per head: qkv, softmax(q k^T) v, proj accumulated in registers -> + x, ONE launch per 16x16
    image) against the reference's AttentionBlock (unet.py:199-250) at T = 256 (tests/golden/f14_blocks16.npz), its per-image output
    statistics, and bit-independence of the batch."""
    import small_block_weights as sbw
    from test_gpu_fused_blocks import image, launch_attn     # (the launch every whole-block test shares)
    f = golden('f14_blocks16')
    sd = sbw.attn16_state()
    assert sbw.digest(sd) == bytes(f['attn_h16_digest']).hex()
    x, want = sbw.attn16_input(), f['attn_h16_y']
    assert sbw.input_digest(x) == bytes(f['attn_h16_xdigest']).hex()

    def run(xb, with_stats=True):
        r = launch_attn(sd, xb, with_stats=with_stats)
        return image(r), r['stats'].view(-1, 64, 2)

    got, stats = run(x)
    err = np.abs(got.numpy() - want).max()
    print('fused AttentionBlock at 16x16: max |hip - reference| = %.3g (|y| max %.3g)' % (err, np.abs(want).max()))
    assert err < 2e-5 * max(1.0, np.abs(want).max())
    g64 = got.double()
    assert (stats[..., 0].double() - g64.mean(dim=(2, 3))).abs().max() < 1e-5
    m2 = ((g64 - g64.mean(dim=(2, 3), keepdim=True)) ** 2).sum(dim=(2, 3))
    assert ((stats[..., 1].double() - m2).abs() / (1 + m2)).max() < 1e-5
    gb, _ = run(torch.cat([x[1:2], x, x[0:1]]), with_stats=False)
    assert torch.equal(gb[1:3], got) and torch.equal(gb[0], got[1]) and torch.equal(gb[3], got[0])


@pytest.mark.parametrize('hs', [8, 4])
def test_fused_small_attention_block_vs_reference(hs):
    """k_attnblock_small (GroupNorm -> qkv -> softmax(q k^T) v per head -> proj -> + x in one launch) against the reference's
    AttentionBlock (unet.py:199-250), 64 channels, 4 heads, T = 64 and 16."""
    import small_block_weights as sbw
    from test_gpu_fused_blocks import image, launch_attn     # (the launch every whole-block test shares)
    f = golden('f13_small_blocks')
    tag = 'attn_h%d_' % hs
    sd = sbw.attn_state(hs)
    assert sbw.digest(sd) == bytes(f[tag + 'digest']).hex()
    x, want = torch.from_numpy(f[tag + 'x']), f[tag + 'y']

    def run(xb):
        return image(launch_attn(sd, xb, with_stats=False))

    got = run(x)
    err = np.abs(got.numpy() - want).max()
    print('fused AttentionBlock at %dx%d: max |hip - reference| = %.3g (|y| max %.3g)' % (hs, hs, err, np.abs(want).max()))
    assert err < 2e-5 * max(1.0, np.abs(want).max())
    gb = run(torch.cat([x[1:2], x]))
    assert torch.equal(gb[1:], got) and torch.equal(gb[0], got[1])
