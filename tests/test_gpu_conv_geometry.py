"""Every block shape and image size the convolution routes admit, one launch at a time against float64.

1. The Winograd families.  tests/conv_geometry_cases.py holds one row per class (family, upsample, n-tile, block of bh x bw tiles, images
per block) the route predicates admit on images up to 96x96 -- 139 classes, 107 of which no square power-of-two image reaches -- and six
images with 3 and 5 blocks per row (tests/test_conv_geometry_cpu.py pins the routes and the coverage).  Each row is launched through
launch() of test_gpu_conv_policy.py, which asserts the route it TOOK -- block shape and statistics size included -- before anything else,
NaN-prefills the output and keeps canaries behind it.  Then, per row:
  against float64 (ref_conv, inputs seeded as in test_conv): F(2x2) rows under conv_tol(w, Cin); F(4x4) and sub-pixel rows under 2e-5,
  the ceiling of test_conv_winograd_f4 -- the arithmetic per output does not depend on the block shape (measured: profiles/geometry);
  where the route emits statistics: the same launch with statistics has the same bits, and its partials pass check_partials_of with the
  layout BLK(4 bh, 4 bw) (BLK(2 bh, 2 bw) for F(2x2), SUBPIX(8 bh, 8 bw) for the sub-pixel kernel) at the default bounds 1e-5 / 1e-5;
  where a block holds several images: image 0 of the launch has the bits of a B = 1 launch of image 0 alone.
2. The implicit-GEMM family at the sizes the Winograd routes refuse (24x24, 12x12, 6x10, 28x20, 14 -> 7, 7 -> 4, 5x5-level shapes ...),
through run_conv / ref_conv under conv_tol: the default route and the direct kernel; and the bf16x3 kernel at the non-square shapes
conv_split_ok admits, under the two relations of test_conv1x1_bf16_split_gemm_is_fp32_grade.
3. GroupNorm coefficients from the tensor at the pixel counts those levels produce, against F.group_norm in float64 (3e-6 plain, 4e-6 with
scale-shift + SiLU: test_groupnorm_coeffs_against_reference_fixture's)."""
import math

import pytest
import torch
import torch.nn.functional as F

from conv_geometry_cases import BY_NAME, GEN, ROWS, alone_route, want_route
from conv_policy_cases import descriptor, query
from dlpm_amd import _lib
from test_gpu_conv_policy import launch, make_of, pick
from test_gpu_gn_stats import BLK, ROWS as ROW_SLOTS, SUBPIX, check_partials_of
from test_gpu_kernels import DEV, L, conv_tol, nhwc, ref_conv, run_conv, st

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. the Winograd families
def run(g, inp, route=None, **kw):
    return launch(g.case, inp, gen=GEN[g.gen], want_route=route or want_route(g), **kw)


def stats_layout(g):
    if g.case.family == 'WINO':
        return BLK(2 * g.bh, 2 * g.bw)
    if g.case.family == 'WINO4':
        return BLK(4 * g.bh, 4 * g.bw)
    return SUBPIX(8 * g.bh, 8 * g.bw)


@pytest.mark.parametrize('name', [g.case.name for g in ROWS])
def test_block_shape(name):
    g = BY_NAME[name]
    c, inp = g.case, make_of(g.case)
    # route (asserted inside launch, before the kernel runs), canaries, every output element written
    r = run(g, inp)
    assert r['rc'] == 0 and r['intact'], name
    assert r['part'] is None and bool(torch.isfinite(r['out']).all()), name
    # against float64
    want = ref_conv(inp['x0'], inp['w'], inp['bias'], inp['x1'], 1, c.ups, inp['coef'], c.act, inp['res'])
    assert r['out'].shape == want.shape
    err = (r['out'] - want).abs().max().item()
    tol = conv_tol(inp['w'], c.C0 + c.C1) if c.family == 'WINO' else 2e-5
    print('GEOMETRY %s %s max |out - fp64| %.3e bound %.3e' % (c.family, name, err, tol))
    assert err < tol, (name, err)
    # statistics
    if g.stats_px > 0:
        s = run(g, inp, stats=True)
        assert s['rc'] == 0 and s['intact'] and torch.equal(s['out'], r['out']), name
        check_partials_of(name, s['out'], s['stats'], s['px'], g.stats_px, stats_layout(g), (1e-5, 1e-5))
    else:
        s = run(g, inp, stats=True)
        assert s['rc'] == -3 and s['untouched'], name               # DLPM_ERR_UNSUPPORTED, as the route says: nothing is written
    # batch independence
    if c.nimg > 1:
        # (the route of the image alone: the row's own, or -- the 64-tile F(2x2) blocks of a large batch -- the 4-wave 32-tile shape, whose
        # bits the project claims to be the same: tests/test_conv_geometry_cpu.py)
        alone = run(g, pick(inp, slice(0, 1)), route=alone_route(g))
        assert alone['rc'] == 0 and alone['intact'] and torch.equal(alone['out'][0], r['out'][0]), name


# ---------------------------------------------------------------- 2. the implicit-GEMM family
IGEMM_CASES = [
    # name, B, C0, C1, Hin, Win, Cout, ks, stride, ups, coef, silu, res
    ('s1_24x24_b2_32to64', 2, 32, 0, 24, 24, 64, 3, 1, 0, False, False, False),       # MODE 1: full 128-pixel tiles, one across two images
    ('s1_12x12_b3_32to64', 3, 32, 0, 12, 12, 64, 3, 1, 0, False, False, False),       # M = 432: ragged M
    ('s1_6x10_b5_32_32to96_coef_silu_res', 5, 32, 32, 6, 10, 96, 3, 1, 0, True, True, True),   # M = 300, Cout 96: ragged M and N
    ('s1_28x20_b2_32to64', 2, 32, 0, 28, 20, 64, 3, 1, 0, False, False, False),
    ('s2_12to6_b2_32to64', 2, 32, 0, 12, 12, 64, 3, 2, 0, False, False, False),
    ('s2_14to7_b3_32to64', 3, 32, 0, 14, 14, 64, 3, 2, 0, False, False, False),
    ('s2_7to4_b2_32to64', 2, 32, 0, 7, 7, 64, 3, 2, 0, False, False, False),
    ('s2_6x10to3x5_b2_32to64', 2, 32, 0, 6, 10, 64, 3, 2, 0, False, False, False),
    ('ups_6to12_b2_32to64', 2, 32, 0, 6, 6, 64, 3, 1, 1, False, False, False),
    ('ups_3x5to6x10_b2_32to64', 2, 32, 0, 3, 5, 64, 3, 1, 1, False, False, False),
    ('ups_12to24_b2_32to64_coef_res', 2, 32, 0, 12, 12, 64, 3, 1, 1, True, False, True),
    ('1x1_12x12_b2_64to192_coef', 2, 64, 0, 12, 12, 192, 1, 1, 0, True, False, False),
    ('1x1_6x6_b2_64to64_res', 2, 64, 0, 6, 6, 64, 1, 1, 0, False, False, True),
    ('1x1_24x24_b2_64_64to128', 2, 64, 64, 24, 24, 128, 1, 1, 0, False, False, False),
]


def out_hw(Hin, Win, ks, stride, ups):
    up = 2 if ups else 1
    return (Hin * up + 2 * (ks // 2) - ks) // stride + 1, (Win * up + 2 * (ks // 2) - ks) // stride + 1


def seeded(name, B, C0, C1, Hin, Win, Cout, ks, stride, ups, use_coef, use_res):
    """Inputs seeded as in test_conv"""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    Cin = C0 + C1
    x0 = torch.randn(B, C0, Hin, Win, generator=g)
    x1 = torch.randn(B, C1, Hin, Win, generator=g) if C1 else None
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / math.sqrt(Cin * ks * ks)
    bias = torch.randn(Cout, generator=g)
    coef = (1 + 0.3 * torch.randn(B, Cin, generator=g), 0.3 * torch.randn(B, Cin, generator=g)) if use_coef else None
    res = torch.randn(B, Cout, *out_hw(Hin, Win, ks, stride, ups), generator=g) if use_res else None
    return x0, x1, w, bias, coef, res


@pytest.mark.parametrize('case', IGEMM_CASES, ids=[c[0] for c in IGEMM_CASES])
def test_implicit_gemm_where_winograd_refuses(case):
    name, B, C0, C1, Hin, Win, Cout, ks, stride, ups, use_coef, silu, use_res = case
    if ks == 3 and stride == 1:       # the route query takes these: no Winograd kernel, no split-K
        r = query(descriptor(B, C0, C1, Hin, Win, Cout, ups, Cout if use_res else 0), _lib.CONV_AUTO, 0)
        assert (_lib.CONV_FAMILIES[r.family], r.ksplit) == ('IGEMM', 1), name
    x0, x1, w, bias, coef, res = seeded(name, B, C0, C1, Hin, Win, Cout, ks, stride, ups, use_coef, use_res)
    want = ref_conv(x0, w, bias, x1, stride, ups, coef, silu, res)
    tol = conv_tol(w, C0 + C1)
    got = run_conv(x0, w, bias, x1, stride, ups, coef, silu, res)
    got_d = run_conv(x0, w, bias, x1, stride, ups, coef, silu, res, force_direct=1)
    assert got.shape == want.shape == got_d.shape and bool(torch.isfinite(got).all()) and bool(torch.isfinite(got_d).all())
    e, e_d = (got - want).abs().max().item(), (got_d - want).abs().max().item()
    print('GEOMETRY IGEMM %s default route %.3e direct kernel %.3e bound %.3e' % (name, e, e_d, tol))
    assert e < tol and e_d < tol, (name, e, e_d)


SPLIT_CASES = [
    # name, C0, Cout, Hin, Win, ks, stride   -- B = 2; whole 128-pixel tiles inside an image (conv_split_ok)
    ('split_1x1_16x24', 128, 128, 16, 24, 1, 1),
    ('split_1x1_48x48', 128, 128, 48, 48, 1, 1),
    ('split_3x3_8x48', 64, 128, 8, 48, 3, 1),
    ('split_3x3s2_32x48to16x24', 64, 128, 32, 48, 3, 2),
]


@pytest.mark.parametrize('case', SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_bf16_split_kernel_beyond_squares(case):
    """force_direct = 16 beside the fp32 MFMA kernel (3x3: force_direct = 2, no Winograd) on the inputs of
    test_conv1x1_bf16_split_gemm_is_fp32_grade -- operands over 12 binades with exact zeros and 1e-30 mixed in -- and its two relations,
    K = taps x Cin."""
    name, C0, Cout, Hin, Win, ks, stride = case
    B = 2
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    scale = lambda *s: torch.exp2(torch.randint(-6, 7, s, generator=g).float())
    x0 = torch.randn(B, C0, Hin, Win, generator=g) * scale(B, C0, Hin, Win)
    x0[0, :8, 0, 0] = 0.0
    x0[0, 8:16, 0, 0] = 1e-30
    w = torch.randn(Cout, C0, ks, ks, generator=g) / math.sqrt(C0 * ks * ks) * scale(Cout, C0, ks, ks) / 8
    w[0, :4] = 0.0
    bias = torch.randn(Cout, generator=g)
    want = F.conv2d(x0.double(), w.double(), bias.double(), stride=stride, padding=ks // 2)
    mag = F.conv2d(x0.double().abs(), w.double().abs(), stride=stride, padding=ks // 2).max().item()
    got32 = run_conv(x0, w, bias, None, stride, 0, force_direct=0 if ks == 1 else 2).double()
    got16 = run_conv(x0, w, bias, None, stride, 0, force_direct=16).double()
    assert got16.shape == want.shape and bool(torch.isfinite(got16).all())
    e32, e16 = (got32 - want).abs().max().item(), (got16 - want).abs().max().item()
    K = ks * ks * C0
    print('GEOMETRY SPLIT %s fp32 MFMA %.3e bf16x3 %.3e bounds %.3e %.3e' % (name, e32, e16, 1.5 * e32 + 1.2e-7 * mag, 3e-7 * math.sqrt(K) * mag))
    assert e16 <= 1.5 * e32 + 1.2e-7 * mag, name
    assert e16 < 3e-7 * math.sqrt(K) * mag, name
    assert not torch.equal(got16, got32)          # the split kernel really ran


def test_bf16_split_kernel_statistics_at_48x48():
    """128-pixel statistics rows at W = 48 (a row of partials covers 2 2/3 image rows): the checks of test_gpu_gn_stats.py's partials, on
    O(1) outputs (inputs seeded as in test_conv), which is what the 1e-5 / 1e-5 bounds are stated for."""
    name = 'split_1x1_48x48_stats'
    x0, x1, w, bias, coef, res = seeded(name, 2, 128, 0, 48, 48, 128, 1, 1, 0, True, True)
    plain = run_conv(x0, w, bias, None, 1, 0, coef, False, res, force_direct=16)
    out, buf, px = run_conv(x0, w, bias, None, 1, 0, coef, False, res, force_direct=16, stats=True)
    assert torch.equal(out, plain)
    assert (out - ref_conv(x0, w, bias, None, 1, 0, coef, False, res)).abs().max().item() < conv_tol(w, 128)
    check_partials_of(name, out, buf, px, 128, ROW_SLOTS, (1e-5, 1e-5))


# ---------------------------------------------------------------- 3. GroupNorm coefficients from the tensor
GN_CASES = [
    # name, C0, C1, groups, H, W
    ('gn_32_hw25', 32, 0, 32, 5, 5),              # k_gn_coeffs_v4 has 64 pixel slices for 25 pixels
    ('gn_64_hw36', 64, 0, 32, 6, 6),
    ('gn_64_32_hw100', 64, 32, 32, 10, 10),       # groups of 3 channels: channels 63 | 64, 65 of one group lie on both sides of the split
    ('gn_18_12_hw35', 18, 12, 6, 5, 7),           # the scalar kernel (C0 % 4 != 0), groups of 5 channels: 15 .. 19 straddle the split
]


@pytest.mark.parametrize('case', GN_CASES, ids=[c[0] for c in GN_CASES])
def test_groupnorm_coeffs_at_odd_pixel_counts(case):
    """dlpm_groupnorm_coeffs_f32 -> x A + B against F.group_norm in float64, plain and with a padded scale-shift row + SiLU; sources as
    the case says, also where the plain fixture test passes one."""
    name, C0, C1, groups, H, W = case
    B, Cc = 3, C0 + C1
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(B, Cc, H, W, generator=g) * 1.5 + 0.3
    gam, bet = 1 + 0.2 * torch.randn(Cc, generator=g), 0.2 * torch.randn(Cc, generator=g)
    ss = 0.3 * torch.randn(B, 2 * Cc, generator=g)
    ss_pad = torch.zeros(B, 2 * Cc + 7)
    ss_pad[:, 5:5 + 2 * Cc] = ss
    xd = x.double()
    gn = F.group_norm(xd, groups, gam.double(), bet.double(), 1e-5)
    want_ss = F.silu(gn * (1 + ss[:, :Cc].double()[:, :, None, None]) + ss[:, Cc:].double()[:, :, None, None])
    x0 = nhwc(x[:, :C0]).to(DEV)
    x1 = nhwc(x[:, C0:]).to(DEV) if C1 else None
    gd, bd, ssd = gam.to(DEV), bet.to(DEV), ss_pad.to(DEV)

    def coeffs(with_ss):
        cA, cB = torch.full((B, Cc), float('nan'), device=DEV), torch.full((B, Cc), float('nan'), device=DEV)
        _lib.check(L().dlpm_groupnorm_coeffs_f32(x0.data_ptr(), x1.data_ptr() if C1 else None, C0, C1, B, H * W, groups, gd.data_ptr(),
                                                bd.data_ptr(), ssd.data_ptr() if with_ss else None, 2 * Cc + 7 if with_ss else 0,
                                                5 if with_ss else 0, cA.data_ptr(), cB.data_ptr(), st()))
        torch.cuda.synchronize()
        return cA.cpu().double()[:, :, None, None], cB.cpu().double()[:, :, None, None]
    cA, cB = coeffs(False)
    e_plain = (xd * cA + cB - gn).abs().max().item()
    cA, cB = coeffs(True)
    e_ss = (F.silu(xd * cA + cB) - want_ss).abs().max().item()
    print('GEOMETRY GN %s plain %.3e (bound 3e-6) scale-shift + SiLU %.3e (bound 4e-6)' % (name, e_plain, e_ss))
    assert e_plain < 3e-6 and e_ss < 4e-6, (name, e_plain, e_ss)
