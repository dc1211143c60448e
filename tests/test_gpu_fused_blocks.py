"""The fused whole-block kernels against float64, through the three C entry points dlpm_resblock_small_f32, dlpm_resblock_img_f32 and
dlpm_attnblock_small_f32: k_resblock_small<8 | 4>, k_resblock_wino4_img, k_resblock_wino4_img16, k_attnblock_small<8 | 4>,
k_attnblock16.  References, judge and cases: tests/block_refs.py (checked on the CPU by tests/test_block_refs_cpu.py).

Shapes.  Every concat split the host checks accept is judged (block_refs.RES_SMALL_SPLITS at 8x8 and 4x4, RES_IMG32_SPLITS,
RES_IMG16_SPLITS; attention has 64 channels and 4 heads at 4x4, 8x8, 16x16 and nothing to sweep) or refused (REFUSALS below).  Read
before the first launch, per kernel, for the splits no test or net had launched:
  k_resblock_small     Cin is 64 or 128 whatever the split, so the LDS carve-up, JC = Cin / 16 (a power of two: jc_shift), the fragment
                       counts 9 JC / 2 = 18 | 36 (the ring of 6 divides both) and the [2][Cin] coefficient area are those of the tested
                       shapes; the split enters phase 0 alone, whose float4 quads lie in one source when C0 % 4 == 0, on rows of pitch
                       C0 | C1 floats (16-byte aligned for multiples of 4).  The identity residual is read from the LDS copy of the concat.
  k_resblock_wino4_img   chunks of 8 channels, first = c < C0 per quad: a chunk lies in one source for C0 % 8 == 0; Cf is [2][128],
                       Cin <= 128; the weight stream is nw * (Cin / 8) * 18 fragments as relayout_weight_wino4 lays them out + F4_PAD.
  k_resblock_wino4_img16 chunks of 16 channels, C0 % 16 == 0; Cin / 16 = 2 .. 8 chunks, two 8-channel phases each; otherwise as above.
  The skip convolution of dlpm_resblock_img_f32 is a launch of its own (launch_conv, implicit GEMM: multiples of 32 per source).

Bounds.  ratio = judge(got, want64, ref32, floor64) <= M (block_refs.M_BOUND), M per kernel = twice the largest ratio measured on
MI355X over its benign and sharp cases, and a second M from its cancellation cases (which pass the coefficient-form floor); no M
above block_refs.M_CAP = 8; no benign or sharp ratio is above 4.  Measured ratios (B = 3; the 8x8 | 4x4 size is given where a kernel has two):
  res_small  benign / sharp max 3.160 -> M = 6.32:  64|0@8x8 1.28, 32|32@8x8 2.41, 4|60@8x8 1.76, 64|64@8x8 2.55, 128|0@8x8 2.37, 96|32@8x8 1.86,
      32|96@8x8 1.99, 124|4@8x8 3.16, 64|0@4x4 1.41, 32|32@4x4 1.11, 4|60@4x4 1.10, 64|64@4x4 3.00, 128|0@4x4 1.35, 96|32@4x4 2.69, 32|96@4x4 1.97,
      124|4@4x4 1.53
  res_small  cancellation   max 2.286 -> M = 4.57:  64|0@8x8 gn1 0.89, 64|0@4x4 gn1 1.04, 64|64@8x8 gn1 1.77, 64|64@4x4 gn1 2.22,
      96|32@4x4 gn1 2.29, 64|0@8x8 gn2 0.71, 64|0@4x4 gn2 0.86, 64|64@8x8 gn2 0.58, 64|64@4x4 gn2 0.66, 96|32@4x4 gn2 0.85, 64|0@8x8 out 0.46,
      64|0@4x4 out 0.49, 64|64@8x8 out 0.48, 64|64@4x4 out 0.44, 96|32@4x4 out 0.48
  res_img32  benign / sharp max 2.999 -> M = 6.00:  32|0 2.64, 64|0 2.42, 32|32 1.89, 96|0 1.83, 64|32 1.56, 32|64 3.00, 128|0 2.16, 64|64 1.85,
      96|32 2.03, 32|96 1.61
  res_img32  cancellation   max 1.206 -> M = 2.41:  32|0 gn1 0.86, 32|32 gn1 0.80, 64|32 gn1 1.21, 32|96 gn1 1.14, 32|0 gn2 0.94, 32|32 gn2 0.80,
      64|32 gn2 0.75, 32|96 gn2 0.72, 32|0 out 0.68, 32|32 out 0.68, 64|32 out 0.68, 32|96 out 0.69
  res_img16  benign / sharp max 2.751 -> M = 5.50:  64|0 2.75, 32|0 1.98, 96|0 1.96, 128|0 2.51, 64|32 2.13, 32|64 1.70, 64|64 2.24, 96|32 2.02,
      32|96 1.44
  res_img16  cancellation   max 1.322 -> M = 2.64:  64|0 gn1 1.00, 64|64 gn1 1.29, 64|32 gn1 1.32, 32|64 gn1 1.19, 64|0 gn2 0.91, 64|64 gn2 0.62,
      64|32 gn2 0.89, 32|64 gn2 1.04, 64|0 out 0.43, 64|64 out 0.42, 64|32 out 0.45, 32|64 out 0.45
  attn_small benign / sharp max 0.970 -> M = 1.94:  4x4 0.97, 4x4 sharp 0.95, 8x8 0.74, 8x8 sharp 0.83
  attn_small cancellation   max 1.475 -> M = 2.95:  4x4 gn1 0.81, 8x8 gn1 1.48, 4x4 out 0.13, 8x8 out 0.12
  attn16     benign / sharp max 0.844 -> M = 1.69:  benign 0.84, sharp 0.83
  attn16     cancellation   max 0.860 -> M = 1.72:  gn1 0.86, out 0.10

Statistics.  Judged against float64 of the kernel's own output by test_gpu_gn_stats.check_partials_of (one partial per image, or
four 16x16 quadrants at 32x32): 1e-5 / 1e-5, 2e-4 / 2e-4 in the cancel_out and cancel_gn1 cases (in both the OUTPUT has |mean| >= 100:
cancel_gn1's x = 100 + .. passes through the skip path); and |M2 - want| <= 2e-4 want where want < 1, which the 1 + want denominator
would hide (measured: at most 3.14e-05, res_img16_64_0_h16_cancel_out; 15 cases have such partials).
(The floor of a cancellation case moves with the float64 summation order of the CPU that computes it -- A and B are rounded to fp32 at
|B| ~ 1000, so the last float64 bit decides an fp32 half-ulp of 6e-5: 0.9e-4 and 1.6e-4 were seen for one case on two machines.  It
enters a ratio only where it exceeds the fp32 oracle's error.)

In the net.  The `mnist` net at B = 2 on the default route against the oracle's float64 forward, per feature
ratio_i = |hip - fp64| / |fp32 oracle - fp64|; bound: twice the largest measured.  Measured (down 0 .. 11, middle, up 0 .. 11, out):
  1.02 2.36 2.45 1.60 1.80 1.84 2.27 1.58 2.33 1.80 1.78 1.74 | 1.79 | 1.94 1.65 1.96 2.33 1.50 2.58 1.94 2.29 1.96 2.13 2.09 2.48 | 2.78
  largest 2.777 (out) -> bound 5.55; largest step between consecutive features 1.34 (down 0 -> down 1), far from the cap of 8 a single block has.
"""
import ctypes as C
import functools

import pytest
import torch

import block_refs as R
import small_block_weights as sbw
from dlpm_amd import _lib
from test_gpu_gn_stats import BLK, ROWS, check_partials_of
from test_gpu_kernels import DEV, nchw, nhwc

pytestmark = pytest.mark.gpu

GUARD = 64                     # floats on either side of a guarded buffer (256 bytes: the inner part keeps float4 alignment)
SENTINEL = -777.25
NET_RATIO_BOUND = 2 * 2.777      # twice the largest measured ratio (out)


# ---------------------------------------------------------------------------------------------------------------- launch helpers
def guarded(n):
    """(whole buffer, inner view of n floats): NaN inside, SENTINEL in the guard words on both sides."""
    full = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    inner = full[GUARD:GUARD + n]
    inner.fill_(float('nan'))
    return full, inner


def guards_intact(full):
    return bool((full[:GUARD] == SENTINEL).all()) and bool((full[-GUARD:] == SENTINEL).all())


def res_scratch_floats(kernel, B, cin, skip):
    if kernel == 'res_small':
        return 64 * cin * 9 + 64 * 64 * 9 + (64 * cin if skip else 0)
    return _lib.lib().dlpm_resblock_img_scratch_floats(B, cin)


def launch_res(kernel, sd, x, ss, c0, c1, with_stats=True, ss_stride=None, scratch_delta=0, skip='auto', x1_null=False):
    """One launch of dlpm_resblock_small_f32 / dlpm_resblock_img_f32 on NaN-prefilled, guarded buffers.  x: [B, C0 + C1, H, H] (split
    into two NHWC tensors when C1 > 0); ss: [B, 2 Cout] rows, padded with NaN to ss_stride.  Returns the status and the buffers."""
    L, st = _lib.lib(), _lib.stream_ptr()
    B, cin, hs = x.shape[0], x.shape[1], x.shape[2]
    co = R.cout_of(kernel)
    xh = nhwc(x).to(DEV)
    x0 = xh[..., :c0].contiguous()
    x1 = xh[..., c0:].contiguous() if c1 else None
    w = {k: v.to(DEV).contiguous() for k, v in sd.items()}
    stride = ss_stride or 2 * co
    ssd = torch.full((B, stride), float('nan'), device=DEV)
    ssd[:, :2 * co] = ss.to(DEV)
    a = _lib.ResBlockArgs()
    a.x0, a.x1, a.C0, a.C1 = x0.data_ptr(), (x1.data_ptr() if c1 and not x1_null else None), c0, c1
    a.B, a.H, a.W = B, hs, hs
    a.gn1_w, a.gn1_b = w['in_layers.0.weight'].data_ptr(), w['in_layers.0.bias'].data_ptr()
    a.conv1_w, a.conv1_b = w['in_layers.2.weight'].data_ptr(), w['in_layers.2.bias'].data_ptr()
    a.ss, a.ss_stride = ssd.data_ptr(), stride
    a.gn2_w, a.gn2_b = w['out_layers.0.weight'].data_ptr(), w['out_layers.0.bias'].data_ptr()
    a.conv2_w, a.conv2_b = w['out_layers.3.weight'].data_ptr(), w['out_layers.3.bias'].data_ptr()
    use_skip = ('skip_connection.weight' in w) if skip == 'auto' else skip
    if use_skip:
        a.skip_w, a.skip_b = w['skip_connection.weight'].data_ptr(), w['skip_connection.bias'].data_ptr()
    out_full, out = guarded(B * hs * hs * co)
    nstat = 2 * B * co * (4 if kernel == 'res_img32' else 1)
    st_full, stats = guarded(nstat)
    a.out, a.stats_out = out.data_ptr(), (stats.data_ptr() if with_stats else None)
    n = res_scratch_floats(kernel, B, cin, use_skip) + scratch_delta
    sc_full, scratch = guarded(n)
    fn = L.dlpm_resblock_small_f32 if kernel == 'res_small' else L.dlpm_resblock_img_f32
    rc = fn(C.byref(a), scratch.data_ptr(), n, st)
    torch.cuda.synchronize()
    return dict(rc=rc, out=out.cpu(), stats=stats.cpu(), scratch=scratch.cpu(), shape=(B, hs, hs, co),
                guards=guards_intact(out_full) and guards_intact(st_full) and guards_intact(sc_full))


def launch_attn(sd, x, with_stats=True, C_=64, heads=4, scratch_delta=0):
    """One launch of dlpm_attnblock_small_f32 (k_attnblock_small at 4x4 / 8x8, k_attnblock16 at 16x16), buffers as in launch_res."""
    L, st = _lib.lib(), _lib.stream_ptr()
    B, hs = x.shape[0], x.shape[2]
    xh = nhwc(x).to(DEV).contiguous()
    w = {k: v.to(DEV).contiguous() for k, v in sd.items()}
    a = _lib.AttnBlockArgs()
    a.x, a.C, a.heads, a.B, a.H, a.W = xh.data_ptr(), C_, heads, B, hs, hs
    a.gn_w, a.gn_b = w['norm.weight'].data_ptr(), w['norm.bias'].data_ptr()
    a.qkv_w, a.qkv_b = w['qkv.weight'].data_ptr(), w['qkv.bias'].data_ptr()
    a.proj_w, a.proj_b = w['proj_out.weight'].data_ptr(), w['proj_out.bias'].data_ptr()
    out_full, out = guarded(B * hs * hs * C_)
    st_full, stats = guarded(2 * B * C_)
    a.out, a.stats_out = out.data_ptr(), (stats.data_ptr() if with_stats else None)
    n = 4 * C_ * C_ + scratch_delta
    sc_full, scratch = guarded(n)
    rc = L.dlpm_attnblock_small_f32(C.byref(a), scratch.data_ptr(), n, st)
    torch.cuda.synchronize()
    return dict(rc=rc, out=out.cpu(), stats=stats.cpu(), scratch=scratch.cpu(), shape=(B, hs, hs, C_),
                guards=guards_intact(out_full) and guards_intact(st_full) and guards_intact(sc_full))


def image(r):
    """The NCHW output of a launch that succeeded."""
    _lib.check(r['rc'])
    assert r['guards'], 'a guard word beside the output, the statistics or the scratch was overwritten'
    return nchw(r['out'].view(*r['shape']))


def launch_case(c, sd=None, x=None, ss=None, **kw):
    sd = sd if sd is not None else c.sd
    x = x if x is not None else c.x
    if c.is_res:
        return launch_res(c.kernel, sd, x, ss if ss is not None else c.ss, c.c0, c.c1, **kw)
    return launch_attn(sd, x, **kw)


# ---------------------------------------------------------------------------------------------------------------- judged cases
# one case per kernel runs with a row pitch that is not the row length
PADDED_SS = {'res_small_96_32_h8_benign', 'res_small_4_60_h4_benign', 'res_img32_32_64_h32_benign', 'res_img16_96_32_h16_benign',
             'res_small_64_64_h8_cancel_gn2', 'res_img32_32_96_h32_cancel_gn2', 'res_img16_32_64_h16_cancel_gn2'}
assert PADDED_SS <= set(R.CASES)


def small_m2_error(out, stats, quadrants):
    """max |M2 - want| / want over the partials whose float64 M2 of the kernel's own output is below 1 (None if there are none)."""
    o = out.double()
    B, Cc, H, W = o.shape
    if quadrants:
        pix = o.reshape(B, Cc, 2, 16, 2, 16).permute(0, 2, 4, 1, 3, 5).reshape(B, 4, Cc, 256)
        part = stats.view(B, 4, Cc, 2).double()
    else:
        pix = o.reshape(B, 1, Cc, H * W)
        part = stats.view(B, 1, Cc, 2).double()
    want = ((pix - pix.mean(-1, keepdim=True)) ** 2).sum(-1)
    sel = want < 1
    if not bool(sel.any()):
        return None
    return ((part[..., 1] - want).abs() / want)[sel].max().item()


def check_case(name):
    c = R.case(name)
    kw = {'ss_stride': 2 * c.cout + 12} if name in PADDED_SS else {}
    r = launch_case(c, **kw)
    got = image(r)
    assert bool(torch.isfinite(got).all()), '%s: non-finite output' % name
    ratio = R.ratio(name, got)
    want, ref32, floor = R.refs(name)
    M = R.M_BOUND[c.kernel][1 if c.kind.startswith('cancel_') else 0]
    print('RATIO %s %.3f (bound %.2f)  err %.3g  e32 %.3g  floor %.3g' % (
        name, ratio, M, (got.double() - want).abs().max().item(), (ref32.double() - want).abs().max().item(),
        (floor - want).abs().max().item() if floor is not None else 0.0))
    # statistics: of the kernel's own output; exactly the slots of this launch are written
    quadrants = c.kernel == 'res_img32'
    # (cancel_gn1 as cancel_out: x = 100 + .. reaches the output through the skip path, |out| = 100 .. 320, where half an ulp of a mean
    # is already 4e-6 .. 1.5e-5 -- 1e-5 is below what fp32 can hold; measured 1.04e-5 at res_small_64_0_h8_cancel_gn1)
    bounds = (2e-4, 2e-4) if c.kind in ('cancel_out', 'cancel_gn1') else (1e-5, 1e-5)
    px = 256 if quadrants else c.hs * c.hs
    check_partials_of(name, got, r['stats'], px, px, BLK(16, 16) if quadrants else ROWS, bounds)
    e_small = small_m2_error(got, r['stats'], quadrants)
    print('SMALLM2 %s %s' % (name, 'none below 1' if e_small is None else '%.3g' % e_small))
    # without statistics: the same bits, and the statistics buffer untouched
    r0 = launch_case(c, with_stats=False, **kw)
    assert torch.equal(image(r0), got), '%s: the launch without statistics wrote another output' % name
    assert bool(torch.isnan(r0['stats']).all())
    # a sample's bits do not depend on its batch
    for i in range(R.BATCH):
        one = launch_case(c, x=c.x[i:i + 1], ss=c.ss[i:i + 1] if c.is_res else None, **kw)
        assert torch.equal(image(one)[0], got[i]), '%s: image %d alone has other bits than in the batch of %d' % (name, i, R.BATCH)
    assert ratio <= M <= R.M_CAP, (name, ratio, M)
    assert e_small is None or e_small <= 2e-4, (name, e_small)


@pytest.mark.parametrize('name', R.BENIGN)
def test_block_against_float64(name):
    """Benign and sharp cases at B = 3: finite, within M of float64 in units of the fp32 oracle's own error; statistics; the same
    bits without statistics; nothing outside the buffers; the B = 1 launches give the batch's bits."""
    check_case(name)


@pytest.mark.parametrize('name', R.CANCEL)
def test_block_against_float64_under_cancellation(name):
    """|mean| >> std in front of GroupNorm-1 (cancel_gn1), GroupNorm-2 (cancel_gn2) or in the output whose statistics the block
    emits (cancel_out): the same checks, the bound includes the coefficient-form floor."""
    check_case(name)


# ---------------------------------------------------------------------------------------------------------------- exact properties
ZERO_TAIL = [n for n in R.BENIGN if R.CASES[n][0].startswith('attn') or R.CASES[n][1] + R.CASES[n][2] == R.cout_of(R.CASES[n][0])]


@pytest.mark.parametrize('name', ZERO_TAIL)
def test_zero_last_layer_returns_the_input_bit_for_bit(name):
    """proj_out = 0 (the reference's own initialisation; sharp cases included), or out_layers.3 = 0 under the identity skip: out is x."""
    c = R.case(name)
    last = 'out_layers.3' if c.is_res else 'proj_out'
    sd = c.with_sd({last + '.weight': torch.zeros_like(c.sd[last + '.weight']), last + '.bias': torch.zeros_like(c.sd[last + '.bias'])})
    assert torch.equal(image(launch_case(c, sd=sd)), c.x), name


# ---------------------------------------------------------------------------------------------------------------- refusals
def _res_refusal(kernel, c0, c1, hs, **kw):
    name = R._name(kernel, c0, c1, hs, 'benign')
    co = R.cout_of(kernel)
    s = R._seed('refusal_' + name)
    sd = sbw._draw(sbw._shapes_res(c0 + c1, 128, co), sbw.RES_KEYS, s)
    if c0 + c1 == co and kw.get('skip') is True:      # skip weights where the block has none of its own
        sd['skip_connection.weight'], sd['skip_connection.bias'] = R._randn((co, c0 + c1, 1, 1), s + 5), R._randn((co,), s + 6)
    x = sbw.seeded_input((2, c0 + c1, hs, hs), s + 1)
    return launch_res(kernel, sd, x, R._randn((2, 2 * co), s + 2), c0, c1, **kw)


def _attn_refusal(C_, heads):
    s = R._seed('refusal_attn_%d_%d' % (C_, heads))
    sd = sbw._draw(sbw._shapes_attn(C_), sbw.ATTN_KEYS, s)
    return launch_attn(sd, sbw.seeded_input((2, C_, 8, 8), s + 1), C_=C_, heads=heads)      # (every buffer sized for the refused shape)


# name -> (launch, expected status, a word of the message).  Every one is a host-side argument check read in unet.hip /
# block_small.hip / conv_wino4.hip, in front of the first launch of the entry point.
REFUSALS = {
    'img32_40_24_skip_needs_multiples_of_32': (lambda: _res_refusal('res_img32', 40, 24, 32), -1, 'multiples of 32'),
    'img16_32_32_without_skip_weights': (lambda: _res_refusal('res_img16', 32, 32, 16), -1, 'concat input'),
    'img16_32_32_with_skip_weights': (lambda: _res_refusal('res_img16', 32, 32, 16, skip=True), -1, 'skip_w'),
    'img32_x1_null': (lambda: _res_refusal('res_img32', 32, 32, 32, x1_null=True), -1, 'x1/C1'),
    'small_x1_null': (lambda: _res_refusal('res_small', 64, 64, 8, x1_null=True), -1, 'x1/C1'),
    'img16_scratch_one_short': (lambda: _res_refusal('res_img16', 64, 32, 16, scratch_delta=-1), -1, 'scratch'),
    'img32_scratch_one_short': (lambda: _res_refusal('res_img32', 32, 0, 32, scratch_delta=-1), -1, 'scratch'),
    'small_scratch_one_short': (lambda: _res_refusal('res_small', 64, 64, 4, scratch_delta=-1), -1, 'scratch'),
    'small_cin_96': (lambda: _res_refusal('res_small', 64, 32, 8, skip=True), -1, '96 input channels'),
    'small_62_2': (lambda: _res_refusal('res_small', 62, 2, 8), -3, '62 + 2'),
    'small_64_with_skip_weights': (lambda: _res_refusal('res_small', 64, 0, 4, skip=True), -3, 'with skip_w'),
    'small_128_without_skip_weights': (lambda: _res_refusal('res_small', 64, 64, 4, skip=False), -3, 'without skip_w'),
    'attn_128_channels': (lambda: _attn_refusal(128, 4), -1, '64 channels, 4 heads'),
    'attn_8_heads': (lambda: _attn_refusal(64, 8), -1, '64 channels, 4 heads'),
    'attn_scratch_one_short': (lambda: launch_attn(R.case('attn_small_64_0_h8_benign').sd, R.case('attn_small_64_0_h8_benign').x,
                                                   scratch_delta=-1), -1, 'scratch'),
}


@pytest.mark.parametrize('name', list(REFUSALS))
def test_refusals(name):
    """An error status, dlpm_last_error set, and nothing written: output, statistics and scratch keep their NaN, the guards their words."""
    fn, status, word = REFUSALS[name]
    r = fn()
    msg = _lib.lib().dlpm_last_error().decode('utf-8', 'replace')
    print(name, r['rc'], msg)
    assert r['rc'] == status, (name, r['rc'], msg)
    assert word in msg, (name, msg)
    assert r['guards'] and bool(torch.isnan(r['out']).all()) and bool(torch.isnan(r['stats']).all()) and bool(torch.isnan(r['scratch']).all())


# ---------------------------------------------------------------------------------------------------------------- in the net
@functools.lru_cache(maxsize=None)
def net_ratios():
    net, sd, x, t = R.net_case()
    f32, f64 = R.net_forwards(sd, x, t)
    with torch.no_grad():
        feats = net.get_feature_vectors(x.to(DEV), t.to(DEV))
        y = net(x.to(DEV), t.to(DEV))
    got = R.flat_feats(y, feats)
    assert [n for n, _ in got] == [n for n, _ in f64]
    rows = []
    for (n, g), (_, a), (_, w) in zip(got, f32, f64):
        g = g.detach().cpu().double()
        assert g.shape == w.shape and bool(torch.isfinite(g).all()), n
        err, e32 = (g - w).abs().max().item(), (a.double() - w).abs().max().item()
        rows.append((n, err / e32, err, e32))
    return rows


def test_every_feature_of_the_mnist_net_against_float64():
    """GroupNorm-1 from the producers' statistics partials, emb_off != 0 and the quadrant statistics a next block consumes are
    reachable only here: every feature of get_feature_vectors and the output against the float64 forward, in units of the fp32
    oracle's own distance from it."""
    rows = net_ratios()
    for n, r, err, e32 in rows:
        print('NETRATIO %-8s %.3f  err %.3g  e32 %.3g' % (n, r, err, e32))
    assert len(rows) == 26
    jumps = [rows[i + 1][1] - rows[i][1] for i in range(len(rows) - 1)]
    assert max(jumps) <= R.M_CAP, 'the ratio jumps by %.2f between %s and %s' % (max(jumps), rows[jumps.index(max(jumps))][0], rows[jumps.index(max(jumps)) + 1][0])
    bad = [i for i, row in enumerate(rows) if row[1] > NET_RATIO_BOUND]
    assert not bad, 'first feature whose ratio leaves the bound %.2f: %s (index %d of %d), ratio %.3f' % (
        NET_RATIO_BOUND, rows[bad[0]][0], bad[0], len(rows), rows[bad[0]][1])
