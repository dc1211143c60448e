"""The convolution launches that exist only under a declared dispatch batch, one launch at a time against float64
(dlpm_conv_policy_f32, include/dlpm_amd_conv.h): the split-K grid copies of k_conv3x3_wino_q and of the 32-channel F(4x4) n-tiles with
launch_splitk_reduce behind them, and the 64- / 32-channel n-tiles of a Cout % 128 == 0 layer.  dlpm_conv2d_f32 declares nothing, so the
kernel tests of test_gpu_kernels.py cannot reach them; before this file they ran only inside whole nets, 60 layers from the assert.

Cases and their routes: tests/conv_policy_cases.py (tests/test_conv_policy_cpu.py pins the routes and what the table covers).  Every
launch here asserts the route it TOOK (family, n-tile, images per block, S) before anything else is looked at: no test passes on
another kernel.  Inputs are seeded as in test_conv: w ~ randn / sqrt(9 Cin), coefficients 1 + 0.3 randn and 0.3 randn per image and
channel, reference = ref_conv in float64.

Bounds.  F(2x2) family: conv_tol(w, Cin), test_conv's.  F(4x4) family: min(2e-5, 2 x POLICY_MEASURED[case]), the convention of
F4_MEASURED.  Each partial output part[s] is held to the bound of its case against the float64 convolution of its own channel slice
(coefficients, SiLU and upsampling applied to the slice; no bias, no residual): a slice sums fewer terms than the whole, and errors
cannot cancel across grid copies there."""
import ctypes as C
import functools
import math

import pytest
import torch

from conv_policy_cases import BY_NAME, CASES, NARROW, SPLIT, out_size, route_tuple, slices
from dlpm_amd import _lib
from test_gpu_gn_stats import BLK, check_partials_of
from test_gpu_kernels import DEV, L, conv_tol, nchw, nhwc, ref_conv, st

pytestmark = pytest.mark.gpu

# max |out - fp64 reference| of the F(4x4)-family cases, measured on MI355X at the commit that added this file (the split-K cases: the
# reduced output; each is under 1e-5).  The bound of a case is twice its figure, never above 2e-5.
POLICY_MEASURED = {'f4_16x16_32_32to32_d64_coef_res': 2.742e-06,
                   'f4_8x16_128_128to32_d64': 3.159e-06,
                   'f4_8x16_128_128to96_d2': 3.576e-06,
                   'f4_ups2to4_256_128to96_d256': 4.340e-06,
                   'f4_ups4to8_32_32to96_d64_coef': 3.457e-06,
                   'f4_ups8to16_128_128to32_d2_rescat': 3.099e-06,
                   'nq32_16x16_32to128_d64': 3.278e-06,
                   'nq64_16x16_32to128_d128': 5.722e-06,
                   'nq64_16x16_32to256_d64': 3.234e-06}
# (the F(2x2) cases measured 0.5 - 1.4e-6 against conv_tol = 0.7 - 1.8e-4; the largest partial of any F(4x4) case 3.40e-6)

CANARY = 4096         # floats behind the partial buffer and behind the output that must stay untouched
SENTINEL = -12345.0


def make(name, B=None):
    """Seeded cpu inputs of a case (NCHW), optionally at another batch"""
    return make_of(BY_NAME[name], B)


def make_of(c, B=None):
    """... of any Case (tests/test_gpu_conv_geometry.py brings its own table)"""
    name = c.name
    B = B or c.B
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    Cin = c.C0 + c.C1
    Ho, Wo = out_size(c)
    x0 = torch.randn(B, c.C0, c.Hin, c.Win, generator=g)
    x1 = torch.randn(B, c.C1, c.Hin, c.Win, generator=g) if c.C1 else None
    w = torch.randn(c.Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    bias = torch.randn(c.Cout, generator=g)
    coef = (1 + 0.3 * torch.randn(B, Cin, generator=g), 0.3 * torch.randn(B, Cin, generator=g)) if c.act else None
    res = torch.randn(B, c.Cout, Ho, Wo, generator=g) if c.res is not None else None
    return dict(x0=x0, x1=x1, w=w, bias=bias if c.bias else None, coef=coef, res=res)


def pick(inp, sl):
    """the same inputs, images `sl` only"""
    cut = lambda t: None if t is None else t[sl].contiguous()
    return dict(inp, x0=cut(inp['x0']), x1=cut(inp['x1']), res=cut(inp['res']),
                coef=None if inp['coef'] is None else (cut(inp['coef'][0]), cut(inp['coef'][1])))


def launch(c, inp, gen=_lib.CONV_AUTO, d=None, stats=False, want_route=None, short_partial=0):
    """One dlpm_conv_policy_f32 launch of case c's layer on `inp` under (gen, d).  The partial buffer holds exactly the floats the route
    asks for, the output exactly B Hout Wout Cout; both are NaN-prefilled with CANARY sentinel floats behind them.  Asserts the route
    taken.  Returns dict(out NCHW cpu, part [S][B][H][W][Cout] cpu or None, route, canaries intact, stats buffer, stats px)."""
    d = c.d if d is None else d
    x0, x1, w = inp['x0'], inp['x1'], inp['w']
    B = x0.shape[0]
    Ho, Wo = out_size(c)
    a = _lib.ConvArgs()
    keep = []

    def dev(t):
        t = t.to(DEV).contiguous()
        keep.append(t)
        return t.data_ptr()
    a.src0, a.C0 = dev(nhwc(x0)), c.C0
    if x1 is not None:
        a.src1, a.C1 = dev(nhwc(x1)), c.C1
    a.B, a.Hin, a.Win, a.Hout, a.Wout = B, c.Hin, c.Win, Ho, Wo
    a.ksize, a.stride, a.upsample, a.Cout = 3, 1, c.ups, c.Cout
    a.weight = dev(w)
    if inp['bias'] is not None:
        a.bias = dev(inp['bias'])
    if inp['coef'] is not None:
        a.coefA, a.coefB = dev(inp['coef'][0]), dev(inp['coef'][1])
    a.act_silu = int(c.act)
    if inp['res'] is not None:
        if c.res == 'one':
            a.res0, a.R0 = dev(nhwc(inp['res'])), c.Cout
        else:
            a.res0, a.res1, a.R0 = dev(nhwc(inp['res'][:, :c.res])), dev(nhwc(inp['res'][:, c.res:])), c.res
    need = _lib.ConvRoute()
    _lib.check(L().dlpm_conv_policy_route(C.byref(a), gen, d, C.byref(need)))
    if want_route is None:
        want_route = (c.family, c.nq, c.nimg, c.ksplit)
    # (family, nq, nimg, ksplit), or those and (bh, bw, stats_px) behind them
    route_of = lambda r: (route_tuple(r) + (r.bh, r.bw, r.stats_px))[:max(4, len(want_route))]
    assert route_of(need) == want_route, (c.name, route_of(need), want_route)
    S, n_out = need.ksplit, B * Ho * Wo * c.Cout
    assert need.partial_floats == (S * n_out if S > 1 else 0)
    scratch = torch.empty(need.scratch_floats, device=DEV)
    a.scratch_floats = scratch.numel()

    def guarded(n):
        t = torch.full((n + CANARY,), float('nan'), device=DEV)
        t[n:] = SENTINEL
        return t
    out, part = guarded(n_out), guarded(need.partial_floats)
    a.out = out.data_ptr()
    nst = 2 * B * max(1, Ho * Wo // 64) * c.Cout
    sbuf = torch.full((nst,), float('nan'), device=DEV) if stats else None
    px = C.c_int32(-1)
    took = _lib.ConvRoute()
    rc = L().dlpm_conv_policy_f32(C.byref(a), gen, d, scratch.data_ptr(), part.data_ptr() if S > 1 else None,
                                  need.partial_floats - short_partial, sbuf.data_ptr() if stats else None, C.byref(px) if stats else None,
                                  C.byref(took), st())
    torch.cuda.synchronize()
    if rc != 0:
        return dict(rc=rc, untouched=bool(torch.isnan(out[:n_out]).all()) and bool(torch.isnan(part[:need.partial_floats]).all()) and
                    (sbuf is None or bool(torch.isnan(sbuf).all())) and px.value == -1)
    assert route_of(took) == want_route and (took.bh, took.bw, took.stats_px, took.grid) == (need.bh, need.bw, need.stats_px, need.grid)
    intact = bool((out[n_out:] == SENTINEL).all()) and bool((part[need.partial_floats:] == SENTINEL).all())
    return dict(rc=0, out=nchw(out[:n_out].view(B, Ho, Wo, c.Cout)).cpu(),
                part=part[:need.partial_floats].view(S, B, Ho, Wo, c.Cout).cpu() if S > 1 else None,
                route=took, intact=intact, stats=sbuf.cpu() if stats else None, px=px.value)


@functools.lru_cache(maxsize=None)
def produce(name):
    """One launch per case, shared by the tests and never modified"""
    return launch(BY_NAME[name], make(name))


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 convolution of the whole case (returned in fp32, as ref_conv does)"""
    c, i = BY_NAME[name], make(name)
    return ref_conv(i['x0'], i['w'], i['bias'], i['x1'], 1, c.ups, i['coef'], c.act, i['res'])


def bound(name):
    c, i = BY_NAME[name], make(name)
    if c.family == 'WINO':
        return conv_tol(i['w'], c.C0 + c.C1)
    assert name in POLICY_MEASURED, '%s: no measured error recorded in POLICY_MEASURED' % name
    return min(2e-5, 2 * POLICY_MEASURED[name])


IDS = [c.name for c in CASES]
SPLIT_IDS = [c.name for c in SPLIT]


@pytest.mark.parametrize('name', IDS)
def test_output_against_fp64(name):
    got, want = produce(name)['out'], reference(name)
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    err = (got - want).abs().max().item()
    print('%s: max |out - fp64| %.3e' % (name, err))
    print('%s: bound %.3e' % (name, bound(name)))
    assert err < bound(name), (name, err)


@pytest.mark.parametrize('name', SPLIT_IDS)
def test_each_partial_against_fp64_of_its_channel_slice(name):
    """part[s] = the convolution of input channels [s Cin / S, (s + 1) Cin / S) alone: a grid copy that starts its coefficients, its
    weight stream or its concat source at the wrong channel is wrong HERE, whatever the other copies do."""
    c, i = BY_NAME[name], make(name)
    part = produce(name)['part']
    assert part.shape[0] == c.ksplit and bool(torch.isfinite(part).all())
    x = i['x0'] if i['x1'] is None else torch.cat([i['x0'], i['x1']], 1)
    errs = []
    for s, (lo, hi) in enumerate(slices(c)):
        coef = None if i['coef'] is None else (i['coef'][0][:, lo:hi], i['coef'][1][:, lo:hi])
        want = ref_conv(x[:, lo:hi], i['w'][:, lo:hi], None, None, 1, c.ups, coef, c.act, None)
        errs.append((nchw(part[s]) - want).abs().max().item())
    print('%s: max |part[s] - fp64 of its slice| %s' % (name, ' '.join('%.3e' % e for e in errs)))
    print('%s: bound %.3e' % (name, bound(name)))
    assert max(errs) < bound(name), (name, errs)


@pytest.mark.parametrize('name', SPLIT_IDS)
def test_reduction_is_the_fixed_order_sum_bit_for_bit(name):
    """out == ((p0 + p1) + p2 ...) + bias + residual in fp32, in that order (additions only: nothing to contract).  The table holds
    launches without bias, without residual, with one residual tensor and with a residual concat at R0."""
    c, i = BY_NAME[name], make(name)
    r = produce(name)
    acc = r['part'][0].clone()
    for s in range(1, c.ksplit):
        acc = acc + r['part'][s]
    if i['bias'] is not None:
        acc = acc + i['bias'].view(1, 1, 1, -1)
    if i['res'] is not None:
        acc = acc + nhwc(i['res'])
    assert torch.equal(nchw(acc), r['out']), (name, (nchw(acc) - r['out']).abs().max().item())


@pytest.mark.parametrize('name', IDS)
def test_nothing_is_written_outside_the_buffers(name):
    """The partial buffer is exactly S B Hout Wout Cout floats, the output exactly B Hout Wout Cout; the floats behind both stay what they
    were, also where the last multi-image block has a batch tail (B = 5 / 19 against 2, 4, 8, 16 images per block) -- and every float
    inside is written."""
    r = produce(name)
    assert r['intact'], name
    assert bool(torch.isfinite(r['out']).all()) and (r['part'] is None or bool(torch.isfinite(r['part']).all()))


INDEPENDENT = [c.name for c in CASES if c.nimg == 1] + ['f4_8x16_128_128to32_d64']


@pytest.mark.parametrize('name', INDEPENDENT)
def test_the_declaration_decides_not_the_call(name):
    """Image i of a B = 5 call has the bits of the same image run alone under the same declaration (same route, asserted by launch):
    every case with one image per block, and one with two (each image then sits alone in a block with a tail)."""
    c, i5 = BY_NAME[name], make(name, 5)
    whole = launch(c, i5)
    assert whole['intact']
    for k in range(5):
        alone = launch(c, pick(i5, slice(k, k + 1)))
        assert alone['intact'] and torch.equal(alone['out'][0], whole['out'][k]), (name, k)
        if c.ksplit > 1:
            assert torch.equal(alone['part'][:, 0], whole['part'][:, k]), (name, k)


@pytest.mark.parametrize('name', [c.name for c in NARROW])
def test_narrow_n_tiles_give_the_wide_kernels_bits(name):
    """wino4_nq_for's claim: a Cout % 128 == 0 layer on 64- / 32-channel n-tiles under a declaration has the bits of the 128-channel
    n-tile it takes without one (generation F4, nothing declared).  (Against float64: test_output_against_fp64.)"""
    c = BY_NAME[name]
    wide = launch(c, make(name), gen=_lib.CONV_F4, d=0, want_route=('WINO4', 128, 1, 1))
    assert wide['intact'] and torch.equal(wide['out'], produce(name)['out']), (name, (wide['out'] - produce(name)['out']).abs().max().item())


@pytest.mark.parametrize('name', SPLIT_IDS)
def test_split_k_refuses_statistics_and_short_buffers(name):
    """DLPM_ERR_UNSUPPORTED for statistics asked of a split-K route, DLPM_ERR_NOMEM for a partial buffer one float short: nothing is
    written -- not the output, not the partial buffer, not the statistics."""
    c = BY_NAME[name]
    r = launch(c, make(name), stats=True)
    assert r['rc'] == -3 and r['untouched'], r
    r = launch(c, make(name), short_partial=1)
    assert r['rc'] == -5 and r['untouched'], r


def test_narrow_n_tile_statistics_against_fp64():
    """Cout = 128 on 32-channel n-tiles (16x16): the statistics partials four workgroups write per block, under the checks
    test_gpu_gn_stats.py applies to every other kernel (bounds 1e-5 / 1e-5), and the output of the launch without statistics."""
    name = 'nq32_16x16_32to128_d64'
    r = launch(BY_NAME[name], make(name), stats=True)
    assert r['rc'] == 0 and r['intact'] and torch.equal(r['out'], produce(name)['out'])
    check_partials_of(name, r['out'], r['stats'], r['px'], 256, BLK(16, 16), (1e-5, 1e-5))
