"""Every tile shape the halo, head and stem convolution kernels admit, one dlpm_conv2d_f32 launch at a time against float64.

tests/conv_tile_cases.py holds one row per class -- halo (ups, Wout, th, nimg), head (family, Wout, tile rows), stem (kernel, Wout, rows
per block) -- on the smallest image that reaches it, and the seam rows (images of 3 and 5 tiles, blocks that span images, a ragged last
block); tests/test_conv_tile_cases_cpu.py pins their routes and the coverage.  Per row:
  the kernel taken: the launch runs under dlpm_prof_enable(1) and the row's profiler classes must be what dlpm_prof_report lists;
  canaries: the output is NaN-prefilled; a strip of NaN stands before and after the output, every input, residual and coefficient
  buffer, and behind the scratch; afterwards every strip has its bits and every output element is finite;
  against float64 (ref_conv): halo and head rows under conv_tol(w, Cin); the one-pass head in both its forms, and its bf16 x 3 form
  under e <= 1.5 e_fp32 + 1e-7 (test_head_conv_as_gemm_plus_gather's relation); stems under 1e-5 with the inputs of
  test_stem_conv_kernels;
  where a tile or a workgroup's walk spans images (nimg > 1; the persistent gather and one-pass head kernels; the 1024-pixel blocks of
  k_conv_stem_regw): image 0 of the launch has the bits of a B = 1 launch of image 0 alone;
  a k_conv3x3_halo row: the weight-streaming kernel and the direct kernel on the same inputs pass the bound too, and the two halo
  kernels agree bit for bit (both accumulate tap by tap, k-group by k-group, chunk by chunk into the same MFMA accumulators)."""
import ctypes as C
import functools
import math

import pytest
import torch

import conv_tile_cases as T
from dlpm_amd import _lib
from test_gpu_kernels import DEV, L, conv_tol, nchw, nhwc, ref_conv, st

pytestmark = pytest.mark.gpu
CAN = 1024                    # floats of each canary strip
NAN_BITS = 0x7fc00000


def inputs_name(r):
    return r.twin or r.name


@functools.lru_cache(maxsize=None)
def make(name):
    """Seeded cpu inputs of a row (NCHW): as test_conv draws them; a stem's as test_stem_conv_kernels (image x 2)"""
    r = T.BY_NAME[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    Cin = r.C0 + r.C1
    Ho, Wo = T.out_size(r)
    x0 = torch.randn(r.B, r.C0, r.Hin, r.Win, generator=g) * (2 if r.kernel.startswith('stem') else 1)
    x1 = torch.randn(r.B, r.C1, r.Hin, r.Win, generator=g) if r.C1 else None
    w = torch.randn(r.Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    bias = torch.randn(r.Cout, generator=g)
    coef = (1 + 0.3 * torch.randn(r.B, Cin, generator=g), 0.3 * torch.randn(r.B, Cin, generator=g)) if r.act else None
    res = torch.randn(r.B, r.Cout, Ho, Wo, generator=g) if r.res is not None else None
    return dict(x0=x0, x1=x1, w=w, bias=bias if r.bias else None, coef=coef, res=res)


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 convolution of the whole row (returned in fp32, as ref_conv does); computed once, never modified"""
    r, i = T.BY_NAME[name], make(name)
    return ref_conv(i['x0'], i['w'], i['bias'], i['x1'], 1, r.ups, i['coef'], r.act, i['res'])


def first_image(inp):
    cut = lambda t: None if t is None else t[:1].contiguous()
    return dict(inp, x0=cut(inp['x0']), x1=cut(inp['x1']), res=cut(inp['res']),
                coef=None if inp['coef'] is None else (cut(inp['coef'][0]), cut(inp['coef'][1])))


def launch(r, inp, fd=None, scratch_floats=None):
    """One dlpm_conv2d_f32 launch of row r's layer on `inp` under the profiler.  Returns (out NCHW cpu, canaries intact, profiler classes)."""
    B = inp['x0'].shape[0]
    Ho, Wo = T.out_size(r)
    stem = r.kernel.startswith('stem')
    strips = []

    def guarded(t):
        """a device copy of t with a NaN strip before and behind it; the pointer to the copy"""
        buf = torch.full((t.numel() + 2 * CAN,), float('nan'), device=DEV)
        buf[CAN:CAN + t.numel()] = t.to(DEV).reshape(-1)
        strips.append((buf, t.numel()))
        return buf.data_ptr() + 4 * CAN
    a = _lib.ConvArgs()
    a.src0, a.C0 = guarded(inp['x0'] if stem else nhwc(inp['x0'])), r.C0
    if inp['x1'] is not None:
        a.src1, a.C1 = guarded(nhwc(inp['x1'])), r.C1
    a.B, a.Hin, a.Win, a.Hout, a.Wout = B, r.Hin, r.Win, Ho, Wo
    a.ksize, a.stride, a.upsample, a.Cout = 3, 1, r.ups, r.Cout
    w = inp['w'].to(DEV).contiguous()
    a.weight = w.data_ptr()
    if inp['bias'] is not None:
        a.bias = guarded(inp['bias'])
    if inp['coef'] is not None:
        a.coefA, a.coefB = guarded(inp['coef'][0]), guarded(inp['coef'][1])
    a.act_silu = int(r.act)
    if inp['res'] is not None:
        if r.res == 'one':
            a.res0, a.R0 = guarded(nhwc(inp['res'])), r.Cout
        else:
            a.res0, a.res1, a.R0 = guarded(nhwc(inp['res'][:, :r.res])), guarded(nhwc(inp['res'][:, r.res:])), r.res
    n_out = B * Ho * Wo * r.Cout
    out = torch.full((n_out + 2 * CAN,), float('nan'), device=DEV)
    strips.append((out, n_out))
    a.out = out.data_ptr() + 4 * CAN
    a.in_nchw, a.out_nchw = int(stem), int(r.out_nchw)
    a.force_direct = T.force_bits(r) if fd is None else fd
    a.scratch_floats = T.scratch_floats(r) if scratch_floats is None else scratch_floats
    scratch = torch.full((a.scratch_floats + CAN,), float('nan'), device=DEV)
    buf = C.create_string_buffer(1 << 14)
    _lib.check(L().dlpm_prof_enable(1))
    try:
        _lib.check(L().dlpm_conv2d_f32(C.byref(a), scratch.data_ptr(), st()))
        _lib.check(L().dlpm_prof_report(buf, len(buf)))
    finally:
        _lib.check(L().dlpm_prof_enable(0))
    torch.cuda.synchronize()
    bits = lambda t: bool((t.view(torch.int32) == NAN_BITS).all())
    intact = all(bits(b[:CAN]) and bits(b[CAN + n:]) for b, n in strips) and bits(scratch[a.scratch_floats:])
    o = out[CAN:CAN + n_out]
    o = o.view(B, r.Cout, Ho, Wo) if r.out_nchw else nchw(o.view(B, Ho, Wo, r.Cout))
    classes = [ln.split()[0].split(':')[0] for ln in buf.value.decode().strip().splitlines()]
    return o.cpu(), intact, classes


def bound(r, inp):
    return 1e-5 if r.kernel.startswith('stem') else conv_tol(inp['w'], r.C0 + r.C1)


def spans_images(r):
    return (r.kernel in ('halo_ws', 'halo') and r.cls[3] > 1) or r.kernel in ('head_gemm', 'head_fused', 'stem_regw')


def checked(r, inp, want, what, **kw):
    """a launch with the checks every launch gets: its kernel, its canaries, every output written, the bound.  Returns (out, error)."""
    out, intact, classes = launch(r, inp, **kw)
    took = ['conv_direct'] if kw.get('fd') == 1 else T.prof_classes(r)
    assert classes == took, (r.name, what, classes)
    assert intact, (r.name, what)
    assert out.shape == want.shape and bool(torch.isfinite(out).all()), (r.name, what)
    err, tol = (out - want).abs().max().item(), bound(r, inp)
    print('TILES %s %s%s max|out - fp64| %.3e bound %.3e' % (T.FAMILY[r.kernel], r.name, what, err, tol))
    assert err < tol, (r.name, what, err)
    return out, err


@pytest.mark.parametrize('name', [r.name for r in T.ROWS])
def test_tile_row(name):
    r = T.BY_NAME[name]
    inp, want = make(inputs_name(r)), reference(inputs_name(r))
    out, err = checked(r, inp, want, '')
    if r.kernel == 'head_fused':          # its fp32-MFMA form beside the bf16 x 3 one
        out32, err32 = checked(r, inp, want, ' (fp32 MFMA)', fd=T.force_bits(r, f32=True))
        assert err <= 1.5 * err32 + 1e-7, (name, err, err32)
    if spans_images(r):
        alone, _, _ = launch(r, first_image(inp))
        assert torch.equal(alone[0], out[0]), name
    if r.kernel == 'halo':
        twin = T.BY_NAME[r.twin]
        ws, _ = checked(twin, inp, want, ' (weight-streaming kernel)')
        checked(r, inp, want, ' (direct kernel)', fd=1, scratch_floats=T.scratch_floats(twin))
        assert torch.equal(ws, out), name
