"""The weight-layout table (conv.h: ConvLayout, conv_layouts.hip) against the code it replaced, bit for bit: sha256 digests of the layout
bytes dlpm_conv_policy_f32 writes, of the outputs of dlpm_conv2d_f32 under the force_direct bits that ask for a layout, and of a whole
net's forward across set_conv_policy calls.  tests/golden/conv_layout_digests.json was recorded on MI355X with the library of the commit
before the table existed (`python tests/test_gpu_conv_layouts.py` rewrites it: every digest is computed twice and kept only if it
repeats); a later change that deliberately moves one of these bits has to re-record it from a tree it trusts."""
import ctypes as C
import hashlib
import json
import math
import os
import sys

import pytest
import torch

from conftest import ROOT
from conv_policy_cases import Case, out_size
from dlpm_amd import _lib
from test_gpu_kernels import DEV, L, nhwc, run_conv, st
from test_host_mirror import build_unet

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_layout_digests.json')
SENTINEL = -12345.0

# ---- layout bytes: the scratch of dlpm_conv_policy_f32, B = 2.  Between them the cases make every layout of a 3x3 stride-1 layer
LAYOUT_CASES = [
    Case('lay_16x16_32to128_d64', 2, 32, 0, 16, 16, 128, 0, False, None, True, 64, None, 0, 0, 0),    # plain, frag, wino, wino4, n64, n32
    Case('lay_ups4to8_32to128_d0', 2, 32, 0, 4, 4, 128, 1, False, None, True, 0, None, 0, 0, 0),      # (sixteen one-tile images: no sub-pixel copy)
    Case('lay_ups8to16_32to128_d0', 2, 32, 0, 8, 8, 128, 1, False, None, True, 0, None, 0, 0, 0),     # + wino4sp
    Case('lay_4x4_64to64_d4096', 2, 64, 0, 4, 4, 64, 0, False, None, True, 4096, None, 0, 0, 0),      # + the one-tile copy
]
# ---- outputs through dlpm_conv2d_f32: (name, B, Cin, H, Cout, ks, ups, head, force_direct).  The GEMM + gather head (bit 32) takes
# images from 16 pixels wide and the one-pass head (bit 64; 128: its fp32 form) 32 or 64 wide, so on the 8x8 head bits 32 and 64 are
# refused -- "a bit asks, a different route is an error" -- and what is recorded for them is the error text; the 32x32 head beside it
# runs all three head kernels.  Likewise the sub-pixel kernel (bit 256) leaves 4x4 low-res images to the F(4x4,3x3) kernel and takes 8x8.
HEAD, HEAD32 = (2, 32, 8, 3, 3, 0, True), (2, 32, 32, 3, 3, 0, True)
OUTPUT_CASES = [('out_head_fd0',) + HEAD + (0,), ('out_head_fd32',) + HEAD + (32,), ('out_head_fd64',) + HEAD + (64,),
                ('out_head_fd192',) + HEAD + (64 | 128,),
                ('out_head32_fd0',) + HEAD32 + (0,), ('out_head32_fd32',) + HEAD32 + (32,), ('out_head32_fd64',) + HEAD32 + (64,),
                ('out_head32_fd192',) + HEAD32 + (64 | 128,),
                ('out_1x1_32to128_fd16', 2, 32, 8, 128, 1, 0, False, 16),
                ('out_4x4_64to64_b16_fd520', 16, 64, 4, 64, 3, 0, False, 8 | 512),
                ('out_ups4to8_32to128_fd264', 2, 32, 4, 128, 3, 1, False, 8 | 256),
                ('out_ups8to16_32to128_fd264', 2, 32, 8, 128, 3, 1, False, 8 | 256)]
NET_STEPS = [('net_undeclared', None), ('net_d64', 64), ('net_back_to_d0', 0), ('net_d64_again', 64)]


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _seeded(name):
    return torch.Generator().manual_seed(sum(map(ord, name)))


def layout_digest(c):
    """Seeded weights as test_gpu_conv_policy.make draws them; the scratch pre-filled with a sentinel; sha256 of scratch[0 : scratch_floats]"""
    g = _seeded(c.name)
    Cin = c.C0 + c.C1
    Ho, Wo = out_size(c)
    x0 = torch.randn(c.B, c.C0, c.Hin, c.Win, generator=g)
    w = torch.randn(c.Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    bias = torch.randn(c.Cout, generator=g)
    keep = [nhwc(x0).to(DEV), w.to(DEV).contiguous(), bias.to(DEV), torch.empty(c.B * Ho * Wo * c.Cout, device=DEV)]
    a = _lib.ConvArgs()
    a.src0, a.weight, a.bias, a.out = (t.data_ptr() for t in keep)
    a.C0, a.B, a.Hin, a.Win, a.Hout, a.Wout = c.C0, c.B, c.Hin, c.Win, Ho, Wo
    a.ksize, a.stride, a.upsample, a.Cout = 3, 1, c.ups, c.Cout
    need = _lib.ConvRoute()
    _lib.check(L().dlpm_conv_policy_route(C.byref(a), _lib.CONV_AUTO, c.d, C.byref(need)))
    scratch = torch.full((need.scratch_floats,), SENTINEL, device=DEV)
    a.scratch_floats = scratch.numel()
    part = torch.empty(max(1, need.partial_floats), device=DEV)
    _lib.check(L().dlpm_conv_policy_f32(C.byref(a), _lib.CONV_AUTO, c.d, scratch.data_ptr(), part.data_ptr(), part.numel(), None, None, None, st()))
    torch.cuda.synchronize()
    return _sha(scratch)


def output_digest(case):
    name, B, Cin, H, Cout, ks, ups, head, fd = case
    g = _seeded(name.rsplit('_fd', 1)[0])        # (the head cases share their inputs)
    x = torch.randn(B, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / math.sqrt(Cin * ks * ks)
    bias = torch.randn(Cout, generator=g)
    coef = (1 + 0.3 * torch.randn(B, Cin, generator=g), 0.3 * torch.randn(B, Cin, generator=g)) if head else None
    # room for the head layouts and the tap-channel tensor; for the one-tile (36 floats per weight) or sub-pixel (104) copy behind the rest
    extra = 112 * Cin + 4096 + B * H * H * 32 if head else 112 * w.numel() + 8192
    try:
        return _sha(run_conv(x, w, bias, None, 1, ups, coef, head, None, out_nchw=head, force_direct=fd, scratch_extra=extra))
    except _lib.DlpmError as e:
        return 'refused: %s' % e


def net_digests():
    """'wide' of test_gpu_models (mc = 128, [1, 2]: every ResBlock / Upsample convolution has Cout % 128 == 0) on 8x8 images, so that its
    second level is 4x4: the forward undeclared, under a declared batch of 64 (which builds the narrow copies), undeclared again
    (which frees them), declared again (which rebuilds them)."""
    net, _ = build_unet('wide')
    g = torch.Generator().manual_seed(21)
    x, t = torch.randn(2, 3, 8, 8, generator=g).to(DEV), torch.rand(2, generator=g).to(DEV)
    out = {}
    for name, d in NET_STEPS:
        if d is not None:
            net.set_conv_policy('auto', d)
        out[name] = _sha(net(x, t))
    return out


def compute():
    d = {c.name: layout_digest(c) for c in LAYOUT_CASES}
    d.update({c[0]: output_digest(c) for c in OUTPUT_CASES})
    d.update(net_digests())
    return d


@pytest.fixture(scope='module')
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize('c', LAYOUT_CASES, ids=[c.name for c in LAYOUT_CASES])
def test_layout_bytes_are_the_parents(c, recorded):
    assert layout_digest(c) == recorded[c.name]


@pytest.mark.parametrize('case', OUTPUT_CASES, ids=[c[0] for c in OUTPUT_CASES])
def test_conv2d_outputs_are_the_parents(case, recorded):
    assert output_digest(case) == recorded[case[0]]


def test_net_forward_across_policy_changes_is_the_parents(recorded):
    got = net_digests()
    assert got['net_undeclared'] == got['net_back_to_d0'] and got['net_d64'] == got['net_d64_again'], got
    for name, _ in NET_STEPS:
        assert got[name] == recorded[name], name


if __name__ == '__main__':
    first, second = compute(), compute()
    keep = {k: v for k, v in first.items() if second[k] == v}
    for k in first:
        print('%s %s %s' % (k, first[k], 'repeats' if k in keep else 'DOES NOT REPEAT: ' + second[k]))
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, 'w') as f:
        json.dump(keep, f, indent=1, sort_keys=True)
        f.write('\n')
