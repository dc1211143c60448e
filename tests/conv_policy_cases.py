"""The case table tests/test_conv_policy_cpu.py and tests/test_gpu_conv_policy.py share: 3x3 stride-1 convolution launches that exist only
under a declared dispatch batch (include/dlpm_amd_conv.h) -- split-K grid copies of the F(2x2) kernel and of the 32-channel F(4x4)
n-tiles, and the 64- / 32-channel n-tiles of a Cout % 128 == 0 layer -- each with the route it is meant to take.  No GPU is needed to
import this module or to ask for a route."""
import collections
import ctypes as C

from dlpm_amd import _lib

# res: None, 'one' (one tensor of Cout channels) or R0 (a concat [R0 | Cout - R0]); act: GroupNorm coefficients + SiLU on the input;
# d: the declared dispatch batch; family, nq, nimg, ksplit: the route
Case = collections.namedtuple('Case', 'name B C0 C1 Hin Win Cout ups act res bias d family nq nimg ksplit')

CASES = [
    # ---- F(2x2) split-K (k_conv3x3_wino_q): 8, 2 or 1 images per block; the first and fourth are the 4-wave small launch
    Case('f2_4x4_32_32to64_d256', 5, 32, 32, 4, 4, 64, 0, False, None, False, 256, 'WINO', 64, 8, 2),
    Case('f2_ups2to4_128_128to64_d2', 5, 128, 128, 2, 2, 64, 1, True, None, True, 2, 'WINO', 64, 8, 8),
    Case('f2_ups2to4_256_128to256_d2_rescat', 5, 256, 128, 2, 2, 256, 1, False, 128, True, 2, 'WINO', 128, 8, 8),
    Case('f2_ups4to8_64_64to64_d64_rescat', 5, 64, 64, 4, 4, 64, 1, True, 32, True, 64, 'WINO', 64, 2, 4),
    Case('f2_16x16_64_32to128_d8_res', 3, 64, 32, 16, 16, 128, 0, False, 'one', True, 8, 'WINO', 128, 1, 2),   # copy 1 starts at channel 48 < C0
    Case('f2_ups4x8to8x16_256_128to128_d64', 2, 256, 128, 4, 8, 128, 1, True, None, True, 64, 'WINO', 128, 1, 4),
    # ---- F(4x4) split-K on 32-channel n-tiles (k_conv3x3_wino4<*, 4, 2>): 16, 4, 2 or 1 images per block, Cout = 96: three n-tiles
    Case('f4_16x16_32_32to32_d64_coef_res', 3, 32, 32, 16, 16, 32, 0, True, 'one', True, 64, 'WINO4', 32, 1, 2),
    Case('f4_8x16_128_128to32_d64', 5, 128, 128, 8, 16, 32, 0, False, None, False, 64, 'WINO4', 32, 2, 8),
    Case('f4_8x16_128_128to96_d2', 5, 128, 128, 8, 16, 96, 0, False, None, True, 2, 'WINO4', 32, 2, 8),
    Case('f4_ups2to4_256_128to96_d256', 19, 256, 128, 2, 2, 96, 1, True, None, True, 256, 'WINO4', 32, 16, 4),
    Case('f4_ups4to8_32_32to96_d64_coef', 5, 32, 32, 4, 4, 96, 1, True, None, True, 64, 'WINO4', 32, 4, 2),
    Case('f4_ups8to16_128_128to32_d2_rescat', 2, 128, 128, 8, 8, 32, 1, False, 16, True, 2, 'WINO4', 32, 1, 8),
    # ---- narrow n-tiles of a Cout % 128 == 0 layer, no split (the w_wino4_n64 / w_wino4_n32 fragment streams)
    Case('nq32_16x16_32to128_d64', 2, 32, 0, 16, 16, 128, 0, True, 'one', True, 64, 'WINO4', 32, 1, 1),
    Case('nq64_16x16_32to128_d128', 2, 32, 0, 16, 16, 128, 0, False, None, True, 128, 'WINO4', 64, 1, 1),
    Case('nq64_16x16_32to256_d64', 2, 32, 0, 16, 16, 256, 0, True, None, True, 64, 'WINO4', 64, 1, 1),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# dlpm_conv_policy_route(..).scratch_floats of each case (AUTO, the case's declared batch), recorded from the commit before the weight
# layouts moved into one table (conv.h: ConvLayout): the floats the layouts of the layer take, one behind the other at multiples of 64
# (the three Cout = 96 cases: those values + one n-block of Cin / 32 * 36 * 256 floats, since the fragment copy is padded to whole
# 128-channel tiles -- frag_weight_floats, csrc/conv_igemm.hip; tests/test_conv_tile_cases_cpu.py holds that size against the kernel's reads)
SCRATCH_FLOATS = {
    'f2_4x4_32_32to64_d256': 440832,
    'f2_ups2to4_128_128to64_d2': 1151488,
    'f2_ups2to4_256_128to256_d2_rescat': 13967872,
    'f2_ups4to8_64_64to64_d64_rescat': 578048,
    'f2_16x16_64_32to128_d8_res': 1753600,
    'f2_ups4x8to8x16_256_128to128_d64': 6988288,
    'f4_16x16_32_32to32_d64_coef_res': 113152,
    'f4_8x16_128_128to32_d64': 444928,
    'f4_8x16_128_128to96_d2': 1403392,
    'f4_ups2to4_256_128to96_d256': 2103808,
    'f4_ups4to8_32_32to96_d64_coef': 352768,
    'f4_ups8to16_128_128to32_d2_rescat': 444928,
    'nq32_16x16_32to128_d64': 590336,
    'nq64_16x16_32to128_d128': 590336,
    'nq64_16x16_32to256_d64': 1171968,
}
assert sorted(SCRATCH_FLOATS) == sorted(BY_NAME)
SPLIT = [c for c in CASES if c.ksplit > 1]
NARROW = [c for c in CASES if c.ksplit == 1]


def out_size(c):
    return (2 * c.Hin, 2 * c.Win) if c.ups else (c.Hin, c.Win)


def descriptor(B, C0, C1, Hin, Win, Cout, ups, R0=0):
    """dlpm_conv_args of a 3x3 stride-1 launch with every pointer null: what the route query reads"""
    a = _lib.ConvArgs()
    a.C0, a.C1, a.B, a.Hin, a.Win = C0, C1, B, Hin, Win
    a.Hout, a.Wout = (2 * Hin, 2 * Win) if ups else (Hin, Win)
    a.ksize, a.stride, a.upsample, a.Cout, a.R0 = 3, 1, int(ups), Cout, R0
    return a


def r0_of(c):
    return 0 if c.res is None else c.Cout if c.res == 'one' else c.res


def query(a, gen, d):
    """dlpm_conv_policy_route: the route as a dlpm_conv_route"""
    r = _lib.ConvRoute()
    _lib.check(_lib.lib().dlpm_conv_policy_route(C.byref(a), gen, d, C.byref(r)))
    return r


def route_tuple(r):
    return (_lib.CONV_FAMILIES[r.family], r.nq, r.nimg, r.ksplit)


def case_route(c, B=None):
    return query(descriptor(B or c.B, c.C0, c.C1, c.Hin, c.Win, c.Cout, c.ups, r0_of(c)), _lib.CONV_AUTO, c.d)


def slices(c):
    """input channel ranges [lo, hi) of the S grid copies"""
    Cin = c.C0 + c.C1
    return [(s * Cin // c.ksplit, (s + 1) * Cin // c.ksplit) for s in range(c.ksplit)]
