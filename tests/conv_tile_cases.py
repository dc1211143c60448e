"""The case table tests/test_conv_tile_cases_cpu.py and tests/test_gpu_conv_tiles.py share: one dlpm_conv2d_f32 launch for every tile shape
the halo, head and stem convolution kernels take from the image's width and height.  No GPU is needed to import this module.

The predicates are mirrored here in Python (each cites the C++ it mirrors; tests/test_conv_tile_cases_cpu.py holds the mirrors against
conv_route itself, through tests/conv_tile_table.cpp), and the classes are enumerated from the mirrors over output sizes Hout, Wout in
1 .. 96 (stems: Hout up to 256):
  halo   (ups, Wout, th, nimg)    k_conv3x3_halo_ws (plain and UPS) and k_conv3x3_halo: th full rows of an image, or nimg whole images
  head   ('HEAD', Wout, TH)       k_conv3x3_head: TH rows per workgroup
         ('HEAD_GEMM', Wout, TH)  1x1 GEMM + k_head_gather: TH rows per gather tile (Cout 1 .. 3: TH follows Cout as well)
         ('HEAD_FUSED', Wout, nr) the one-pass kernel of head_fused.hip: nr rows per phase
  stem   (kernel, Wout, rows)     k_conv_stem_lds: rows = 1024 / Wout rows of one image per block; k_conv_stem_regw (blocks of 1024 pixels of
                                  the flattened batch) and k_conv_stem (one thread per pixel and channel quad) take nothing from the image's
                                  shape: one class each, (kernel, 0, 0)
ROWS holds one row per class on the smallest image (fewest output pixels) that reaches it, then the seam rows: halo images of 3 and 5
tiles (16x24 and 32x20 outputs, plain and upsampled), head images of 2 and 3 tiles for each head family (the GEMM head, whose height is
a power of two: 2 and 4), a 96x32 stem (three blocks per image), a regw stem whose 1024-pixel blocks span images (28x28, B = 3), one with
a ragged last block (5x7) and a k_conv_stem row beyond the 1x1 image of its class.  Then, for every third
non-upsampling halo class and both classes on the LDS budget nimg (th + 2)(W + 2) 8 <= 9 * 256, a second row for k_conv3x3_halo, and two
halo rows that write NCHW with Cout = 3 (the scalar epilogue).

What the rows carry.  Halo row i: Cout = (128, 64, 32, 96, 128, 64, 32, 192)[i % 8] -- the three BN instantiations, and 96 / 192 whose
last BN = 128 tile is ragged; plain (no bias) for i % 4 == 0, GroupNorm coefficients + SiLU for 1, one residual for 2, a residual concat
with R0 = 16 for 3; a 32+32 input concat where (i // 2) % 2 == 1, else 32 channels.  B = nimg + 1 where nimg > 1 (the last tile holds one
live image and dead ones), else 2.  Heads and stems: B = 3; heads rotate Cout 3 / 1 / 2 (k_conv3x3_head also 4) and 32 / 64 input
channels, stems Cout 32 / 64 / 128 and 3 / 1 image channels."""
import collections

BM, KC, HALO_NIT = 128, 32, 9           # conv_igemm.hip: pixels per tile, channels per chunk, halo staging iterations

# kernel: 'halo_ws' / 'halo' (k_conv3x3_halo, reached by a scratch too small for the fragment copy) / 'head' / 'head_gemm' / 'head_fused' /
# 'stem_lds' / 'stem_regw' / 'stem'; act: GroupNorm coefficients + SiLU; res: None, 'one' or R0 of a concat; cls: the class (see above);
# twin: for a 'halo' row, the name of the 'halo_ws' row with the same launch (and the same seeded inputs)
T = collections.namedtuple('T', 'name kernel B C0 C1 Hin Win Cout ups act res bias out_nchw cls twin')

FAMILY = {'halo_ws': 'IGEMM', 'halo': 'IGEMM', 'head': 'HEAD', 'head_gemm': 'HEAD_GEMM', 'head_fused': 'HEAD_FUSED', 'stem_lds': 'STEM',
          'stem_regw': 'STEM', 'stem': 'STEM'}


# ---------------------------------------------------------------- the mirrors
def halo_ok(Hout, Wout, ups, Cin=32, w_frag=True):
    """halo_ok (csrc/conv_igemm.hip:1023-1040) of a 3x3 stride-1 launch: (th, nimg) or None"""
    if ups and (not w_frag or Wout & 1 or Hout & 1):
        return None
    W, HW = Wout, Hout * Wout
    if W < 4 or W > 64 or BM % W:
        return None
    if HW >= BM:
        if HW % BM:
            return None
        th, nimg = BM // W, 1
    else:
        if BM % HW:
            return None
        th, nimg = Hout, BM // HW
    if ups and (th & 1 or Cin % KC):
        return None
    return (th, nimg) if nimg * (th + 2) * (W + 2) * 8 <= HALO_NIT * 256 else None


def igemm_bn(Cout):
    """launch_igemm's BN (csrc/conv_igemm.hip:1227-1229, 1234-1236): the instantiation <BN, WAVES_M, WAVES_N, RM, RN>"""
    return 128 if Cout > 64 else 64 if Cout > 32 else 32


def frag_last_float_read(Cout, Cin):
    """Index of the last float of w_frag that k_conv3x3_halo_ws<BN, ..., RING = 2> reads (csrc/conv_igemm.hip:643-646, 679, 697-698): the wave
    with the highest n-block nb = ntile_n BN / 32 - 1 starts its stream at group nb nch 36 and reads nch 36 + 1 groups (the one-ahead
    prefetch of the last iteration) of 64 lanes x 4 floats."""
    bn, nch = igemm_bn(Cout), Cin // KC
    nb = (Cout + bn - 1) // bn * (bn // 32) - 1
    return ((nb + 1) * nch * 36) * 256 + 255


def head_rows(Hout, Wout):
    """head_rows (csrc/conv_direct.hip:368)"""
    return min(Hout, 512 // Wout)


def head_conv_ok(Hout, Wout, Cout=3, C0=32):
    """head_conv_ok (csrc/conv_direct.hip:370-378) of a 3x3 stride-1 launch that carries w_small: TH or None"""
    if Cout < 1 or Cout > 4 or C0 % 16:
        return None
    W, H = Wout, Hout
    if W < 8 or W > 64 or W & 3 or 512 % W:
        return None
    TH = head_rows(H, W)
    nthr = TH * (W // 4)
    return TH if H % TH == 0 and nthr % 64 == 0 and nthr <= 128 else None


HG_LD = 29


def head_gather_rows(Hout, Wout, Cout):
    """head_gather_rows (csrc/conv_direct.hip:402-409)"""
    th, nq4 = Hout, (9 * Cout + 3) // 4
    while th > 1 and ((th + 2) * (Wout + 2) * HG_LD * 4 > 48 * 1024 or Cout * th * (Wout // 4) > 256 or (th + 2) * (Wout + 2) * nq4 > 2560):
        th >>= 1
    return th


def head_gemm_ok(Hout, Wout, Cout=3, C0=32):
    """head_gemm_ok (csrc/conv_direct.hip:411-420) of a launch that carries w_taps: the gather's TH or None"""
    if Cout < 1 or Cout > 3 or C0 % 32:
        return None
    W, H = Wout, Hout
    if W < 16 or W > 64 or W & 3 or H & (H - 1) or (H * W) % 128:
        return None
    TH = head_gather_rows(H, W, Cout)
    items = (TH + 2) * (W + 2) * ((9 * Cout + 3) // 4)
    ok = H % TH == 0 and (TH + 2) * (W + 2) * HG_LD * 4 <= 48 * 1024 and Cout * TH * (W // 4) <= 256 and items <= 2560
    return TH if ok else None


def head_fused_ok(Hout, Wout, Cout=3, C0=32, bf=True):
    """head_fused_ok (csrc/head_fused.hip:463-470; LDS: 456-459) of a launch with coefficients + SiLU that carries w_hfused: nr or None"""
    if Cout < 1 or Cout > 3 or C0 % 32 or C0 > 128 or Wout not in (32, 64):
        return None
    nr = 8 // (Wout >> 5)
    lds = 9 * Cout * ((nr + 2) * Wout + 4) + C0 * (48 if bf else 32) + 4 * C0
    return nr if Hout % nr == 0 and Hout // nr >= 2 and lds * 4 <= 80 * 1024 else None


def stem_kernel(Hout, Wout, Cout):
    """launch_conv_stem's lds_ok / regw (csrc/conv_igemm.hip:1087-1111) of a stem launch (1 or 3 image channels, bias): (kernel, W, rows)"""
    Cq = Cout // 4
    regw = 1 <= Cq <= 256 and Cq & (Cq - 1) == 0
    W = Wout
    if regw and W & (W - 1) == 0 and 4 <= W <= 64 and 1024 % W == 0 and (Hout * W) % 1024 == 0:
        return ('stem_lds', W, 1024 // W)
    return ('stem_regw', 0, 0) if regw else ('stem', 0, 0)


# ---------------------------------------------------------------- the classes
SIDES = range(1, 97)


def _smallest(found, cls, key, val):
    if cls not in found or key < found[cls][0]:
        found[cls] = (key, val)


def enumerate_halo():
    """{(ups, Wout, th, nimg): (Hout, Wout) of the smallest image}"""
    found = {}
    for ups in (0, 1):
        for H in SIDES:
            for W in SIDES:
                r = halo_ok(H, W, ups)
                if r:
                    _smallest(found, (ups, W) + r, (H * W, H), (H, W))
    return {k: v[1] for k, v in found.items()}


def enumerate_heads():
    """{(family, Wout, tile rows): (Hout, Wout, Cout)}; the GEMM head over Cout 3, 2, 1 (at equal size the largest Cout)"""
    found = {}
    for H in SIDES:
        for W in SIDES:
            if head_conv_ok(H, W):
                _smallest(found, ('HEAD', W, head_conv_ok(H, W)), (H * W, 0), (H, W, 3))
            for Cout in (3, 2, 1):
                if head_gemm_ok(H, W, Cout):
                    _smallest(found, ('HEAD_GEMM', W, head_gemm_ok(H, W, Cout)), (H * W, -Cout), (H, W, Cout))
            if head_fused_ok(H, W):
                _smallest(found, ('HEAD_FUSED', W, head_fused_ok(H, W)), (H * W, 0), (H, W, 3))
    return {k: v[1] for k, v in found.items()}


def enumerate_stems():
    """{(kernel, Wout, rows): (Hout, Wout, Cout)}, Hout up to 256; Cout 32 (8 channel quads) and 24 (6: no power of two)"""
    found = {}
    for H in range(1, 257):
        for W in SIDES:
            for Cout in (32, 24):
                _smallest(found, stem_kernel(H, W, Cout), (H * W, -Cout), (H, W, Cout))
    return {k: v[1] for k, v in found.items()}


def square_pow2_classes():
    """the classes of the three enumerations that a square image with a power-of-two side reaches"""
    halo, head, stem = set(), set(), set()
    for S in (1, 2, 4, 8, 16, 32, 64):
        for ups in (0, 1):
            r = halo_ok(S, S, ups)
            if r:
                halo.add((ups, S) + r)
        if head_conv_ok(S, S):
            head.add(('HEAD', S, head_conv_ok(S, S)))
        for Cout in (3, 2, 1):
            if head_gemm_ok(S, S, Cout):
                head.add(('HEAD_GEMM', S, head_gemm_ok(S, S, Cout)))
        if head_fused_ok(S, S):
            head.add(('HEAD_FUSED', S, head_fused_ok(S, S)))
        for Cout in (32, 24):
            stem.add(stem_kernel(S, S, Cout))
    return halo, head, stem


# ---------------------------------------------------------------- the rows
HALO_COUT = (128, 64, 32, 96, 128, 64, 32, 192)
CARRY = ((False, None, False, ''), (True, None, True, '_coef'), (False, 'one', True, '_res'), (False, 16, True, '_rescat'))


def _halo_rows():
    rows = []

    def add(ups, Ho, Wo, note=''):
        i = len(rows)
        th, nimg = halo_ok(Ho, Wo, ups)
        Cout, C1 = HALO_COUT[i % 8], 32 if (i // 2) % 2 else 0
        act, res, bias, tag = CARRY[i % 4]
        Hin, Win = (Ho // 2, Wo // 2) if ups else (Ho, Wo)
        name = 'halo_%sW%d_th%d_n%d_%dx%d_%sto%d%s%s' % ('ups_' if ups else '', Wo, th, nimg, Ho, Wo, '32_32' if C1 else '32', Cout, tag, note)
        rows.append(T(name, 'halo_ws', nimg + 1 if nimg > 1 else 2, 32, C1, Hin, Win, Cout, ups, act, res, bias, False, (ups, Wo, th, nimg), None))
    classes = enumerate_halo()
    for cls in sorted(classes):
        add(cls[0], *classes[cls])
    for ups in (0, 1):                  # 3 and 5 tiles per image: the m0 -> (pb, y0) decode divides by H W and W
        add(ups, 24, 16, '_tiles3')
        add(ups, 20, 32, '_tiles5')
    return rows


def _budget_edge(cls):
    ups, W, th, nimg = cls
    return nimg * (th + 2) * (W + 2) * 8 == HALO_NIT * 256


def _plain_halo_rows(halo_rows):
    """k_conv3x3_halo on every third non-upsampling class and on both budget-edge classes: the twin's launch with the scratch cut short"""
    plain = [r for r in halo_rows if not r.ups and not r.name.endswith(('_tiles3', '_tiles5'))]
    pick = [r for i, r in enumerate(plain) if i % 3 == 0 or _budget_edge(r.cls)]
    return [r._replace(name=r.name.replace('halo_', 'halo_plain_', 1), kernel='halo', twin=r.name) for r in pick]


def _nchw_rows():
    """Cout = 3 written as NCHW: BN = 32, the scalar epilogue (the head's shape kept on the halo kernel by force_direct = 2)"""
    return [T('halo_W16_th8_n1_16x16_32to3_nchw_coef', 'halo_ws', 2, 32, 0, 16, 16, 3, 0, True, None, True, True, (0, 16, 8, 1), None),
            T('halo_W8_th8_n2_8x8_32to3_nchw', 'halo_ws', 3, 32, 0, 8, 8, 3, 0, False, None, True, True, (0, 8, 8, 2), None)]


def _head_rows():
    rows = []
    kern = {'HEAD': 'head', 'HEAD_GEMM': 'head_gemm', 'HEAD_FUSED': 'head_fused'}

    def add(fam, Ho, Wo, Cout, seam=False):
        i = len(rows)
        C0 = (32, 64)[i % 2]
        if fam == 'HEAD':
            Cout, t = (3, 1, 2, 4)[i % 4], head_conv_ok(Ho, Wo)
        elif fam == 'HEAD_GEMM':
            t = head_gemm_ok(Ho, Wo, Cout)
        else:
            Cout = (3, 1, 2)[i % 3]
            t = head_fused_ok(Ho, Wo, Cout, C0)
        name = '%s_W%d_t%d_%dx%d_%dto%d%s' % (kern[fam], Wo, t, Ho, Wo, C0, Cout, '_tiles%d' % (Ho // t) if seam else '')
        # (the one-pass kernel takes launches with coefficients + SiLU only; the others rotate: activation on even rows)
        act = fam == 'HEAD_FUSED' or i % 2 == 0
        rows.append(T(name, kern[fam], 3, C0, 0, Ho, Wo, Cout, 0, act, None, True, i % 3 != 2, (fam, Wo, t), None))
    classes = enumerate_heads()
    for cls in sorted(classes):
        add(cls[0], *classes[cls])
    # images of 2 and 3 tiles (the one-pass kernel's class rows have 2 phases already; the GEMM head's H is a power of two: 2 and 4)
    for fam, Ho, Wo in (('HEAD', 32, 32), ('HEAD', 48, 32), ('HEAD_GEMM', 32, 16), ('HEAD_GEMM', 64, 16), ('HEAD_FUSED', 24, 32), ('HEAD_FUSED', 12, 64)):
        add(fam, Ho, Wo, 3, True)
    return rows


def _stem_rows():
    rows = []

    def add(Ho, Wo, Cout, note=''):
        i = len(rows)
        kernel, W, r = stem_kernel(Ho, Wo, Cout)
        C0 = (3, 1)[i % 2]
        rows.append(T('%s_%dx%d_%dto%d%s' % (kernel, Ho, Wo, C0, Cout, note), kernel, 3, C0, 0, Ho, Wo, Cout, 0, False, None, True, False,
                      (kernel, W, r), None))
    classes = enumerate_stems()
    for i, cls in enumerate(sorted(classes)):
        Ho, Wo, Cout = classes[cls]
        add(Ho, Wo, Cout if cls[0] == 'stem' else (32, 64, 128)[i % 3])
    add(96, 32, 64, '_blocks3')
    add(28, 28, 32, '_spans_images')            # 784 pixels per image: the 1024-pixel blocks 0 and 1 end inside images 1 and 2
    add(5, 7, 64, '_ragged')                    # 105 pixels in all: one block, most of it past the end
    add(6, 10, 24, '_quads6')                   # k_conv_stem beyond the 1x1 image of its class row
    return rows


HALO_ROWS = _halo_rows()
ROWS = HALO_ROWS + _plain_halo_rows(HALO_ROWS) + _nchw_rows() + _head_rows() + _stem_rows()
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)

# classes enumerated, classes with a row, classes a square power-of-two image reaches -- pinned by tests/test_conv_tile_cases_cpu.py
N_HALO, N_HEAD, N_STEM = (26, 26, 10), (30, 30, 9), (7, 7, 4)


def out_size(r):
    return (2 * r.Hin, 2 * r.Win) if r.ups else (r.Hin, r.Win)


def r0_of(r):
    return 0 if r.res is None else r.Cout if r.res == 'one' else r.res


def force_bits(r, f32=False):
    """dlpm_conv2d_f32's force_direct of a row: 2 (no Winograd) for the halo rows, 32 / 64 (| 128: the fp32-MFMA form) for the GEMM and
    one-pass heads, none for k_conv3x3_head and the stems (which read NCHW)"""
    return {'halo_ws': 2, 'halo': 2, 'head_gemm': 32, 'head_fused': 64 | (128 if f32 else 0)}.get(r.kernel, 0)


def plain_floats(r):
    return r.Cout * (r.C0 + r.C1) * 9


def scratch_floats(r):
    """what the launch of a row offers as scratch: run_conv's size (tests/test_gpu_kernels.py) with the heads' extras -- or, for a
    k_conv3x3_halo row, the plain copy alone, so that conv2d_entry (csrc/unet.hip) leaves the fragment copy out"""
    if r.kernel == 'halo':
        return plain_floats(r)
    Ho, Wo = out_size(r)
    # (k_conv3x3_head's copy goes to the END of the scratch and is offered only where the plain and fragment copies fit in front of it:
    # room for both, or a narrow head on many channels falls to the halo kernel without a word)
    extra = {'head_gemm': 32 * r.C0 + r.B * Ho * Wo * 32, 'head_fused': 80 * r.C0 + 4096, 'head': (r.C0 // 32 * 144 + 2) * 256 + 36 * r.C0}.get(r.kernel, 0)
    return 9 * plain_floats(r) + 16 * 1024 * (1 + r.Cout // 32) + extra


def prof_classes(r):
    """the profiler classes the launch of a row reports (conv_route's ConvRoute::name; launch_conv_head, launch_conv_head_gemm,
    launch_conv_head_fused and launch_conv_stem name their own)"""
    return {'halo_ws': ['conv3x3_halo'], 'halo': ['conv3x3_halo'], 'head': ['conv3x3_head'], 'head_gemm': ['conv1x1_igemm', 'head_gather'],
            'head_fused': ['head_fused']}.get(r.kernel, ['conv_stem'])


def descriptor_line(r, f32=False):
    """a row as tests/conv_tile_table.cpp reads it"""
    Ho, Wo = out_size(r)
    stem = r.kernel.startswith('stem')
    return ' '.join(str(v) for v in (r.name, r.B, r.C0, r.C1, r.Hin, r.Win, Ho, Wo, r.Cout, r.ups, int(r.act), r0_of(r), int(r.res not in (None, 'one')),
                                     int(r.bias), int(stem), int(r.out_nchw), force_bits(r, f32), scratch_floats(r)))
