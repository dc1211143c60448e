"""The case table tests/test_conv_geometry_cpu.py and tests/test_gpu_conv_geometry.py share: one 3x3 stride-1 launch for every block
shape the Winograd route predicates admit -- wino_geometry (F(2x2), csrc/conv_wino.hip), f4_block / wino4_geometry_nq (F(4x4)) and
wino4sp_block (the sub-pixel upsample kernel, both csrc/conv_wino4.hip) -- each with the route it is meant to take.  No GPU is needed
to import this module or to ask for a route.

The grid.  enumerate_classes() asks dlpm_conv_policy_route for every launch of: input H and W even from 2 to 64, plus 80 and 96; output
at most 96x96 pixels; Cout 128, 64 and 32; inputs of 32, 64 and 32+32 (a concat) channels; upsample 0 and 1; generations AUTO, F4, F2 and
IGEMM; declared batch 0 and 64; B = 2 and 1024.  139 distinct classes (family, upsample, nq, bh, bw, nimg) reach a Winograd kernel
(counted at the commit that added this file): 124 at B = 2, and 15 more at B = 1024 -- a 64-channel F(2x2) layer on images smaller
than a 64-tile block runs 32-tile blocks on 4 waves while the grid of 64-tile blocks would leave CUs empty (wino_small_launch follows
the batch of the CALL), so the 64-tile blocks of two or four whole images exist only from 256 such blocks up.  A square image whose
side is a power of two reaches 32 of the 139, so 107 had never run in a test.  (Before this file there were 18 such classes: images of
1 x 32 and 2 x 16 tiles ran two per 64-tile block in a large batch and on the implicit GEMM in a small one, which the 32-tile shape
cannot cut into 4 x 8-tile blocks; wino_geometry now refuses them at every batch.)

The rows.  ROWS[:139] hold one row per class, in sorted class order, on the smallest image (fewest output pixels) that reaches it:
  B = nimg + 1 where nimg > 1 (the last block holds one live image, the rest dead), else 2; the 15 large-batch classes take
  B = 256 nimg - (nimg - 1): the smallest batch that reaches them, 256 blocks, again with one live image in the last (names end _B<B>);
  the generation is the first of (F4, 0), (F2, 0), (AUTO, 0), (F4, 64), (F2, 64), (AUTO, 64) -- generation, declared batch -- that
  reaches the class, so ksplit == 1 wherever a class does not need a declaration (one class does: 16 one-tile images on 128-channel
  n-tiles; its route keeps ksplit 1 too);
  Cout = one or two n-tiles of nq (rows alternate which is tried first; 64- and 32-channel n-tiles exist only for one n-tile);
  row i is plain (no bias) for i % 4 == 0, has GroupNorm coefficients + SiLU for 1, one residual for 2, a residual concat with R0 = 16
  for 3; rows with (i // 2) % 2 == 1 take a 32+32 input concat, the others 32 channels.  (A 16+16 concat is not in the table: the policy
  entry gives a layer its Winograd layouts only where the implicit GEMM takes it, C0 % 32 == 0, and routes 16+16 to the direct kernel.)
ROWS[139:] are six more, for the mb -> (img0, ty0, tx0) decode where the blocks per row are no power of two: for each of the three
families an image of two block rows with 3 and one with 5 blocks per row.  The sub-pixel kernel's blocks are 16 low-res tiles wide, so
its 5-blocks-per-row image is 32x80 -> 64x160, wider than the grid; its class (4x4 tiles, one image) is in the enumeration."""
import collections
import itertools

from conv_policy_cases import Case, descriptor, out_size, query, r0_of, route_tuple
from dlpm_amd import _lib

GEN = {'AUTO': _lib.CONV_AUTO, 'F4': _lib.CONV_F4, 'F2': _lib.CONV_F2, 'IGEMM': _lib.CONV_IGEMM}
WINOGRAD = ('WINO', 'WINO4', 'WINO4SP')
# case: the launch and (family, nq, nimg, ksplit) of its route, d its declared batch; gen: the generation; bh, bw, stats_px: the rest of the route
G = collections.namedtuple('G', 'case gen bh bw stats_px')

ROWS = [
    G(Case('f2_nq64_b1x8_n4_2x16_32to64', 5, 32, 0, 2, 16, 64, 0, False, None, False, 0, 'WINO', 64, 4, 1), 'F4', 1, 8, 0),
    G(Case('f2_nq64_b1x16_n2_2x32_32to64_coef', 3, 32, 0, 2, 32, 64, 0, True, None, True, 0, 'WINO', 64, 2, 1), 'F4', 1, 16, 0),
    G(Case('f2_nq64_b1x16_n4_2x32_32_32to64_res_B1021', 1021, 32, 32, 2, 32, 64, 0, False, 'one', True, 0, 'WINO', 64, 4, 1), 'F4', 1, 16, 0),
    G(Case('f2_nq64_b2x2_n8_4x4_32_32to64_rescat', 9, 32, 32, 4, 4, 64, 0, False, 16, True, 0, 'WINO', 64, 8, 1), 'F2', 2, 2, 0),
    G(Case('f2_nq64_b2x4_n4_4x8_32to64', 5, 32, 0, 4, 8, 64, 0, False, None, False, 0, 'WINO', 64, 4, 1), 'F4', 2, 4, 0),
    G(Case('f2_nq64_b2x8_n2_4x16_32to64_coef', 3, 32, 0, 4, 16, 64, 0, True, None, True, 0, 'WINO', 64, 2, 1), 'F4', 2, 8, 0),
    G(Case('f2_nq64_b2x8_n4_4x16_32_32to64_res_B1021', 1021, 32, 32, 4, 16, 64, 0, False, 'one', True, 0, 'WINO', 64, 4, 1), 'F4', 2, 8, 0),
    G(Case('f2_nq64_b4x2_n4_8x4_32_32to64_rescat', 5, 32, 32, 8, 4, 64, 0, False, 16, True, 0, 'WINO', 64, 4, 1), 'F4', 4, 2, 0),
    G(Case('f2_nq64_b4x4_n2_8x8_32to64', 3, 32, 0, 8, 8, 64, 0, False, None, False, 0, 'WINO', 64, 2, 1), 'F2', 4, 4, 0),
    G(Case('f2_nq64_b4x4_n4_8x8_32to64_coef_B1021', 1021, 32, 0, 8, 8, 64, 0, True, None, True, 0, 'WINO', 64, 4, 1), 'F2', 4, 4, 0),
    G(Case('f2_nq64_b4x8_n1_8x16_32_32to64_res', 2, 32, 32, 8, 16, 64, 0, False, 'one', True, 0, 'WINO', 64, 1, 1), 'F2', 4, 8, 128),
    G(Case('f2_nq64_b4x8_n2_8x16_32_32to64_rescat_B511', 511, 32, 32, 8, 16, 64, 0, False, 16, True, 0, 'WINO', 64, 2, 1), 'F2', 4, 8, 0),
    G(Case('f2_nq64_b8x1_n4_16x2_32to64', 5, 32, 0, 16, 2, 64, 0, False, None, False, 0, 'WINO', 64, 4, 1), 'F4', 8, 1, 0),
    G(Case('f2_nq64_b8x2_n2_16x4_32to64_coef', 3, 32, 0, 16, 4, 64, 0, True, None, True, 0, 'WINO', 64, 2, 1), 'F4', 8, 2, 0),
    G(Case('f2_nq64_b8x2_n4_16x4_32_32to64_res_B1021', 1021, 32, 32, 16, 4, 64, 0, False, 'one', True, 0, 'WINO', 64, 4, 1), 'F4', 8, 2, 0),
    G(Case('f2_nq64_b8x4_n1_16x8_32_32to64_rescat', 2, 32, 32, 16, 8, 64, 0, False, 16, True, 0, 'WINO', 64, 1, 1), 'F2', 8, 4, 128),
    G(Case('f2_nq64_b8x4_n2_16x8_32to64_B511', 511, 32, 0, 16, 8, 64, 0, False, None, False, 0, 'WINO', 64, 2, 1), 'F2', 8, 4, 0),
    G(Case('f2_nq64_b8x8_n1_16x16_32to64_coef', 2, 32, 0, 16, 16, 64, 0, True, None, True, 0, 'WINO', 64, 1, 1), 'F2', 8, 8, 256),
    G(Case('f2_nq64_b16x1_n2_32x2_32_32to64_res', 3, 32, 32, 32, 2, 64, 0, False, 'one', True, 0, 'WINO', 64, 2, 1), 'F4', 16, 1, 0),
    G(Case('f2_nq64_b16x1_n4_32x2_32_32to64_rescat_B1021', 1021, 32, 32, 32, 2, 64, 0, False, 16, True, 0, 'WINO', 64, 4, 1), 'F4', 16, 1, 0),
    G(Case('f2_nq64_b16x2_n1_32x4_32to64', 2, 32, 0, 32, 4, 64, 0, False, None, False, 0, 'WINO', 64, 1, 1), 'F4', 16, 2, 128),
    G(Case('f2_nq64_b16x2_n2_32x4_32to64_coef_B511', 511, 32, 0, 32, 4, 64, 0, True, None, True, 0, 'WINO', 64, 2, 1), 'F4', 16, 2, 0),
    G(Case('f2_nq64_b16x4_n1_32x8_32_32to64_res', 2, 32, 32, 32, 8, 64, 0, False, 'one', True, 0, 'WINO', 64, 1, 1), 'F2', 16, 4, 256),
    G(Case('f2_nq64_b32x1_n1_64x2_32_32to64_rescat', 2, 32, 32, 64, 2, 64, 0, False, 16, True, 0, 'WINO', 64, 1, 1), 'F4', 32, 1, 128),
    G(Case('f2_nq64_b32x1_n2_64x2_32to64_B511', 511, 32, 0, 64, 2, 64, 0, False, None, False, 0, 'WINO', 64, 2, 1), 'F4', 32, 1, 0),
    G(Case('f2_nq64_b32x2_n1_64x4_32to64_coef', 2, 32, 0, 64, 4, 64, 0, True, None, True, 0, 'WINO', 64, 1, 1), 'F2', 32, 2, 256),
    G(Case('f2_nq128_b1x8_n4_2x16_32_32to128_res', 5, 32, 32, 2, 16, 128, 0, False, 'one', True, 0, 'WINO', 128, 4, 1), 'F4', 1, 8, 0),
    G(Case('f2_nq128_b1x16_n2_2x32_32_32to256_rescat', 3, 32, 32, 2, 32, 256, 0, False, 16, True, 0, 'WINO', 128, 2, 1), 'F4', 1, 16, 0),
    G(Case('f2_nq128_b2x2_n8_4x4_32to128', 9, 32, 0, 4, 4, 128, 0, False, None, False, 0, 'WINO', 128, 8, 1), 'F2', 2, 2, 0),
    G(Case('f2_nq128_b2x4_n4_4x8_32to256_coef', 5, 32, 0, 4, 8, 256, 0, True, None, True, 0, 'WINO', 128, 4, 1), 'F2', 2, 4, 0),
    G(Case('f2_nq128_b2x8_n2_4x16_32_32to128_res', 3, 32, 32, 4, 16, 128, 0, False, 'one', True, 0, 'WINO', 128, 2, 1), 'F2', 2, 8, 0),
    G(Case('f2_nq128_b4x2_n4_8x4_32_32to256_rescat', 5, 32, 32, 8, 4, 256, 0, False, 16, True, 0, 'WINO', 128, 4, 1), 'F2', 4, 2, 0),
    G(Case('f2_nq128_b4x4_n2_8x8_32to128', 3, 32, 0, 8, 8, 128, 0, False, None, False, 0, 'WINO', 128, 2, 1), 'F2', 4, 4, 0),
    G(Case('f2_nq128_b4x8_n1_8x32_32to256_coef', 2, 32, 0, 8, 32, 256, 0, True, None, True, 0, 'WINO', 128, 1, 1), 'F4', 4, 8, 128),
    G(Case('f2_nq128_b8x1_n4_16x2_32_32to128_res', 5, 32, 32, 16, 2, 128, 0, False, 'one', True, 0, 'WINO', 128, 4, 1), 'F4', 8, 1, 0),
    G(Case('f2_nq128_b8x2_n2_16x4_32_32to256_rescat', 3, 32, 32, 16, 4, 256, 0, False, 16, True, 0, 'WINO', 128, 2, 1), 'F2', 8, 2, 0),
    G(Case('f2_nq128_b8x4_n1_48x8_32to128', 2, 32, 0, 48, 8, 128, 0, False, None, False, 0, 'WINO', 128, 1, 1), 'F4', 8, 4, 128),
    G(Case('f2_nq128_b16x1_n2_32x2_32to256_coef', 3, 32, 0, 32, 2, 256, 0, True, None, True, 0, 'WINO', 128, 2, 1), 'F4', 16, 1, 0),
    G(Case('f2_nq128_b16x2_n1_96x4_32_32to128_res', 2, 32, 32, 96, 4, 128, 0, False, 'one', True, 0, 'WINO', 128, 1, 1), 'F4', 16, 2, 128),
    G(Case('f2_nq128_b32x1_n1_64x2_32_32to256_rescat', 2, 32, 32, 64, 2, 256, 0, False, 16, True, 0, 'WINO', 128, 1, 1), 'F4', 32, 1, 128),
    G(Case('f2_nq64_b2x2_n8_ups2x2to4x4_32to64', 9, 32, 0, 2, 2, 64, 1, False, None, False, 0, 'WINO', 64, 8, 1), 'F2', 2, 2, 0),
    G(Case('f2_nq64_b2x4_n4_ups2x4to4x8_32to64_coef', 5, 32, 0, 2, 4, 64, 1, True, None, True, 0, 'WINO', 64, 4, 1), 'F2', 2, 4, 0),
    G(Case('f2_nq64_b2x8_n2_ups2x8to4x16_32_32to64_res', 3, 32, 32, 2, 8, 64, 1, False, 'one', True, 0, 'WINO', 64, 2, 1), 'F2', 2, 8, 0),
    G(Case('f2_nq64_b2x8_n4_ups2x8to4x16_32_32to64_rescat_B1021', 1021, 32, 32, 2, 8, 64, 1, False, 16, True, 0, 'WINO', 64, 4, 1), 'F2', 2, 8, 0),
    G(Case('f2_nq64_b4x2_n4_ups4x2to8x4_32to64', 5, 32, 0, 4, 2, 64, 1, False, None, False, 0, 'WINO', 64, 4, 1), 'F2', 4, 2, 0),
    G(Case('f2_nq64_b4x4_n2_ups4x4to8x8_32to64_coef', 3, 32, 0, 4, 4, 64, 1, True, None, True, 0, 'WINO', 64, 2, 1), 'F2', 4, 4, 0),
    G(Case('f2_nq64_b4x4_n4_ups4x4to8x8_32_32to64_res_B1021', 1021, 32, 32, 4, 4, 64, 1, False, 'one', True, 0, 'WINO', 64, 4, 1), 'F2', 4, 4, 0),
    G(Case('f2_nq64_b4x8_n1_ups4x8to8x16_32_32to64_rescat', 2, 32, 32, 4, 8, 64, 1, False, 16, True, 0, 'WINO', 64, 1, 1), 'F2', 4, 8, 128),
    G(Case('f2_nq64_b4x8_n2_ups4x8to8x16_32to64_B511', 511, 32, 0, 4, 8, 64, 1, False, None, False, 0, 'WINO', 64, 2, 1), 'F2', 4, 8, 0),
    G(Case('f2_nq64_b8x2_n2_ups8x2to16x4_32to64_coef', 3, 32, 0, 8, 2, 64, 1, True, None, True, 0, 'WINO', 64, 2, 1), 'F2', 8, 2, 0),
    G(Case('f2_nq64_b8x2_n4_ups8x2to16x4_32_32to64_res_B1021', 1021, 32, 32, 8, 2, 64, 1, False, 'one', True, 0, 'WINO', 64, 4, 1), 'F2', 8, 2, 0),
    G(Case('f2_nq64_b8x4_n1_ups8x4to16x8_32_32to64_rescat', 2, 32, 32, 8, 4, 64, 1, False, 16, True, 0, 'WINO', 64, 1, 1), 'F2', 8, 4, 128),
    G(Case('f2_nq64_b8x4_n2_ups8x4to16x8_32to64_B511', 511, 32, 0, 8, 4, 64, 1, False, None, False, 0, 'WINO', 64, 2, 1), 'F2', 8, 4, 0),
    G(Case('f2_nq64_b8x8_n1_ups8x8to16x16_32to64_coef', 2, 32, 0, 8, 8, 64, 1, True, None, True, 0, 'WINO', 64, 1, 1), 'F2', 8, 8, 256),
    G(Case('f2_nq64_b16x2_n1_ups16x2to32x4_32_32to64_res', 2, 32, 32, 16, 2, 64, 1, False, 'one', True, 0, 'WINO', 64, 1, 1), 'F2', 16, 2, 128),
    G(Case('f2_nq64_b16x2_n2_ups16x2to32x4_32_32to64_rescat_B511', 511, 32, 32, 16, 2, 64, 1, False, 16, True, 0, 'WINO', 64, 2, 1), 'F2', 16, 2, 0),
    G(Case('f2_nq64_b16x4_n1_ups16x4to32x8_32to64', 2, 32, 0, 16, 4, 64, 1, False, None, False, 0, 'WINO', 64, 1, 1), 'F2', 16, 4, 256),
    G(Case('f2_nq64_b32x2_n1_ups32x2to64x4_32to64_coef', 2, 32, 0, 32, 2, 64, 1, True, None, True, 0, 'WINO', 64, 1, 1), 'F2', 32, 2, 256),
    G(Case('f2_nq128_b2x2_n8_ups2x2to4x4_32_32to128_res', 9, 32, 32, 2, 2, 128, 1, False, 'one', True, 0, 'WINO', 128, 8, 1), 'F2', 2, 2, 0),
    G(Case('f2_nq128_b2x4_n4_ups2x4to4x8_32_32to256_rescat', 5, 32, 32, 2, 4, 256, 1, False, 16, True, 0, 'WINO', 128, 4, 1), 'F2', 2, 4, 0),
    G(Case('f2_nq128_b2x8_n2_ups2x8to4x16_32to128', 3, 32, 0, 2, 8, 128, 1, False, None, False, 0, 'WINO', 128, 2, 1), 'F2', 2, 8, 0),
    G(Case('f2_nq128_b4x2_n4_ups4x2to8x4_32to256_coef', 5, 32, 0, 4, 2, 256, 1, True, None, True, 0, 'WINO', 128, 4, 1), 'F2', 4, 2, 0),
    G(Case('f2_nq128_b4x4_n2_ups4x4to8x8_32_32to128_res', 3, 32, 32, 4, 4, 128, 1, False, 'one', True, 0, 'WINO', 128, 2, 1), 'F2', 4, 4, 0),
    G(Case('f2_nq128_b4x8_n1_ups4x16to8x32_32_32to256_rescat', 2, 32, 32, 4, 16, 256, 1, False, 16, True, 0, 'WINO', 128, 1, 1), 'F4', 4, 8, 128),
    G(Case('f2_nq128_b8x2_n2_ups8x2to16x4_32to128', 3, 32, 0, 8, 2, 128, 1, False, None, False, 0, 'WINO', 128, 2, 1), 'F2', 8, 2, 0),
    G(Case('f2_nq128_b8x4_n1_ups24x4to48x8_32to256_coef', 2, 32, 0, 24, 4, 256, 1, True, None, True, 0, 'WINO', 128, 1, 1), 'F4', 8, 4, 128),
    G(Case('f2_nq128_b16x2_n1_ups48x2to96x4_32_32to128_res', 2, 32, 32, 48, 2, 128, 1, False, 'one', True, 0, 'WINO', 128, 1, 1), 'F4', 16, 2, 128),
    G(Case('f4_nq32_b2x2_n4_8x8_32_32to32_rescat', 5, 32, 32, 8, 8, 32, 0, False, 16, True, 0, 'WINO4', 32, 4, 1), 'F4', 2, 2, 64),
    G(Case('f4_nq32_b2x4_n2_8x16_32to32', 3, 32, 0, 8, 16, 32, 0, False, None, False, 0, 'WINO4', 32, 2, 1), 'F4', 2, 4, 0),
    G(Case('f4_nq32_b4x2_n2_16x8_32to32_coef', 3, 32, 0, 16, 8, 32, 0, True, None, True, 0, 'WINO4', 32, 2, 1), 'F4', 4, 2, 0),
    G(Case('f4_nq32_b4x4_n1_16x16_32_32to32_res', 2, 32, 32, 16, 16, 32, 0, False, 'one', True, 0, 'WINO4', 32, 1, 1), 'F4', 4, 4, 256),
    G(Case('f4_nq32_b8x2_n1_32x8_32_32to32_rescat', 2, 32, 32, 32, 8, 32, 0, False, 16, True, 0, 'WINO4', 32, 1, 1), 'F4', 8, 2, 256),
    G(Case('f4_nq32_b16x1_n1_64x4_32to32', 2, 32, 0, 64, 4, 32, 0, False, None, False, 0, 'WINO4', 32, 1, 1), 'F4', 16, 1, 256),
    G(Case('f4_nq64_b1x1_n16_4x4_32to128_coef', 17, 32, 0, 4, 4, 128, 0, True, None, True, 0, 'WINO4', 64, 16, 1), 'F4', 1, 1, 16),
    G(Case('f4_nq64_b2x2_n4_8x8_32_32to64_res', 5, 32, 32, 8, 8, 64, 0, False, 'one', True, 0, 'WINO4', 64, 4, 1), 'F4', 2, 2, 64),
    G(Case('f4_nq64_b2x4_n2_8x16_32_32to64_rescat', 3, 32, 32, 8, 16, 64, 0, False, 16, True, 0, 'WINO4', 64, 2, 1), 'F4', 2, 4, 0),
    G(Case('f4_nq64_b4x2_n2_16x8_32to64', 3, 32, 0, 16, 8, 64, 0, False, None, False, 0, 'WINO4', 64, 2, 1), 'F4', 4, 2, 0),
    G(Case('f4_nq64_b4x4_n1_16x16_32to64_coef', 2, 32, 0, 16, 16, 64, 0, True, None, True, 0, 'WINO4', 64, 1, 1), 'F4', 4, 4, 256),
    G(Case('f4_nq64_b8x2_n1_32x8_32_32to64_res', 2, 32, 32, 32, 8, 64, 0, False, 'one', True, 0, 'WINO4', 64, 1, 1), 'F4', 8, 2, 256),
    G(Case('f4_nq64_b16x1_n1_64x4_32_32to64_rescat', 2, 32, 32, 64, 4, 64, 0, False, 16, True, 0, 'WINO4', 64, 1, 1), 'F4', 16, 1, 256),
    G(Case('f4_nq128_b1x1_n16_4x4_32to128_d64', 17, 32, 0, 4, 4, 128, 0, False, None, False, 64, 'WINO4', 128, 16, 1), 'F4', 1, 1, 0),
    G(Case('f4_nq128_b1x2_n8_4x8_32to256_coef', 9, 32, 0, 4, 8, 256, 0, True, None, True, 0, 'WINO4', 128, 8, 1), 'F4', 1, 2, 0),
    G(Case('f4_nq128_b1x4_n4_4x16_32_32to128_res', 5, 32, 32, 4, 16, 128, 0, False, 'one', True, 0, 'WINO4', 128, 4, 1), 'F4', 1, 4, 64),
    G(Case('f4_nq128_b1x8_n2_4x32_32_32to256_rescat', 3, 32, 32, 4, 32, 256, 0, False, 16, True, 0, 'WINO4', 128, 2, 1), 'F4', 1, 8, 0),
    G(Case('f4_nq128_b2x1_n8_8x4_32to128', 9, 32, 0, 8, 4, 128, 0, False, None, False, 0, 'WINO4', 128, 8, 1), 'F4', 2, 1, 0),
    G(Case('f4_nq128_b2x2_n4_8x8_32to256_coef', 5, 32, 0, 8, 8, 256, 0, True, None, True, 0, 'WINO4', 128, 4, 1), 'F4', 2, 2, 64),
    G(Case('f4_nq128_b2x4_n2_8x16_32_32to128_res', 3, 32, 32, 8, 16, 128, 0, False, 'one', True, 0, 'WINO4', 128, 2, 1), 'F4', 2, 4, 0),
    G(Case('f4_nq128_b4x1_n4_16x4_32_32to256_rescat', 5, 32, 32, 16, 4, 256, 0, False, 16, True, 0, 'WINO4', 128, 4, 1), 'F4', 4, 1, 64),
    G(Case('f4_nq128_b4x2_n2_16x8_32to128', 3, 32, 0, 16, 8, 128, 0, False, None, False, 0, 'WINO4', 128, 2, 1), 'F4', 4, 2, 0),
    G(Case('f4_nq128_b4x4_n1_16x16_32to256_coef', 2, 32, 0, 16, 16, 256, 0, True, None, True, 0, 'WINO4', 128, 1, 1), 'F4', 4, 4, 256),
    G(Case('f4_nq128_b8x1_n2_32x4_32_32to128_res', 3, 32, 32, 32, 4, 128, 0, False, 'one', True, 0, 'WINO4', 128, 2, 1), 'F4', 8, 1, 0),
    G(Case('f4_nq128_b8x2_n1_32x8_32_32to256_rescat', 2, 32, 32, 32, 8, 256, 0, False, 16, True, 0, 'WINO4', 128, 1, 1), 'F4', 8, 2, 256),
    G(Case('f4_nq128_b16x1_n1_64x4_32to128', 2, 32, 0, 64, 4, 128, 0, False, None, False, 0, 'WINO4', 128, 1, 1), 'F4', 16, 1, 256),
    G(Case('f4_nq32_b1x1_n16_ups2x2to4x4_32to32_coef', 17, 32, 0, 2, 2, 32, 1, True, None, True, 0, 'WINO4', 32, 16, 1), 'F4', 1, 1, 0),
    G(Case('f4_nq32_b1x2_n8_ups2x4to4x8_32_32to32_res', 9, 32, 32, 2, 4, 32, 1, False, 'one', True, 0, 'WINO4', 32, 8, 1), 'F4', 1, 2, 0),
    G(Case('f4_nq32_b1x4_n4_ups2x8to4x16_32_32to32_rescat', 5, 32, 32, 2, 8, 32, 1, False, 16, True, 0, 'WINO4', 32, 4, 1), 'F4', 1, 4, 64),
    G(Case('f4_nq32_b1x8_n2_ups2x16to4x32_32to32', 3, 32, 0, 2, 16, 32, 1, False, None, False, 0, 'WINO4', 32, 2, 1), 'F4', 1, 8, 0),
    G(Case('f4_nq32_b2x1_n8_ups4x2to8x4_32to32_coef', 9, 32, 0, 4, 2, 32, 1, True, None, True, 0, 'WINO4', 32, 8, 1), 'F4', 2, 1, 0),
    G(Case('f4_nq32_b2x2_n4_ups4x4to8x8_32_32to32_res', 5, 32, 32, 4, 4, 32, 1, False, 'one', True, 0, 'WINO4', 32, 4, 1), 'F4', 2, 2, 64),
    G(Case('f4_nq32_b2x4_n2_ups4x8to8x16_32_32to32_rescat', 3, 32, 32, 4, 8, 32, 1, False, 16, True, 0, 'WINO4', 32, 2, 1), 'F4', 2, 4, 0),
    G(Case('f4_nq32_b4x1_n4_ups8x2to16x4_32to32', 5, 32, 0, 8, 2, 32, 1, False, None, False, 0, 'WINO4', 32, 4, 1), 'F4', 4, 1, 64),
    G(Case('f4_nq32_b4x2_n2_ups8x4to16x8_32to32_coef', 3, 32, 0, 8, 4, 32, 1, True, None, True, 0, 'WINO4', 32, 2, 1), 'F4', 4, 2, 0),
    G(Case('f4_nq32_b4x4_n1_ups8x8to16x16_32_32to32_res', 2, 32, 32, 8, 8, 32, 1, False, 'one', True, 0, 'WINO4', 32, 1, 1), 'F4', 4, 4, 256),
    G(Case('f4_nq32_b8x1_n2_ups16x2to32x4_32_32to32_rescat', 3, 32, 32, 16, 2, 32, 1, False, 16, True, 0, 'WINO4', 32, 2, 1), 'F4', 8, 1, 0),
    G(Case('f4_nq32_b8x2_n1_ups16x4to32x8_32to32', 2, 32, 0, 16, 4, 32, 1, False, None, False, 0, 'WINO4', 32, 1, 1), 'F4', 8, 2, 256),
    G(Case('f4_nq32_b16x1_n1_ups32x2to64x4_32to32_coef', 2, 32, 0, 32, 2, 32, 1, True, None, True, 0, 'WINO4', 32, 1, 1), 'F4', 16, 1, 256),
    G(Case('f4_nq64_b1x1_n16_ups2x2to4x4_32_32to64_res', 17, 32, 32, 2, 2, 64, 1, False, 'one', True, 0, 'WINO4', 64, 16, 1), 'F4', 1, 1, 0),
    G(Case('f4_nq64_b1x2_n8_ups2x4to4x8_32_32to64_rescat', 9, 32, 32, 2, 4, 64, 1, False, 16, True, 0, 'WINO4', 64, 8, 1), 'F4', 1, 2, 0),
    G(Case('f4_nq64_b1x4_n4_ups2x8to4x16_32to64', 5, 32, 0, 2, 8, 64, 1, False, None, False, 0, 'WINO4', 64, 4, 1), 'F4', 1, 4, 64),
    G(Case('f4_nq64_b1x8_n2_ups2x16to4x32_32to64_coef', 3, 32, 0, 2, 16, 64, 1, True, None, True, 0, 'WINO4', 64, 2, 1), 'F4', 1, 8, 0),
    G(Case('f4_nq64_b2x1_n8_ups4x2to8x4_32_32to64_res', 9, 32, 32, 4, 2, 64, 1, False, 'one', True, 0, 'WINO4', 64, 8, 1), 'F4', 2, 1, 0),
    G(Case('f4_nq64_b2x2_n4_ups4x4to8x8_32_32to64_rescat', 5, 32, 32, 4, 4, 64, 1, False, 16, True, 0, 'WINO4', 64, 4, 1), 'F4', 2, 2, 64),
    G(Case('f4_nq64_b2x4_n2_ups4x8to8x16_32to64', 3, 32, 0, 4, 8, 64, 1, False, None, False, 0, 'WINO4', 64, 2, 1), 'F4', 2, 4, 0),
    G(Case('f4_nq64_b4x1_n4_ups8x2to16x4_32to64_coef', 5, 32, 0, 8, 2, 64, 1, True, None, True, 0, 'WINO4', 64, 4, 1), 'F4', 4, 1, 64),
    G(Case('f4_nq64_b4x2_n2_ups8x4to16x8_32_32to64_res', 3, 32, 32, 8, 4, 64, 1, False, 'one', True, 0, 'WINO4', 64, 2, 1), 'F4', 4, 2, 0),
    G(Case('f4_nq64_b4x4_n1_ups8x8to16x16_32_32to64_rescat', 2, 32, 32, 8, 8, 64, 1, False, 16, True, 0, 'WINO4', 64, 1, 1), 'F4', 4, 4, 256),
    G(Case('f4_nq64_b8x1_n2_ups16x2to32x4_32to64', 3, 32, 0, 16, 2, 64, 1, False, None, False, 0, 'WINO4', 64, 2, 1), 'F4', 8, 1, 0),
    G(Case('f4_nq64_b8x2_n1_ups16x4to32x8_32to64_coef', 2, 32, 0, 16, 4, 64, 1, True, None, True, 0, 'WINO4', 64, 1, 1), 'F4', 8, 2, 256),
    G(Case('f4_nq64_b16x1_n1_ups32x2to64x4_32_32to64_res', 2, 32, 32, 32, 2, 64, 1, False, 'one', True, 0, 'WINO4', 64, 1, 1), 'F4', 16, 1, 256),
    G(Case('f4_nq128_b1x1_n16_ups2x2to4x4_32_32to256_rescat', 17, 32, 32, 2, 2, 256, 1, False, 16, True, 0, 'WINO4', 128, 16, 1), 'F4', 1, 1, 0),
    G(Case('f4_nq128_b1x2_n8_ups2x4to4x8_32to128', 9, 32, 0, 2, 4, 128, 1, False, None, False, 0, 'WINO4', 128, 8, 1), 'F4', 1, 2, 0),
    G(Case('f4_nq128_b1x4_n4_ups2x8to4x16_32to256_coef', 5, 32, 0, 2, 8, 256, 1, True, None, True, 0, 'WINO4', 128, 4, 1), 'F4', 1, 4, 64),
    G(Case('f4_nq128_b1x8_n2_ups2x16to4x32_32_32to128_res', 3, 32, 32, 2, 16, 128, 1, False, 'one', True, 0, 'WINO4', 128, 2, 1), 'F4', 1, 8, 0),
    G(Case('f4_nq128_b2x1_n8_ups4x2to8x4_32_32to256_rescat', 9, 32, 32, 4, 2, 256, 1, False, 16, True, 0, 'WINO4', 128, 8, 1), 'F4', 2, 1, 0),
    G(Case('f4_nq128_b2x2_n4_ups4x4to8x8_32to128', 5, 32, 0, 4, 4, 128, 1, False, None, False, 0, 'WINO4', 128, 4, 1), 'F4', 2, 2, 64),
    G(Case('f4_nq128_b2x4_n2_ups4x8to8x16_32to256_coef', 3, 32, 0, 4, 8, 256, 1, True, None, True, 0, 'WINO4', 128, 2, 1), 'F4', 2, 4, 0),
    G(Case('f4_nq128_b4x1_n4_ups8x2to16x4_32_32to128_res', 5, 32, 32, 8, 2, 128, 1, False, 'one', True, 0, 'WINO4', 128, 4, 1), 'F4', 4, 1, 64),
    G(Case('f4_nq128_b4x2_n2_ups8x4to16x8_32_32to256_rescat', 3, 32, 32, 8, 4, 256, 1, False, 16, True, 0, 'WINO4', 128, 2, 1), 'F4', 4, 2, 0),
    G(Case('f4_nq128_b4x4_n1_ups8x24to16x48_32to128', 2, 32, 0, 8, 24, 128, 1, False, None, False, 0, 'WINO4', 128, 1, 1), 'F4', 4, 4, 256),
    G(Case('f4_nq128_b8x1_n2_ups16x2to32x4_32to256_coef', 3, 32, 0, 16, 2, 256, 1, True, None, True, 0, 'WINO4', 128, 2, 1), 'F4', 8, 1, 0),
    G(Case('f4_nq128_b8x2_n1_ups48x4to96x8_32_32to128_res', 2, 32, 32, 48, 4, 128, 1, False, 'one', True, 0, 'WINO4', 128, 1, 1), 'F4', 8, 2, 256),
    G(Case('f4_nq128_b16x1_n1_ups32x2to64x4_32_32to256_rescat', 2, 32, 32, 32, 2, 256, 1, False, 16, True, 0, 'WINO4', 128, 1, 1), 'F4', 16, 1, 256),
    G(Case('sp_nq128_b2x2_n4_ups8x8to16x16_32to128', 5, 32, 0, 8, 8, 128, 1, False, None, False, 0, 'WINO4SP', 128, 4, 1), 'F4', 2, 2, 64),
    G(Case('sp_nq128_b2x4_n2_ups8x16to16x32_32to256_coef', 3, 32, 0, 8, 16, 256, 1, True, None, True, 0, 'WINO4SP', 128, 2, 1), 'F4', 2, 4, 0),
    G(Case('sp_nq128_b4x1_n4_ups16x4to32x8_32_32to128_res', 5, 32, 32, 16, 4, 128, 1, False, 'one', True, 0, 'WINO4SP', 128, 4, 1), 'F4', 4, 1, 64),
    G(Case('sp_nq128_b4x2_n2_ups16x8to32x16_32_32to256_rescat', 3, 32, 32, 16, 8, 256, 1, False, 16, True, 0, 'WINO4SP', 128, 2, 1), 'F4', 4, 2, 0),
    G(Case('sp_nq128_b4x4_n1_ups16x16to32x32_32to128', 2, 32, 0, 16, 16, 128, 1, False, None, False, 0, 'WINO4SP', 128, 1, 1), 'F4', 4, 4, 256),
    G(Case('sp_nq128_b8x1_n2_ups32x4to64x8_32to256_coef', 3, 32, 0, 32, 4, 256, 1, True, None, True, 0, 'WINO4SP', 128, 2, 1), 'F4', 8, 1, 0),
    G(Case('sp_nq128_b8x2_n1_ups32x8to64x16_32_32to128_res', 2, 32, 32, 32, 8, 128, 1, False, 'one', True, 0, 'WINO4SP', 128, 1, 1), 'F4', 8, 2, 256),
    G(Case('f2_nq64_b8x8_n1_32x48_32_32to64_rescat_bpr3', 2, 32, 32, 32, 48, 64, 0, False, 16, True, 0, 'WINO', 64, 1, 1), 'F2', 8, 8, 256),
    G(Case('f2_nq64_b8x8_n1_32x80_32to64_bpr5', 2, 32, 0, 32, 80, 64, 0, False, None, False, 0, 'WINO', 64, 1, 1), 'F2', 8, 8, 256),
    G(Case('f4_nq32_b4x4_n1_32x48_32to32_coef_bpr3', 2, 32, 0, 32, 48, 32, 0, True, None, True, 0, 'WINO4', 32, 1, 1), 'F4', 4, 4, 256),
    G(Case('f4_nq32_b4x4_n1_32x80_32_32to32_res_bpr5', 2, 32, 32, 32, 80, 32, 0, False, 'one', True, 0, 'WINO4', 32, 1, 1), 'F4', 4, 4, 256),
    G(Case('sp_nq128_b4x4_n1_ups32x48to64x96_32_32to256_rescat_bpr3', 2, 32, 32, 32, 48, 256, 1, False, 16, True, 0, 'WINO4SP', 128, 1, 1), 'F4', 4, 4, 256),
    G(Case('sp_nq128_b4x4_n1_ups32x80to64x160_32to128_bpr5', 2, 32, 0, 32, 80, 128, 1, False, None, False, 0, 'WINO4SP', 128, 1, 1), 'F4', 4, 4, 256),
]
N_CLASSES = 139
BY_NAME = {g.case.name: g for g in ROWS}
assert len(BY_NAME) == len(ROWS)

SIDES = list(range(2, 65, 2)) + [80, 96]
CHANNELS = [(32, 0), (64, 0), (32, 32)]
BATCHES = (2, 1024)


def full_route(r):
    """route_tuple and the block shape and statistics size behind it"""
    return route_tuple(r) + (r.bh, r.bw, r.stats_px)


def want_route(g):
    c = g.case
    return (c.family, c.nq, c.nimg, c.ksplit, g.bh, g.bw, g.stats_px)


def row_route(g, B=None):
    c = g.case
    return query(descriptor(B or c.B, c.C0, c.C1, c.Hin, c.Win, c.Cout, c.ups, r0_of(c)), GEN[g.gen], c.d)


def tail_batch(nimg):
    """the smallest batch of 256 blocks of nimg images whose last block holds one live image"""
    return 256 * nimg - (nimg - 1)


def alone_route(g):
    """the route of a multi-image row's image 0 launched alone (B = 1)"""
    return full_route(row_route(g, 1))


def row_class(g):
    c = g.case
    return (c.family, int(c.ups), c.nq, g.bh, g.bw, c.nimg)


def tile_px(family):
    """output pixels per tile side: 2 for F(2x2), 4 for F(4x4), 8 for the sub-pixel kernel (4 low-res pixels)"""
    return {'WINO': 2, 'WINO4': 4, 'WINO4SP': 8}[family]


def blocks(g):
    """(block rows, blocks per row) of a one-image-per-block row's output image"""
    Ho, Wo = out_size(g.case)
    t = tile_px(g.case.family)
    return Ho // (t * g.bh), Wo // (t * g.bw)


def enumerate_classes():
    """The classes (family, upsample, nq, bh, bw, nimg) of every launch of the grid in the module docstring that a Winograd kernel takes"""
    seen = set()
    for H, W, ups in itertools.product(SIDES, SIDES, (0, 1)):
        if max(H, W) * (2 if ups else 1) > 96:
            continue
        for (c0, c1), Cout in itertools.product(CHANNELS, (128, 64, 32)):
            for B, gen, d in itertools.product(BATCHES, range(4), (0, 64)):
                r = query(descriptor(B, c0, c1, H, W, Cout, ups), gen, d)
                fam = _lib.CONV_FAMILIES[r.family]
                if fam in WINOGRAD:
                    seen.add((fam, ups, r.nq, r.bh, r.bw, r.nimg))
    return seen
