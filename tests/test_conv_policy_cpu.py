"""The convolution launches that exist only under a declared dispatch batch, the parts that need no GPU: the C ABI of
include/dlpm_amd_conv.h, the route of every case of the table the GPU test runs (tests/conv_policy_cases.py), what that table must
cover, which (family, n-tile, split-K) combinations a 3x3 stride-1 layer can reach at all, and the refusals of the launch entry --
all of them before anything is enqueued."""
import ctypes as C
import itertools

import pytest

from dlpm_amd import _lib
from conv_policy_cases import CASES, NARROW, SPLIT, case_route, descriptor, out_size, query, r0_of, route_tuple, slices
from metric_helpers import buffers



# ---------------------------------------------------------------- the case table
@pytest.mark.parametrize('c', CASES, ids=[c.name for c in CASES])
def test_case_takes_its_route(c):
    r = case_route(c)
    assert route_tuple(r) == (c.family, c.nq, c.nimg, c.ksplit), (c.name, route_tuple(r))
    Ho, Wo = out_size(c)
    assert r.partial_floats == (c.ksplit * c.B * Ho * Wo * c.Cout if c.ksplit > 1 else 0)
    assert (r.stats_px == 0) if c.ksplit > 1 else (r.stats_px == 256)
    Cin = c.C0 + c.C1
    assert r.scratch_floats >= (9 + 9 + 36) * c.Cout * Cin         # the plain, fragment-order and F(4x4)-domain copies at the least
    # the route follows the declaration, not the batch the call carries (the 4-wave F(2x2) small launch may: bit-identical, conv_wino.hip)
    for B in (1, 5, 64):
        rb = case_route(c, B)
        assert route_tuple(rb)[0::3] == (c.family, c.ksplit) and rb.grid == r.grid
        if c.family == 'WINO4':
            assert route_tuple(rb) == route_tuple(r)
    # ... and without a declaration the layer runs unsplit on its own n-tile width
    r0 = query(descriptor(c.B, c.C0, c.C1, c.Hin, c.Win, c.Cout, c.ups, r0_of(c)), _lib.CONV_AUTO, 0)
    assert r0.ksplit == 1 and r0.partial_floats == 0 and r0.grid == 0
    if c.family == 'WINO4' and c.Cout % 128 == 0:
        assert r0.nq == 128 and route_tuple(query(descriptor(c.B, c.C0, c.C1, c.Hin, c.Win, c.Cout, c.ups, r0_of(c)), _lib.CONV_F4, 0))[1] == 128


def straddles_or_starts_inside_src1(c):
    """a grid copy's channel slice starts strictly inside src1, or holds channels of both concat sources"""
    return c.C1 > 0 and any(lo > c.C0 or lo < c.C0 < hi for lo, hi in slices(c))


def test_table_covers_what_the_issue_names():
    """A cap on what the table may leave out (conditions on the table, not a measurement)."""
    for fam in ('WINO', 'WINO4'):
        assert {c.ksplit for c in SPLIT if c.family == fam} == {2, 4, 8}, fam
    assert all(c.nq == 32 for c in SPLIT if c.family == 'WINO4')
    assert {c.nimg for c in SPLIT} == {1, 2, 4, 8, 16}
    assert sum(1 for c in SPLIT if c.ups) >= 3
    assert any(out_size(c)[0] != out_size(c)[1] for c in CASES) and any(c.ups and c.Hin != c.Win for c in SPLIT)
    assert sum(1 for c in SPLIT if straddles_or_starts_inside_src1(c)) >= 4
    assert any(lo < c.C0 < hi for c in SPLIT for lo, hi in slices(c))           # ... one of them across the boundary itself
    assert all((hi - lo) % 8 == 0 and (hi - lo) // 8 >= 4 for c in SPLIT for lo, hi in slices(c))    # whole 8-channel chunks, ksplit_for's floor
    assert sum(1 for c in CASES if c.act) >= 4 and sum(1 for c in SPLIT if c.act) >= 4
    assert sum(1 for c in SPLIT if isinstance(c.res, int) and c.res % 16 == 0 and 0 < c.res < c.Cout) >= 2
    assert any(c.res == 'one' for c in SPLIT) and any(c.res is None for c in SPLIT) and any(not c.bias for c in SPLIT)
    assert sum(1 for c in SPLIT if c.B % c.nimg != 0) >= 3
    assert {4, 8, 16} <= {c.nimg for c in SPLIT if c.B % c.nimg != 0 and c.B in (5, 19)}
    assert any(c.Cout == 96 for c in SPLIT)
    for nq in (64, 32):
        assert any(c.nq == nq and c.Cout % 128 == 0 and c.family == 'WINO4' for c in NARROW), nq
    assert any(c.Cout == 256 for c in NARROW)


# ---------------------------------------------------------------- reachability
# the axes of tests/conv_route_table.cpp, restricted to what the entry takes: 3x3 stride-1 with NHWC on both sides (its CIN < 16 rows are
# NCHW stems, its Cout < 32 rows NCHW heads)
SIZE = [(4, 4), (8, 8), (14, 14), (16, 16), (28, 28), (32, 32), (64, 64), (8, 16)]
CIN = [(16, 16), (24, 0), (32, 0), (32, 32), (64, 64), (128, 0), (128, 128), (256, 128)]
COUT = [32, 64, 96, 128, 256]
DISPATCH = [0, 2, 64, 256, 4096]
BATCH = [2, 5, 64]


def test_which_split_k_kernels_a_layer_can_reach():
    """Every (family, n-tile width) that runs split-K over the grid of conv_route_table.cpp, all four generations: the F(2x2) kernel on
    both block widths and the 32-channel F(4x4) n-tile, each with S = 2, 4 and 8 -- and nothing else.  The 64-channel n-tile NEVER splits:
    a layer that runs on it has Cout % 64 == 0, so it carries the F(2x2) weights too; AUTO then keeps it on F(4x4) only where the grid
    reaches 256 workgroups at the declared batch (wino4_preferred), and ksplit_for splits only where twice the grid is at most 256.  The
    instantiations k_conv3x3_wino4<*, 2, 4> therefore never see ConvLaunch::ksplit > 1 (beside the split-K section)."""
    seen = set()
    fam = _lib.CONV_FAMILIES
    L = _lib.lib()
    r = _lib.ConvRoute()
    for (Ho, Wo), (c0, c1), Cout, res, ups, B in itertools.product(SIZE, CIN, COUT, range(3), range(2), BATCH):
        if ups and (Ho % 2 or Wo % 2):
            continue
        a = descriptor(B, c0, c1, Ho // 2 if ups else Ho, Wo // 2 if ups else Wo, Cout, ups, (0, Cout, Cout // 2)[res])
        for gen, d in itertools.product(range(4), DISPATCH):
            assert L.dlpm_conv_policy_route(C.byref(a), gen, d, C.byref(r)) == 0
            assert r.ksplit in (1, 2, 4, 8)
            if r.ksplit > 1:
                assert gen == _lib.CONV_AUTO and d > 0 and r.stats_px == 0 and r.grid * r.ksplit <= 256
                seen.add((fam[r.family], r.nq, r.ksplit))
    assert seen == {(f, nq, S) for f, nq in (('WINO', 64), ('WINO', 128), ('WINO4', 32)) for S in (2, 4, 8)}, sorted(seen)


# ---------------------------------------------------------------- refusals, all before anything is enqueued
def test_launch_refuses_before_anything_is_enqueued():
    """No GPU here: every one of these returns before a kernel is launched (the device pointers are host addresses, never followed)."""
    L = _lib.lib()
    buf, p = buffers()
    c = SPLIT[0]
    need = case_route(c)

    def call(scratch_floats, partial_floats, stats=False, gen=_lib.CONV_AUTO, d=c.d, **o):
        a = descriptor(c.B, c.C0, c.C1, c.Hin, c.Win, c.Cout, c.ups)
        a.src0 = a.src1 = a.weight = a.out = p
        a.scratch_floats = scratch_floats
        for k, v in o.items():
            setattr(a, k, v)
        px = C.c_int32(-7)
        rc = L.dlpm_conv_policy_f32(C.byref(a), gen, d, p, p, partial_floats, p if stats else None, C.byref(px) if stats else None, None, None)
        assert px.value == -7
        return rc

    assert need.ksplit == c.ksplit and need.scratch_floats > 0 and need.partial_floats > 0
    assert call(need.scratch_floats - 1, need.partial_floats) == -5                       # DLPM_ERR_NOMEM: scratch
    assert call(need.scratch_floats, need.partial_floats - 1) == -5                       # ... partial buffer
    assert b'partial' in L.dlpm_last_error()
    assert call(need.scratch_floats, need.partial_floats, stats=True) == -3               # DLPM_ERR_UNSUPPORTED: a split-K launch has no statistics
    assert call(need.scratch_floats, need.partial_floats, ksize=1) == -3
    assert call(need.scratch_floats, need.partial_floats, stride=2) == -3
    assert call(need.scratch_floats, need.partial_floats, out_nchw=1) == -3
    assert call(need.scratch_floats, need.partial_floats, force_direct=8) == -3
    assert call(need.scratch_floats, need.partial_floats, gen=4) == -1                    # DLPM_ERR_ARG
    assert call(need.scratch_floats, need.partial_floats, d=-1) == -1
    assert call(need.scratch_floats, need.partial_floats, Hout=c.Hin + 1) == -1
    assert call(need.scratch_floats, need.partial_floats, src1=None) == -1                # C1 > 0 without src1
    r = _lib.ConvRoute()
    a = descriptor(c.B, c.C0, c.C1, c.Hin, c.Win, c.Cout, c.ups)
    assert L.dlpm_conv_policy_route(C.byref(a), 0, c.d, None) == -1 and L.dlpm_conv_policy_route(None, 0, c.d, C.byref(r)) == -1
