"""Every block shape the Winograd route predicates admit, the parts that need no GPU: the route of every row of the table the GPU test
runs (tests/conv_geometry_cases.py), and that the table has a row for every class the grid reaches -- no more, no fewer."""
import itertools

import pytest

from conv_geometry_cases import (CHANNELS, N_CLASSES, ROWS, SIDES, WINOGRAD, alone_route, blocks, enumerate_classes, full_route, row_class,
                                 row_route, tail_batch, want_route)
from conv_policy_cases import descriptor, out_size, query
from dlpm_amd import _lib


@pytest.fixture(scope='module')
def classes():
    return enumerate_classes()


@pytest.mark.parametrize('g', ROWS, ids=[g.case.name for g in ROWS])
def test_row_takes_its_route(g):
    c = g.case
    r = row_route(g)
    assert full_route(r) == want_route(g), (c.name, full_route(r))
    assert c.family in WINOGRAD and r.partial_floats == 0 and c.ksplit == 1
    Ho, Wo = out_size(c)
    t = {'WINO': 2, 'WINO4': 4, 'WINO4SP': 8}[c.family]
    if c.nimg == 1:          # blocks of bh x bw tiles tile the image
        assert Ho % (t * g.bh) == 0 and Wo % (t * g.bw) == 0 and c.B == 2
    else:                    # nimg whole images per block; the last block of the launch holds one live image
        assert (Ho, Wo) == (t * g.bh, t * g.bw) and c.B in (c.nimg + 1, tail_batch(c.nimg))
        if c.B == c.nimg + 1:
            assert alone_route(g) == want_route(g)                   # ... and image 0 alone takes the same route
        else:                # a class of the large batch only: alone, the image runs in a 32-tile block of the 4-wave F(2x2) shape --
            #                  two images per block, or (32-tile images) one, which then emits statistics
            assert c.family == 'WINO' and c.nq == 64 and g.bh * g.bw * c.nimg == 64 and full_route(row_route(g, c.B - 1)) != want_route(g)
            assert alone_route(g) == ('WINO', 64, c.nimg // 2, 1, g.bh, g.bw, 128 if c.nimg == 2 else 0)
    assert c.C0 + c.C1 in (32, 64) and c.C0 == 32 and c.Cout in (c.nq, 2 * c.nq)


def test_every_class_has_a_row_and_no_row_is_outside_the_grid(classes):
    """No skip list: the classes of the rows ARE the classes of the grid."""
    assert len(classes) == N_CLASSES, len(classes)
    have = {row_class(g) for g in ROWS}
    assert not classes - have, sorted(classes - have)
    assert not have - classes, sorted(have - classes)
    assert [row_class(g) for g in ROWS[:N_CLASSES]] == sorted(classes)     # one row per class, in class order, then the extras


def test_family_does_not_follow_the_batch_of_the_call():
    """conv.h's invariant on the grid: the route is a function of the layer and the declared policy.  The one exception is the block
    shape of the F(2x2) small launch, which has the bits of the large one -- so it may change the block, never the family.  (Images of
    1 x 32 and 2 x 16 tiles used to run F(2x2) from B = 511 up and the implicit GEMM below.)"""
    for H, W, ups in itertools.product(SIDES, SIDES, (0, 1)):
        if max(H, W) * (2 if ups else 1) > 96:
            continue
        for (c0, c1), Cout, gen, d in itertools.product(CHANNELS, (128, 64, 32), range(4), (0, 64)):
            seen = {}
            for B in (1, 2, 64, 511, 1024, 4096):
                r = query(descriptor(B, c0, c1, H, W, Cout, ups), gen, d)
                seen[B] = (r.family, r.ksplit) if _lib.CONV_FAMILIES[r.family] == 'WINO' else full_route(r)
            assert len(set(seen.values())) == 1, (H, W, ups, c0, c1, Cout, gen, d, seen)


def test_rows_rotate_over_what_a_launch_carries():
    for i, g in enumerate(ROWS):
        c = g.case
        assert (c.act, c.res, c.bias) == [(False, None, False), (True, None, True), (False, 'one', True), (False, 16, True)][i % 4], c.name
    for fam in WINOGRAD:
        mine = [g.case for g in ROWS if g.case.family == fam]
        assert any(c.C1 for c in mine) and any(not c.C1 for c in mine), fam
        assert {c.res for c in mine} == {None, 'one', 16} and any(c.act for c in mine), fam
        assert any(c.Cout == 2 * c.nq for c in mine), fam


@pytest.mark.parametrize('fam', WINOGRAD)
def test_table_holds_images_with_3_and_5_blocks_per_row(fam):
    """bpr no power of two in the mb -> (img0, ty0, tx0) decode -- with more than one block row, so that both the quotient and the
    remainder by bpr are exercised."""
    per_row = {blocks(g) for g in ROWS if g.case.family == fam and g.case.nimg == 1}
    assert {n for rows, n in per_row if rows >= 2} >= {3, 5}, sorted(per_row)
