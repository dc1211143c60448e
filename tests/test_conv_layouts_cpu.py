"""conv_layouts and the layout table (conv.h) against the code they replaced: tests/conv_layout_table.cpp walks a grid of layers and prints
the layouts conv_layouts grants each, with their float counts; tests/golden/conv_layouts.txt holds the same table as conv3_layouts, the
*_weight_floats functions and prep_conv's inline conditions gave it on the commit before.  And dlpm_conv_policy_route's scratch_floats --
the table's placement -- against the values that commit gave (conv_policy_cases.SCRATCH_FLOATS).  Host code only: no GPU is touched."""
import os
import subprocess

import pytest

import conv_policy_cases as P
from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_layouts.txt')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
LAYOUTS = ['plain', 'plain_direct', 'frag', 'wino', 'wino4', 'wino4sp', 'wino4_one', 'wino4_n64', 'wino4_n32', 'split', 'head', 'head_taps',
           'head_fused', 'small']        # ConvLayout, in the order of the enum
NARROW_COPIES_MAX_BATCH = 512


def _golden():
    with open(GOLDEN) as f:
        return f.read().splitlines()


def _columns(row):
    """kind, ks, input channels (C0, C1), Cout, declared batch, and {layout: floats}"""
    desc, _, lay = row.partition(' |')
    kind, ks, _, cin, cout, d = desc.split()
    return kind, int(ks[1:]), tuple(int(c) for c in cin[1:].split('+')), int(cout[1:]), int(d[1:]), {n: int(f) for n, f in (g.split(':') for g in lay.split())}


def test_golden_table_covers_every_layout():
    """The table cannot hide a layout or a rule: these conditions hold on the golden file itself."""
    rows = [_columns(r) for r in _golden()]
    assert os.path.getsize(GOLDEN) < 300 * 1000
    assert {k for k, *_ in rows} == {'ordinary', 'stem', 'head', 'time_mlp', 'stride2', 'upsample'}
    for name in LAYOUTS:
        assert sum(1 for *_, lay in rows if name in lay) >= 10, name
    assert all(set(lay) <= set(LAYOUTS) for *_, lay in rows)
    # the narrow copies on both sides of NARROW_COPIES_MAX_BATCH
    wide = [(d, lay) for _, ks, _, cout, d, lay in rows if 'wino4' in lay and cout % 128 == 0]
    assert any(d == NARROW_COPIES_MAX_BATCH and 'wino4_n64' in lay and 'wino4_n32' in lay for d, lay in wide)
    assert any(d == NARROW_COPIES_MAX_BATCH + 1 and 'wino4_n64' not in lay and 'wino4_n32' not in lay for d, lay in wide)
    # a 1x1 implicit-GEMM layer owns no plain copy (the parameter is that layout already)
    assert any(ks == 1 and 'plain' not in lay and 'plain_direct' not in lay for _, ks, _, _, _, lay in rows)
    # a 3x3 layer the implicit GEMM does not take (C0 % 32 != 0): the plain copy -- in the direct kernel's order -- and nothing else
    assert any(ks == 3 and c0 % 32 != 0 and list(lay) == ['plain_direct'] for _, ks, (c0, _), _, _, lay in rows)


def test_conv_layouts_match_the_code_they_replaced(tmp_path):
    libdir = os.path.join(ROOT, 'dlpm_amd', 'lib')
    exe = str(tmp_path / 'conv_layout_table')
    subprocess.check_call([HIPCC, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', os.path.join(ROOT, 'tests', 'conv_layout_table.cpp'),
                           '-o', exe, '-L', libdir, '-ldlpm_amd', '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib'])
    env = {k: v for k, v in os.environ.items() if not k.startswith('DLPM_')}      # the switches at their defaults
    got = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env, check=True).stdout.splitlines()
    want = _golden()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, 'row %d: conv_layouts gives\n  %s\nthe parent gave\n  %s' % (i + 1, g, w)
    assert len(got) == len(want)


@pytest.mark.parametrize('c', P.CASES, ids=[c.name for c in P.CASES])
def test_policy_scratch_floats_are_the_parents(c):
    assert P.case_route(c).scratch_floats == P.SCRATCH_FLOATS[c.name]
