"""conv_route (conv.h) against the selector cascade it replaced: tests/conv_route_table.cpp walks a grid of convolution descriptors and
prints the route of each; tests/golden/conv_routes.txt holds the same table as the separate selectors (launch order, conv_stats_pixels,
conv_ksplit_for, the grid formulas) gave it.  Host code only: no GPU is touched."""
import os
import subprocess

from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_routes.txt')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FAMILIES = ['HEAD_FUSED', 'HEAD_GEMM', 'HEAD', 'SPLIT', 'WINO4SP', 'WINO4', 'WINO', 'IGEMM', 'STEM', 'DIRECT']


def _golden():
    with open(GOLDEN) as f:
        return f.read().splitlines()


def _columns(row):
    """descriptor fields, and the route: family, bh, bw, nimg, nq, stats_px, ksplit, grid"""
    desc, route = row.split(' | ')
    r = route.split()
    return desc.split(), r[0], [int(v) for v in r[1:]]


def test_golden_table_covers_every_route():
    """The table cannot hide a family or a geometry: these conditions hold on the golden file itself."""
    rows = [_columns(r) for r in _golden()]
    assert 1000 <= len(rows) and os.path.getsize(GOLDEN) <= 300 * 1024
    for fam in FAMILIES:
        assert sum(1 for _, f, _ in rows if f == fam) >= 10, fam
    assert {1, 2, 4, 8} <= {v[5] for _, _, v in rows}                                   # ksplit
    assert {128, 64, 32} <= {v[3] for _, f, v in rows if f in ('WINO4', 'WINO4SP')}      # the F(4x4) n-tile widths
    assert {0, 64, 128, 256, 1024} <= {v[4] for _, _, v in rows}                        # stats_px
    assert any(f == 'WINO' and v[4] > 0 for _, f, v in rows)                            # ... and an F(2x2) one
    assert any(v[2] == 16 for _, _, v in rows)                                          # sixteen one-tile 4x4 images per block
    assert any(d[0] == 'k3s1u0' and d[1] == '4x4' and d[6] == 'g0' and f == 'WINO' for d, f, _ in rows)   # ... which AUTO sends to F(2x2)
    assert any(f == 'WINO4' and sum(int(c) for c in d[2][1:].split('+')) % 32 != 0 for d, f, _ in rows)


def test_conv_route_matches_the_selector_cascade(tmp_path):
    libdir = os.path.join(ROOT, 'dlpm_amd', 'lib')
    exe = str(tmp_path / 'conv_route_table')
    subprocess.check_call([HIPCC, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', os.path.join(ROOT, 'tests', 'conv_route_table.cpp'),
                           '-o', exe, '-L', libdir, '-ldlpm_amd', '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib'])
    env = {k: v for k, v in os.environ.items() if not k.startswith('DLPM_')}      # the switches at their defaults
    got = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env, check=True).stdout.splitlines()
    want = _golden()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, 'row %d: conv_route gives\n  %s\nthe selector cascade gave\n  %s' % (i + 1, g, w)
    assert len(got) == len(want)
