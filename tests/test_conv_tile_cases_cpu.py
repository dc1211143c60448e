"""The tile shapes of the halo, head and stem convolution kernels, the parts that need no GPU: tests/conv_tile_table.cpp prints the route
conv_route gives every row of tests/conv_tile_cases.py (layouts attached as dlpm_conv2d_f32 would), and the same for a grid of probe
launches over every output size from 1x1 to 96x96, which holds the Python mirrors of halo_ok, head_conv_ok, head_gemm_ok and
head_fused_ok against the predicates themselves.  (launch_conv_stem chooses between its three kernels below the route: that mirror
stands on its citation alone, and the GPU test on the numbers.)  Host code only: no GPU is touched."""
import os
import subprocess

import pytest

import conv_tile_cases as T
from conftest import ROOT

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
BIG = 1 << 40         # a scratch that holds every layout


@pytest.fixture(scope='module')
def table(tmp_path_factory):
    libdir = os.path.join(ROOT, 'dlpm_amd', 'lib')
    exe = str(tmp_path_factory.mktemp('tiles') / 'conv_tile_table')
    subprocess.check_call([HIPCC, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', os.path.join(ROOT, 'tests', 'conv_tile_table.cpp'),
                           '-o', exe, '-L', libdir, '-ldlpm_amd', '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib'])
    env = {k: v for k, v in os.environ.items() if not k.startswith('DLPM_')}      # the switches at their defaults

    def ask(lines):
        """{name: (family, route name, frag_weight_floats)}"""
        out = subprocess.run([exe], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=120, env=env, check=True).stdout
        got = {}
        for ln in out.splitlines():
            name, fam, cls, frag = ln.split()
            got[name] = (fam, cls, int(frag))
        assert len(got) == len(lines)
        return got
    return ask


@pytest.fixture(scope='module')
def routes(table):
    lines = [T.descriptor_line(r) for r in T.ROWS]
    lines += [T.descriptor_line(r._replace(name=r.name + '@f32'), f32=True) for r in T.ROWS if r.kernel == 'head_fused']
    lines += [T.descriptor_line(r._replace(name=r.name + '@B1', B=1)) for r in T.ROWS]
    return table(lines)


@pytest.mark.parametrize('r', T.ROWS, ids=[r.name for r in T.ROWS])
def test_row_takes_its_route(r, routes):
    want = (T.FAMILY[r.kernel], 'conv3x3_halo' if r.kernel in ('halo_ws', 'halo') else '-')
    assert routes[r.name][:2] == want, (r.name, routes[r.name])
    assert routes[r.name + '@B1'][:2] == want                    # ... whatever the batch of the call
    if r.kernel == 'head_fused':
        assert routes[r.name + '@f32'][:2] == want
    # the class the row claims is the class the mirrors give its image
    Ho, Wo = T.out_size(r)
    if r.kernel in ('halo_ws', 'halo'):
        assert (r.ups, Wo) + T.halo_ok(Ho, Wo, r.ups, r.C0 + r.C1, r.kernel == 'halo_ws') == r.cls
        assert r.B == (r.cls[3] + 1 if r.cls[3] > 1 else 2) and r.B <= 9
        if r.kernel == 'halo':          # the scratch holds the plain copy and not the fragment copy behind it
            assert not r.ups and T.scratch_floats(r) < T.plain_floats(r) + routes[r.name][2] and T.BY_NAME[r.twin].cls == r.cls
    elif r.kernel == 'head':
        assert ('HEAD', Wo, T.head_conv_ok(Ho, Wo, r.Cout, r.C0)) == r.cls
    elif r.kernel == 'head_gemm':
        assert ('HEAD_GEMM', Wo, T.head_gemm_ok(Ho, Wo, r.Cout, r.C0)) == r.cls
    elif r.kernel == 'head_fused':
        assert ('HEAD_FUSED', Wo, T.head_fused_ok(Ho, Wo, r.Cout, r.C0)) == r.cls == ('HEAD_FUSED', Wo, T.head_fused_ok(Ho, Wo, r.Cout, r.C0, False))
        assert r.act
    else:
        assert T.stem_kernel(Ho, Wo, r.Cout) == r.cls and r.cls[0] == r.kernel and r.C0 in (1, 3) and r.bias and not r.act and r.res is None
    assert Ho * Wo <= 96 * 64 or r.name in ('stem_lds_256x4_1to64', 'stem_lds_128x8_3to128', 'stem_lds_96x32_1to64_blocks3')


def probe(name, Ho, Wo, Cout, ups=0, act=0, fd=0, C0=32, B=2):
    Hin, Win = (Ho // 2, Wo // 2) if ups else (Ho, Wo)
    return ' '.join(str(v) for v in (name, B, C0, 0, Hin, Win, Ho, Wo, Cout, ups, act, 0, 0, 1, 0, int(Cout <= 4), fd, BIG))


def test_mirrors_agree_with_the_predicates_at_every_size(table):
    """Every Hout x Wout from 1x1 to 96x96: the launch is on the halo kernels / the head family exactly where the mirror says so."""
    lines, want = [], {}
    for Ho in T.SIDES:
        for Wo in T.SIDES:
            for ups in (0, 1):
                if ups and (Ho & 1 or Wo & 1):
                    continue
                n = 'halo_%d_%d_%d' % (ups, Ho, Wo)
                lines.append(probe(n, Ho, Wo, 64, ups, fd=2))
                want[n] = ('IGEMM', 'conv3x3_halo' if T.halo_ok(Ho, Wo, ups) else 'conv3x3_igemm')
            for Cout in (1, 2, 3):
                for C0 in (32, 128):
                    for fam, fd, ok in (('HEAD', 0, T.head_conv_ok(Ho, Wo, Cout, C0)), ('HEAD_GEMM', 32, T.head_gemm_ok(Ho, Wo, Cout, C0)),
                                        ('HEAD_FUSED', 64, T.head_fused_ok(Ho, Wo, Cout, C0)),
                                        ('HEAD_FUSED', 64 | 128, T.head_fused_ok(Ho, Wo, Cout, C0, False))):
                        n = 'head_%d_%d_%d_%d_%d' % (fd, Ho, Wo, Cout, C0)
                        lines.append(probe(n, Ho, Wo, Cout, act=1, fd=fd, C0=C0, B=3))
                        want[n] = (fam, ok is not None)
    got = table(lines)
    for n, w in want.items():
        if n.startswith('halo'):
            assert got[n][:2] == w, (n, got[n])
        else:
            assert (got[n][0] == w[0]) == w[1], (n, got[n], w)


def test_coverage_counts():
    """classes enumerated, classes with a row, classes a square power-of-two image reaches -- and the 13 + 13 of halo_ok by hand"""
    halo, head, stem = T.enumerate_halo(), T.enumerate_heads(), T.enumerate_stems()
    sq_halo, sq_head, sq_stem = T.square_pow2_classes()
    rows = {r.cls for r in T.ROWS}
    by_hand = [(4, 32, 1), (4, 16, 2), (4, 8, 4), (4, 4, 8), (8, 16, 1), (8, 8, 2), (8, 4, 4), (16, 8, 1), (16, 4, 2), (16, 2, 4), (32, 4, 1),
               (32, 2, 2), (64, 2, 1)]
    assert sorted(halo) == sorted((u,) + c for u in (0, 1) for c in by_hand)
    assert (len(halo), len(rows & set(halo)), len(sq_halo)) == T.N_HALO == (26, 26, 10)
    assert (len(head), len(rows & set(head)), len(sq_head)) == T.N_HEAD == (30, 30, 9)
    assert (len(stem), len(rows & set(stem)), len(sq_stem)) == T.N_STEM == (7, 7, 4)
    assert sq_halo <= set(halo) and sq_head <= set(head) and sq_stem <= set(stem)
    assert rows == set(halo) | set(head) | set(stem)              # no row outside the enumeration
    assert sorted(c for c in head if c[0] == 'HEAD') == [('HEAD', W, TH) for W in (8, 16, 32, 64) for TH in (256 // W, 512 // W)]
    assert {c[1] for c in head if c[0] == 'HEAD_GEMM'} == set(range(16, 65, 4))       # widths 20 and 48 among them
    # the k_conv3x3_halo rows: a third of the non-upsampling classes, both classes on the LDS budget among them
    plain = {r.cls for r in T.ROWS if r.kernel == 'halo'}
    edge = {c for c in halo if T._budget_edge(c)}
    assert {c[1:] for c in edge} == {(4, 4, 8), (16, 2, 4)} and {c for c in edge if not c[0]} <= plain and len(plain) >= 13 // 3


def test_rows_rotate_over_what_a_launch_carries():
    halo = [r for r in T.ROWS if r.kernel == 'halo_ws']
    assert {T.igemm_bn(r.Cout) for r in halo} == {128, 64, 32}
    assert sum(r.Cout == 96 for r in halo) >= 2 and sum(r.Cout == 192 for r in halo) >= 1
    assert {r.res for r in halo} == {None, 'one', 16} and any(r.act for r in halo) and any(not r.bias for r in halo)
    assert any(r.C1 for r in halo) and any(not r.C1 for r in halo)
    assert sum(r.out_nchw and r.Cout == 3 for r in halo) == 2
    tiles = lambda r: T.out_size(r)[0] // r.cls[2]
    for ups in (0, 1):
        assert {tiles(r) for r in halo if r.ups == ups and r.cls[3] == 1} >= {3, 5}
    for k in ('head', 'head_gemm', 'head_fused'):
        assert {tiles(r) for r in T.ROWS if r.kernel == k} >= {2}
    assert {tiles(r) for r in T.ROWS if r.kernel in ('head', 'head_fused')} >= {2, 3}
    assert all(r.B == 3 for r in T.ROWS if r.kernel.startswith(('head', 'stem')))


def test_weight_stream_reads_stay_inside_the_fragment_copy(routes):
    """k_conv3x3_halo_ws<BN> streams BN / 32 n-blocks per tile whether the layer has those channels or not: the copy is padded to whole
    BN tiles.  (Before, frag_weight_floats counted ceil(Cout / 32) n-blocks, and the last tile of a Cout = 96, 160 or 192 layer read
    36 KB (Cin / 32) per missing n-block past it.)"""
    seen = set()
    for r in T.ROWS:
        if r.kernel != 'halo_ws':
            continue
        Cin = r.C0 + r.C1
        last, have = T.frag_last_float_read(r.Cout, Cin), routes[r.name][2]
        assert last < have, (r.name, last, have)
        assert have - last <= 2 * 256, r.name            # ... and the copy is no larger than the stream + its two groups of padding
        seen.add(r.Cout)
    assert {32, 64, 96, 128, 192, 3} <= seen
