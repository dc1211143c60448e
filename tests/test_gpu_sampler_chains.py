"""The sampler step as two half-batch chains of kernels in one captured graph: bit-identity to the one-chain step, to
the two shards, graph == eager, reseed / set_state without a recapture, the variants that stay on one chain, and the layout of the
two arenas.  DLPM_SAMPLER_CHAINS is read once per process: each setting runs every scenario ONCE in a child process
(sampler_chains_child.py) and the tests compare what the two children stored.  Tiny UNet, 3 x 16 x 16 images, T = 9."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dlpm_amd import _lib

pytestmark = pytest.mark.gpu
BATCHES = (4, 5, 2)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp('chains')
    out = {}
    for setting in ('1', '2'):
        path = str(d / ('chains%s.npz' % setting))
        env = dict(os.environ, DLPM_SAMPLER_CHAINS=setting)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'sampler_chains_child.py'), path], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out[int(setting)] = dict(np.load(path))
    return out


@pytest.mark.parametrize('B', BATCHES)
def test_two_chains_equal_one_chain_bit_for_bit(runs, B):
    """8 steps with the graph on, same seed: B = 4, B = 5 (2 + 3 rows) and B = 2 (one sample per chain)."""
    one, two = runs[1], runs[2]
    assert tuple(one['info_B%d' % B]) == (1, 1)          # (chains, graphs captured)
    assert tuple(two['info_B%d' % B]) == (2, 1)
    assert np.isfinite(two['full_B%d' % B]).all()
    assert np.array_equal(one['full_B%d' % B], two['full_B%d' % B])


@pytest.mark.parametrize('B', BATCHES)
def test_two_chains_equal_the_two_shards(runs, B):
    """rows [0, B/2) and the rest == two separate samplers of those sizes with sample_offset 0 and B/2, all under the declared
    dispatch batch B -- the shards of either setting (a shard of 2 or 3 rows is itself chained under DLPM_SAMPLER_CHAINS=2)."""
    full = runs[2]['full_B%d' % B]
    for setting in (1, 2):
        lo, hi = runs[setting]['shard_lo_B%d' % B], runs[setting]['shard_hi_B%d' % B]
        assert lo.shape[0] == B // 2 and hi.shape[0] == B - B // 2
        assert np.array_equal(np.concatenate([lo, hi]), full)
    assert not np.array_equal(full[0], full[B // 2])       # (the chains drew their own noise)


def test_graph_equals_eager(runs):
    for setting in (1, 2):
        assert np.array_equal(runs[setting]['eager_B4'], runs[setting]['full_B4'])


def test_reseed_and_set_state_keep_the_graph(runs):
    """After dlpm_sampler_reseed to (seed 7, sample_offset 3) the next steps equal a fresh sampler's, a trajectory resumed with
    set_state under the new key too, and neither captured a second graph nor moved the plan version."""
    for setting in (1, 2):
        r = runs[setting]
        cap0, cap1, ver0, ver1, chains = (int(v) for v in r['reseed_counters'])
        assert chains == setting
        assert cap0 == 1 and cap1 == 1 and ver0 == ver1
        assert np.array_equal(r['native_first'], r['full_B4'])
        assert not np.array_equal(r['reseeded'], r['native_first'])
        assert np.array_equal(r['reseeded'], r['fresh_reseeded'])
        assert np.array_equal(r['resumed'], r['fresh_reseeded'])
    assert np.array_equal(runs[1]['reseeded'], runs[2]['reseeded'])


@pytest.mark.parametrize('name', ['clip', 'label', 'one'])
def test_variants_that_stay_on_one_chain(runs, name):
    """a clip sampler, a label-conditional sampler and B = 1 run with DLPM_SAMPLER_CHAINS=2 set, on one chain, with the same bits"""
    assert int(runs[2]['info_' + name][0]) == 1
    assert np.isfinite(runs[2][name]).all()
    assert np.array_equal(runs[1][name], runs[2][name])


@pytest.mark.parametrize('B', BATCHES)
def test_the_two_arenas_are_disjoint_and_inside_the_allocation(B):
    """host arithmetic of the sizing function: no kernel runs"""
    from sampler_chains_child import tiny
    net = tiny()
    net.set_conv_policy('auto', B)
    L, h = _lib.lib(), net.native_handle(16)
    i64x2 = C.c_int64 * 2
    r0, n, off, size, single, slack = i64x2(), i64x2(), i64x2(), i64x2(), C.c_int64(), C.c_int64()
    both = L.dlpm_unet_chain_workspace(h, B, 2, r0, n, off, size, C.byref(single), C.byref(slack))
    print('B = %d: arenas %d + %d = %d bytes, single arena %d, rounding slack %d' % (B, size[0], size[1], both, single.value,
                                                                                    slack.value))
    assert list(r0) == [0, B // 2] and list(n) == [B // 2, B - B // 2]
    assert single.value == L.dlpm_unet_workspace_bytes(h, B)
    assert [size[c] for c in range(2)] == [L.dlpm_unet_workspace_bytes(h, n[c]) for c in range(2)]
    assert off[0] == 0 and off[1] >= off[0] + size[0] and off[1] % 256 == 0          # disjoint, block-aligned
    assert both == off[1] + size[1]                                                    # and the sum is all the sampler allocates
    assert 0 < slack.value and both <= single.value + slack.value
    assert L.dlpm_unet_chain_workspace(h, 1, 2, r0, n, off, size, None, None) == -1    # fewer rows than chains
