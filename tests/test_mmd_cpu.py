"""MMD without a GPU: the fp64 numpy restatement that stands in for the reference where the reference cannot run (unequal counts)
held to the reference's own fp64 results (fixture family F18), the quadrant identity behind `return_parts`, and the refusals of the
two C entry points and of the Python functions -- all of which happen before anything touches a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden
import dlpm_amd
from dlpm_amd import _lib, metrics
from metric_helpers import buffers

DIRECT = ['toy64', 'toy257', 'toy257_same', 'toy1000', 'd3', 'd16', 'params_k3', 'params_sigma']   # D <= 16
GRAM = ['d17', 'g147', 'g192', 'g3072_img']                                                        # D > 16
CASES = DIRECT + GRAM


def case(name):
    f = golden('f18_mmd_' + name)
    kw = dict(kernel_mul=float(f['kernel_mul']), kernel_num=int(f['kernel_num']), fix_sigma=float(f['fix_sigma']) or None)
    return f, kw


def np_mmd(x, y, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """bem/evaluate/mmd_loss.py:13-37 in fp64 numpy, with the normalisation generalised to n1 != n2.
    Returns (mmd, bandwidth before the ladder's division, sum XX, sum YY, sum XY)."""
    x, y = np.asarray(x, np.float64).reshape(len(x), -1), np.asarray(y, np.float64).reshape(len(y), -1)
    n1, n2 = len(x), len(y)
    p = np.concatenate([x, y])
    n = n1 + n2
    l2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(2)
    bw = fix_sigma if fix_sigma else l2.sum() / (n * n - n)
    b0 = bw / kernel_mul ** (kernel_num // 2)
    k = sum(np.exp(-l2 / (b0 * kernel_mul ** q)) for q in range(kernel_num))
    xx, yy, xy = k[:n1, :n1].sum(), k[n1:, n1:].sum(), k[:n1, n1:].sum()
    return xx / n1 ** 2 + yy / n2 ** 2 - 2.0 * xy / (n1 * n2), bw, xx, yy, xy


def unequal_case(n1, n2, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n1, D, generator=g), torch.randn(n2, D, generator=g) + 0.3


@pytest.mark.parametrize('name', CASES)
def test_restatement_equals_the_reference_in_fp64(name):
    f, kw = case(name)
    got = np_mmd(f['x'], f['y'], **kw)
    assert abs(got[0] - float(f['ref64'])) <= 1e-12, (got[0], float(f['ref64']))
    assert abs(got[1] - float(f['bandwidth64'])) <= 1e-12 * float(f['bandwidth64'])


@pytest.mark.parametrize('name', ['toy257', 'g147'])
def test_quadrant_identity_of_return_parts(name):
    """mean(XX + YY - XY - YX) of the reference is sum XX / n1^2 + sum YY / n2^2 - 2 sum XY / (n1 n2) at n1 == n2."""
    f, kw = case(name)
    m, bw, xx, yy, xy = np_mmd(f['x'], f['y'], **kw)
    n1, n2 = len(f['x']), len(f['y'])
    assert abs(xx / n1 ** 2 + yy / n2 ** 2 - 2 * xy / (n1 * n2) - float(f['ref64'])) <= 1e-12
    # and at unequal counts each quadrant is a mean of its own
    x, y = unequal_case(64, 80, 2, 5)
    m, bw, xx, yy, xy = np_mmd(x, y)
    assert 0 < m < 2 * 5 and xx <= 64 * 64 * 5 and yy <= 80 * 80 * 5 and xy <= 64 * 80 * 5


def test_fixtures_are_small_and_complete():
    for name in CASES:
        f, _ = case(name)
        assert set(f.files) >= {'x', 'y', 'ref32', 'ref64', 'bandwidth32', 'bandwidth64', 'kernel_num', 'kernel_mul', 'fix_sigma'}
        assert f['x'].dtype == np.float32 and f['y'].dtype == np.float32 and f['ref64'].dtype == np.float64
        assert (f['x'].shape[1] > 16) == (name in GRAM)


def test_workspace_bytes_refusals():
    L = _lib.lib()
    for n1, n2, D in [(0, 4, 2), (4, 0, 2), (4, 4, 0), (-1, 4, 2)]:
        assert L.dlpm_mmd_workspace_bytes(n1, n2, D) == -1
        assert b'bad shape' in L.dlpm_last_error()
    assert L.dlpm_mmd_workspace_bytes(64, 64, 2) > 0
    assert L.dlpm_mmd_workspace_bytes(64, 64, 3072) > L.dlpm_mmd_workspace_bytes(64, 64, 2)     # mean, column partials, row norms
    # 46341^2 overflows 32 bits: the tile count and the workspace size are 64-bit
    big = L.dlpm_mmd_workspace_bytes(3000000, 3000000, 2)
    side = -(-6000000 // 128)
    tiles = side * (side + 1) // 2
    assert big >= tiles * 24 > 2 ** 31


def test_mmd_f32_refuses_before_any_launch():
    """No GPU here: every one of these returns before a kernel is launched (the pointers are host addresses, never followed)."""
    L = _lib.lib()
    buf, base = buffers()
    x, y, ws, out = base, base + 4096, base + 8192, base + 60000 // 8 * 8
    need = L.dlpm_mmd_workspace_bytes(8, 8, 2)
    good = dict(x=x, n1=8, y=y, n2=8, D=2, mul=2.0, num=5, sigma=0.0, ws=ws, wsb=need, out=out)

    def call(**over):
        a = dict(good, **over)
        return L.dlpm_mmd_f32(a['x'], a['n1'], a['y'], a['n2'], a['D'], a['mul'], a['num'], a['sigma'], a['ws'], a['wsb'], a['out'], None)

    for over, word in [(dict(n1=0), 'bad shape'), (dict(n2=0), 'bad shape'), (dict(D=0), 'bad shape'), (dict(num=0), 'kernel_num'),
                       (dict(num=17), 'kernel_num'), (dict(mul=0.0), 'kernel_mul'), (dict(mul=-2.0), 'kernel_mul'),
                       (dict(x=None), 'null'), (dict(y=None), 'null'), (dict(ws=None), 'null'), (dict(out=None), 'null')]:
        with pytest.raises(ValueError, match=word):
            _lib.check(call(**over))
    with pytest.raises(_lib.DlpmError, match='workspace'):
        _lib.check(call(wsb=need - 1))
    assert call(wsb=need - 1) == -5          # DLPM_ERR_NOMEM


def test_python_refusals():
    x = torch.zeros(4, 2)
    for bad, word in [((x.double(), x), 'float32'), ((x, x.to(torch.float16)), 'float32'), ((x, torch.zeros(4, 3)), 'values'),
                      ((torch.zeros(0, 2), x), 'at least one point'), ((np.zeros((4, 2), np.int64), x), 'float32')]:
        with pytest.raises(AssertionError, match=word):
            metrics.mmd(*bad)
    for kw, word in [(dict(kernel_num=0), 'kernel_num'), (dict(kernel_num=17), 'kernel_num'), (dict(kernel_num=2.5), 'kernel_num'),
                     (dict(kernel_mul=0.0), 'kernel_mul'), (dict(kernel_mul=-1.0), 'kernel_mul'), (dict(fix_sigma=-0.5), 'fix_sigma')]:
        with pytest.raises(AssertionError, match=word):
            metrics.mmd(x, x, **kw)
    loss = dlpm_amd.MMD_loss(kernel_mul=3.0, kernel_num=3)
    assert (loss.kernel_mul, loss.kernel_num, loss.fix_sigma) == (3.0, 3, None) and isinstance(loss, torch.nn.Module)
    assert dlpm_amd.mmd is metrics.mmd
    with pytest.raises(AssertionError, match='float32'):
        loss(x.double(), x)


def test_evaluate_mmd_refusals():
    ev = dlpm_amd.EvaluationManager(None, None, None, verbose=False)
    with pytest.raises(AssertionError, match='float32'):
        ev.evaluate_mmd({}, np.zeros((8, 1, 2)), 8, 4)
    with pytest.raises(AssertionError, match='real samples'):
        ev.evaluate_mmd({}, np.zeros((4, 1, 2), np.float32), 8, 4)
    assert ev.evals['mmd'] == []
