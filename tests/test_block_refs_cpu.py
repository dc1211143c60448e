"""tests/block_refs.py on the CPU: the float64 references reproduce the recorded fixtures, the sharp and cancellation cases are what
they claim to be, the judge rejects outputs that are subtly wrong at the bounds tests/test_gpu_fused_blocks.py asserts, and the
oracle's float64 net forward (the reference of the in-net test there) agrees with its fp32 one."""
import pytest
import torch
import torch.nn.functional as F

import block_refs as R
import small_block_weights as sbw
from conftest import golden
from oracle import nets


def _ss(sd, emb):
    return F.linear(nets.silu(emb), sd['emb_layers.1.weight'], sd['emb_layers.1.bias'])


def test_float64_references_reproduce_the_recorded_fixtures():
    """Every recorded output the seven whole-block tests of test_gpu_kernels.py use (F13, F14): measured at most 3.49e-6 (ResBlocks)
    and 6.75e-7 (AttentionBlocks), the fp32 rounding of the recording; the bounds are 7e-6 and 1.4e-6."""
    f13, f14 = golden('f13_small_blocks'), golden('f14_blocks16')
    res, att = [], []
    for cin, hs in [(64, 8), (64, 4), (128, 8), (128, 4)]:
        tag, sd = 'res_c%d_h%d_' % (cin, hs), sbw.res_state(cin, hs)
        x, emb = torch.from_numpy(f13[tag + 'x']), torch.from_numpy(f13[tag + 'emb'])
        res.append((tag, (R.res_block64(sd, x, _ss(sd, emb)) - torch.from_numpy(f13[tag + 'y'])).abs().max().item()))
    for cin, co, hs, B in [(64, 64, 16, 2), (128, 64, 16, 2), (96, 64, 16, 2), (32, 32, 32, 1), (64, 32, 32, 1), (96, 32, 32, 1)]:
        tag, sd = 'res_c%d_o%d_h%d_' % (cin, co, hs), sbw.res_fine_state(cin, co, hs)
        x, emb = sbw.res_fine_input(cin, hs, B)
        res.append((tag, (R.res_block64(sd, x, _ss(sd, emb)) - torch.from_numpy(f14[tag + 'y'])).abs().max().item()))
    for hs in (8, 4):
        tag = 'attn_h%d_' % hs
        got = R.attn_block64(sbw.attn_state(hs), torch.from_numpy(f13[tag + 'x']), 4)[0]
        att.append((tag, (got - torch.from_numpy(f13[tag + 'y'])).abs().max().item()))
    att.append(('attn_h16_', (R.attn_block64(sbw.attn16_state(), sbw.attn16_input(), 4)[0] - torch.from_numpy(f14['attn_h16_y'])).abs().max().item()))
    print(res, att)
    assert max(e for _, e in res) < 7e-6, res
    assert max(e for _, e in att) < 1.4e-6, att


def test_the_case_list_covers_what_it_says():
    assert len(R.CASES) == len(R.BENIGN) + len(R.CANCEL) == 86
    for k in R.KERNELS:
        assert any(R.CASES[n][0] == k for n in R.BENIGN) and any(R.CASES[n][0] == k for n in R.CANCEL), k
    for c0, c1 in R.RES_SMALL_SPLITS:
        assert c0 % 4 == 0 and c1 % 4 == 0 and c0 + c1 in (64, 128)
    for c0, c1 in R.RES_IMG32_SPLITS + R.RES_IMG16_SPLITS:
        assert c0 % 32 == 0 and c1 % 32 == 0 and 32 <= c0 + c1 <= 128
    assert (32, 32) not in R.RES_IMG16_SPLITS       # refused: test_gpu_fused_blocks.py::test_refusals


@pytest.mark.parametrize('name', [n for n in R.CASES if R.CASES[n][4] != 'benign'])
def test_conditions(name):
    """sharp: at least 15 % of the softmax rows have a logit above 89 (fp32 exp overflows), at least 15 % are not one-hot
    (pmax < 0.99), some row lies wholly below -40.  cancel_gn1 / cancel_gn2: every group GroupNorm sees has |mean| > 100 std.
    cancel_out: every output channel has |mean| = 100 +- 1.5 and std < 0.2 (the statistics the block emits)."""
    c = R.conditions(name)
    print(name, c)
    kind = R.CASES[name][4]
    if kind == 'sharp':
        assert c['over89'] >= 0.15 and c['soft'] >= 0.15 and c['min_rowmax'] < -40
    elif kind in ('cancel_gn1', 'cancel_gn2'):
        assert c['mean_over_std'] > 100
    else:
        assert kind == 'cancel_out' and c['mean_abs_min'] > 98.5 and c['mean_abs_max'] < 101.5 and c['std_max'] < 0.2


def _gn_scaled(c, f):
    keys = ['in_layers.0.weight', 'out_layers.0.weight'] if c.is_res else ['norm.weight']
    return c.with_sd({k: f * c.sd[k] for k in keys})


@pytest.mark.parametrize('name', R.BENIGN)
def test_judge_rejects_a_wrong_block_benign(name):
    """The float64 block with every GroupNorm weight 0.1 % too large is rejected at the kernel's bound (and at the cap); the reference
    itself scores 0, the fp32 oracle 1.  Sharp cases: a softmax without max subtraction in fp32 is not finite, and rejected."""
    c = R.case(name)
    want, ref32, _ = R.refs(name)
    assert R.ratio(name, want) == 0.0 and R.ratio(name, ref32) == 1.0
    r = R.ratio(name, c.want64(_gn_scaled(c, 1.001)))
    print('%s: ratio of a block with GroupNorm weights x 1.001 = %.1f (bound %.2f)' % (name, r, R.M_BOUND[c.kernel][0]))
    assert r > R.M_CAP >= R.M_BOUND[c.kernel][0]
    if c.kind == 'sharp':
        with torch.no_grad():
            bad = R.softmax_no_max_fp32(c.sd, c.x, R.HEADS)
        assert not bool(torch.isfinite(bad).all())
        assert R.ratio(name, bad) == float('inf')


@pytest.mark.parametrize('name', R.CANCEL)
def test_judge_rejects_a_wrong_block_cancel(name):
    """... and with the weights 1 % too large in every cancellation case (whose bound includes the coefficient-form floor)."""
    c = R.case(name)
    want, ref32, floor = R.refs(name)
    assert floor is not None and R.ratio(name, want) == 0.0 and R.ratio(name, ref32) <= 1.0 and R.ratio(name, floor) <= 1.0
    r = R.ratio(name, c.want64(_gn_scaled(c, 1.01)))
    print('%s: ratio of a block with GroupNorm weights x 1.01 = %.1f (bound %.2f)' % (name, r, R.M_BOUND[c.kernel][1]))
    assert r > R.M_CAP >= R.M_BOUND[c.kernel][1]


def test_fp32_oracle_is_unchanged_by_the_float64_path():
    """A float64 input keeps its type through every oracle function the references use; an fp32 one gives fp32 (the bits of
    test_oracle_golden.py / test_geometry_cpu.py)."""
    t = torch.tensor([0.25, 0.5])
    assert nets.timestep_embedding(t, 8).dtype == torch.float32 and nets.timestep_embedding(t.double(), 8).dtype == torch.float64
    x = torch.randn(2, 64, 4, 4, generator=torch.Generator().manual_seed(0))
    w, b = torch.ones(64), torch.zeros(64)
    assert nets.group_norm(x, w, b).dtype == torch.float32 and nets.group_norm(x.double(), w.double(), b.double()).dtype == torch.float64
    assert nets.group_norm(x.half(), w, b).dtype == torch.float32
    assert (nets.group_norm(x.double(), w.double(), b.double()) - R.gn_exact(x.double(), w, b)).abs().max().item() < 1e-13


def test_float64_net_forward():
    """unet_forward in float64 on the `mnist` net at B = 2: every feature and the output are float64 and within 1e-5 of the fp32
    forward (measured: at most 2.9e-6)."""
    _, sd, x, t = R.net_case()
    f32, f64 = R.net_forwards(sd, x, t)
    assert len(f32) == len(f64) == 26
    errs = []
    for (n, a), (_, b) in zip(f32, f64):
        assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape, n
        errs.append((a.double() - b).abs().max().item())
    print(' '.join('%.2e' % e for e in errs))
    assert max(errs) < 1e-5 and min(errs) > 0, errs
