"""Geometries beyond the four shipped configs on the MI355X: the general attention kernel (any token count 1..4096, any head dim
1..256) through dlpm_attention_f32 / dlpm_attention_general_f32, and the 28x28 MNIST UNet of dlpm_amd/configs/mnist28.yml (attention
at 14x14 / 7x7, stride-2 downsample 14 -> 7, upsample 7 -> 14) end to end: forward, sampler, GenerationManager and the CLI's PNG dump."""
import functools
import math
import os
import struct

import numpy as np
import pytest
import torch

from conftest import golden
import dlpm_amd
from dlpm_amd import _lib
from dlpm_amd.weights import state_digest
from oracle import nets, process as P

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GENERATIONS = ['auto', 'f4', 'f2', 'igemm']


def attention(qkv, heads, general=False):
    """qkv: [B, heads * 3 ch, T] (the reference's layout before its reshape) -> HIP result [B, heads * ch, T] on the CPU."""
    B, C3, T = qkv.shape
    C = C3 // 3
    x = qkv.permute(0, 2, 1).contiguous().to(DEV)
    out = torch.empty(B, T, C, device=DEV)
    fn = _lib.lib().dlpm_attention_general_f32 if general else _lib.lib().dlpm_attention_f32
    _lib.check(fn(x.data_ptr(), out.data_ptr(), B, T, C, heads, _lib.stream_ptr()))
    return out.cpu().permute(0, 2, 1)


def attention_fp64(qkv, heads):
    """Independent full-tensor reference: QKVAttention (unet.py:236-250) in fp64, on the GPU for speed."""
    B, C3, T = qkv.shape
    x = qkv.to(DEV, torch.float64).reshape(B * heads, C3 // heads, T)
    ch = x.shape[1] // 3
    q, k, v = x[:, :ch], x[:, ch:2 * ch], x[:, 2 * ch:]
    w = torch.softmax(torch.einsum('bct,bcs->bts', q, k) / math.sqrt(ch), dim=-1)
    return torch.einsum('bts,bcs->bct', w, v).reshape(B, heads * ch, T).cpu()


def tol(T):
    return 3e-6 if T < 1024 else 1e-5


@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('ch,T', [(16, 49), (16, 196), (8, 784), (8, 4), (32, 1024), (24, 100), (256, 64)])
def test_attention_against_f15(ch, T, general):
    f = golden('f15_attention_any')
    qkv = torch.from_numpy(f['ch%d_T%d_in' % (ch, T)].astype(np.float32))     # [heads, 3 ch, T] with b = 1
    heads = qkv.shape[0]
    got = attention(qkv.reshape(1, heads * 3 * ch, T), heads, general).reshape(heads, ch, T)
    err = float((got - torch.from_numpy(f['ch%d_T%d_out' % (ch, T)])).abs().max())
    print('attention ch %d T %d (%s): max |hip - reference| = %.3g' % (ch, T, 'general' if general else 'dispatch', err))
    assert err < tol(T)


@pytest.mark.parametrize('ch', [8, 16, 24, 32, 64, 128, 256])
@pytest.mark.parametrize('T', [1, 3, 15, 17, 49, 100, 196, 784, 1024, 4096])
def test_attention_sweep_against_fp64(T, ch):
    B, heads = (2, 2) if T * ch >= 1024 * 128 else (3, 3)
    g = torch.Generator().manual_seed(T * 1000 + ch)
    qkv = torch.randn(B, heads * 3 * ch, T, generator=g)
    want = attention_fp64(qkv, heads)
    got = attention(qkv, heads)
    err = float((got.double() - want).abs().max())
    assert torch.isfinite(got).all()
    if T >= 1024:
        print('attention T %d ch %d: max |hip - fp64| = %.3g' % (T, ch, err))
    assert err < tol(T), (T, ch, err)
    # and the scalar-load path: the same data at a row offset that is not 16-byte aligned
    if ch % 4 == 0 and T <= 784:
        B_, C3 = B, heads * 3 * ch
        buf = torch.empty(B_ * T * C3 + 1, device=DEV)
        x = buf[1:].view(B_, T, C3)
        x.copy_(qkv.permute(0, 2, 1))
        ob = torch.empty(B_ * T * heads * ch + 1, device=DEV)
        o = ob[1:].view(B_, T, heads * ch)
        _lib.check(_lib.lib().dlpm_attention_general_f32(x.data_ptr(), o.data_ptr(), B_, T, heads * ch, heads, _lib.stream_ptr()))
        err2 = float((o.cpu().permute(0, 2, 1).double() - want).abs().max())
        assert err2 < tol(T), (T, ch, err2)


@pytest.mark.parametrize('ch', [1, 3, 6, 10, 50, 130, 255])
@pytest.mark.parametrize('T', [5, 70, 300])
def test_attention_odd_head_dims_against_fp64(T, ch):
    """Head dims that are no multiple of 4: scalar loads, zero padding up to the next of 16 / 32 / 64 / 128 / 256."""
    B, heads = 2, 3
    g = torch.Generator().manual_seed(T * 1000 + ch + 1)
    qkv = torch.randn(B, heads * 3 * ch, T, generator=g)
    err = float((attention(qkv, heads).double() - attention_fp64(qkv, heads)).abs().max())
    assert err < 3e-6, (T, ch, err)


@pytest.mark.parametrize('ch', [16, 32, 256])
def test_attention_online_softmax_rescale_is_exercised(ch):
    """Rule: a rare data-dependent branch needs its own test.  The running max of a query row must jump in a LATE key block (the
    rescale of O and of the running sum by exp(m_old - m_new)) and also in the FIRST block: one K row is spiked against one Q row in
    each place, so that the spiked key dominates that row's softmax.  Compared over the full tensor with an fp64 host result."""
    T, B, heads = 300, 2, 2             # key blocks of 64 (32 for ch 256): keys 5 and 250 lie in the first and in a late block
    g = torch.Generator().manual_seed(26)
    qkv = torch.randn(B, heads, 3, ch, T, generator=g)
    for b, h, q_row, k_row in [(0, 0, 100, 250), (1, 1, 7, 5), (0, 1, 299, 290), (1, 0, 0, 299)]:
        qv = qkv[b, h, 0, :, q_row]
        # score = q.k / sqrt(ch) = 20 for this pair, against O(1) for every other one
        qkv[b, h, 1, :, k_row] = qv * (20.0 * ch ** 0.5 / float(qv.dot(qv)))
    qkv = qkv.reshape(B, heads * 3 * ch, T)
    want = attention_fp64(qkv, heads)
    w = want.reshape(B, heads, ch, T)
    # the spiked rows really are dominated by their spiked key (the rescale branch moved the whole row)
    v = qkv.reshape(B, heads, 3, ch, T)[:, :, 2].double()
    assert float((w[0, 0, :, 100] - v[0, 0, :, 250]).abs().max()) < 1e-3
    for general in (False, True):
        got = attention(qkv, heads, general)
        err = float((got.double() - want).abs().max())
        assert err < 3e-6, (general, err)


@pytest.mark.parametrize('ch', [16, 32, 64, 128])
@pytest.mark.parametrize('T', [16, 64, 256])
def test_general_kernel_matches_the_specialised_one_at_the_shipped_shapes(T, ch):
    B, heads = 3, 2
    g = torch.Generator().manual_seed(7 * T + ch)
    qkv = torch.randn(B, heads * 3 * ch, T, generator=g)
    a, b = attention(qkv, heads), attention(qkv, heads, general=True)
    want = attention_fp64(qkv, heads)
    assert float((a - b).abs().max()) < 3e-6
    assert float((b.double() - want).abs().max()) < 3e-6


def test_head_dim_above_256_is_refused():
    x = torch.zeros(1, 4, 3 * 260, device=DEV)
    o = torch.empty(1, 4, 260, device=DEV)
    with pytest.raises(_lib.DlpmError, match='head dim 260'):
        _lib.check(_lib.lib().dlpm_attention_f32(x.data_ptr(), o.data_ptr(), 1, 4, 260, 1, _lib.stream_ptr()))


# ---------------------------------------------------------------- the 28x28 MNIST net (BASELINE configs[1] as written)
def mnist28_net(head_scale=1.0):
    p = dlpm_amd.load_config('mnist28')
    torch.manual_seed(1234)
    net = dlpm_amd.init_model_by_parameter(p)
    dlpm_amd.rerandomize_(net, 4321)
    if head_scale != 1.0:
        with torch.no_grad():
            getattr(net.out, '2').weight.mul_(head_scale)
            getattr(net.out, '2').bias.mul_(head_scale)
    return net


@pytest.mark.parametrize('gemm', ['bf16x3', 'f32'])
@pytest.mark.parametrize('gen', GENERATIONS)
def test_mnist28_forward_against_reference(gen, gemm):
    f = golden('f15_unet_mnist28')
    net = mnist28_net()
    assert state_digest(net) == bytes(f['digest_final']).hex()
    net.set_conv_policy(gen)
    net.set_gemm_policy(gemm)
    x = torch.from_numpy(f['x']).to(DEV)
    y = net(x, torch.from_numpy(f['t']).to(DEV)).cpu().numpy()
    y2 = net(x, torch.from_numpy(f['t_same']).to(DEV)).cpu().numpy()
    err = max(float(np.abs(y - f['y']).max()), float(np.abs(y2 - f['y_same_t']).max()))
    print('mnist28 forward (%s, %s): max |hip - reference| = %.3g' % (gen, gemm, err))
    assert err < 1e-4


@pytest.mark.parametrize('mult,attn', [([1, 2, 2, 2], [1, 2, 4]),          # attention at 32x32: T = 1024, head dim 8
                                       ([1, 2, 2, 2, 2], [16])])           # 5 levels: attention at 2x2, T = 4
def test_32x32_nets_with_new_attention_shapes_against_oracle(mult, attn):
    torch.manual_seed(1234)
    net = dlpm_amd.UNetModel(1, 32, 1, 2, attn, channel_mult=mult, num_heads=4, use_scale_shift_norm=True)
    dlpm_amd.rerandomize_(net, 4321)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(77)
    x = torch.randn(3, 1, 32, 32, generator=g)
    t = torch.rand(3, generator=g)
    with torch.no_grad():
        want = nets.unet_forward(sd, x, t, 4).numpy()
    for gen in ('auto', 'igemm'):
        net.set_conv_policy(gen)
        got = net(x.to(DEV), t.to(DEV)).cpu().numpy()
        err = float(np.abs(got - want).max())
        print('32x32 net %s attn %s (%s): max |hip - oracle| = %.3g' % (mult, attn, gen, err))
        assert err < 1e-4


ODD_NETS = {
    # 48x48: F(4x4) with 3 blocks per row, the 24 -> 48 upsample on the UPS instantiation, 24x24 / 12x12 / 6x6 on the generic implicit GEMM;
    # attention at T = 576 and 144
    '48x48': (48, [1, 2, 2, 2]),
    # 20x20: a 5x5 level, stride-2 10 -> 5 and upsample 5 -> 10; attention at T = 100 and 25
    '20x20': (20, [1, 2, 2]),
}


@functools.lru_cache(maxsize=None)
def odd_net(name):
    """(net, x, t, the oracle's forward on the CPU), computed once and shared by every generation and GEMM policy"""
    size, mult = ODD_NETS[name]
    torch.manual_seed(1234)
    net = dlpm_amd.UNetModel(1, 32, 1, 2, [2, 4], channel_mult=mult, num_heads=4, use_scale_shift_norm=True)
    dlpm_amd.rerandomize_(net, 4321)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(77)
    x = torch.randn(3, 1, size, size, generator=g)
    t = torch.rand(3, generator=g)
    with torch.no_grad():
        want = nets.unet_forward(sd, x, t, 4).numpy()
    return net, x, t, want


@pytest.mark.parametrize('gemm', ['bf16x3', 'f32'])
@pytest.mark.parametrize('gen', GENERATIONS)
@pytest.mark.parametrize('name', list(ODD_NETS))
def test_48x48_and_20x20_nets_against_oracle(name, gen, gemm):
    """image_size is a free value of the reference's configs: two nets whose levels are no power of two, B = 3, under every
    generation and both GEMM policies, against the oracle (the bound of test_32x32_nets_with_new_attention_shapes_against_oracle)."""
    net, x, t, want = odd_net(name)
    net.set_conv_policy(gen)
    net.set_gemm_policy(gemm)
    got = net(x.to(DEV), t.to(DEV)).cpu().numpy()
    assert np.isfinite(got).all()
    err = float(np.abs(got - want).max())
    print('%s net (%s, %s): max |hip - oracle| = %.3g' % (name, gen, gemm, err))
    assert err < 1e-4


@pytest.mark.parametrize('gemm', ['bf16x3', 'f32'])
@pytest.mark.parametrize('gen', GENERATIONS)
def test_mnist28_bounded_trajectory_against_reference(gen, gemm):
    """A bounded (clip_denoised) reference sample() of the 28x28 net at T = 1000, alpha = 1.7, on the reference's streams; the
    recorded states within 1e-4 and the GenerationManager-post-processed pixels within 1e-4 absolute."""
    f = golden('f15_traj_unet_mnist28_clip_T1000')
    net = mnist28_net(float(f['head_scale']))
    assert state_digest(net) == bytes(f['digest']).hex()
    net.set_conv_policy(gen)
    net.set_gemm_policy(gemm)
    T, alpha, ca, ce = f['meta']
    meth = dlpm_amd.GenerativeLevyProcess(float(alpha), DEV, int(T), rescale_timesteps=True, rng='reference', seed=0)
    x, hist = meth.sample({'default': net}, [int(v) for v in f['shape']], int(T), clamp_a=float(ca), clamp_eps=float(ce),
                          clip_denoised=True, get_sample_history=True)
    err_state = float(np.abs(hist[::int(f['every'])].cpu().numpy() - f['history_sub']).max())
    gm = dlpm_amd.GenerationManager(None, None, True)
    got = gm._post(x).numpy()
    want = P.generation_postprocess(torch.from_numpy(f['final']), True).numpy()
    err = float(np.abs(got - want).max())
    print('mnist28 trajectory (%s, %s): states %.3g, post-processed pixels %.3g (fixture sensitivity %.3g)'
          % (gen, gemm, err_state, err, float(f['sensitivity'])))
    meth.close()
    assert err_state < 1e-4 * max(1.0, float(np.abs(f['history_sub']).max()))
    assert err < 1e-4


def test_mnist28_sampler_graph_vs_eager_and_chunking():
    """Philox sampling of the 28x28 net: the captured-graph loop equals the eager one bit for bit, and under a declared batch the
    samples do not depend on the chunking (B = 4 gives the first 4 samples of B = 8)."""
    net = mnist28_net(4.0)
    net.set_conv_policy('auto', 8)
    T, alpha = 50, 1.7

    def run(B, graph):
        m = dlpm_amd.GenerativeLevyProcess(alpha, DEV, T, rescale_timesteps=True, seed=3, use_graph=graph)
        x = m.sample({'default': net}, [B, 1, 28, 28], T, clamp_a=20, clamp_eps=200, clip_denoised=True).cpu()
        m.close()
        return x
    a, b, c = run(8, True), run(8, False), run(4, True)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), 'graph and eager sampling differ'
    assert torch.equal(c, a[:4]), 'samples depend on the chunking'


def test_mnist28_generation_manager_and_png_dump(tmp_path):
    p = dlpm_amd.load_config('mnist28')
    p['device'] = DEV
    torch.manual_seed(0)
    net = dlpm_amd.rerandomize_(dlpm_amd.init_model_by_parameter(p), 1)
    meth = dlpm_amd.init_method_by_parameter(p, seed=1)
    kw = dict(p['eval']['dlpm'])
    kw['reverse_steps'] = 8
    gm = dlpm_amd.GenerationManager(meth, dlpm_amd.ShapeProbe(dlpm_amd.config.sample_shape(p)), True, **kw)
    s = gm.generate({'default': net}, 6)
    assert s.shape == (6, 1, 28, 28) and torch.isfinite(s).all() and s.min() >= 0 and s.max() <= 1
    from dlpm_amd import cli
    out = str(tmp_path / 'png')
    cli.main(['--config', 'mnist28', '--generate', '5', '--batch_size', '4', '--reverse_steps', '6', '--alpha', '1.7',
              '--synthetic_weights', '3', '--set_seed', '7', '--gen_data_path', out])
    files = sorted(os.listdir(out))
    assert files == ['%d.png' % i for i in range(5)], files
    for fn in files:
        with open(os.path.join(out, fn), 'rb') as fh:
            head = fh.read(24)
        assert head[:8] == b'\x89PNG\r\n\x1a\n' and struct.unpack('>II', head[16:24]) == (28, 28)
