"""Geometries beyond the four shipped configs, on the CPU: the oracle against the F15 fixtures (QKVAttention at any token count /
head dim, the 28x28 MNIST UNet of dlpm_amd/configs/mnist28.yml), the config's parameter layout against the reference's, and the
native launch planner on the 28x28 and T = 1024 nets (a host-side dry run: no GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden
import dlpm_amd
from dlpm_amd import _lib
from dlpm_amd.weights import state_digest
from oracle import nets, process as P, sampler

ATTN_SHAPES = [(16, 49), (16, 196), (8, 784), (8, 4), (32, 1024), (24, 100), (256, 64)]


def mnist28_net(head_scale=1.0):
    """The F15 net: dlpm_amd/configs/mnist28.yml's UNet, weights seeded and re-randomised as in F6."""
    p = dlpm_amd.load_config('mnist28')
    torch.manual_seed(1234)
    net = dlpm_amd.init_model_by_parameter(p)
    dlpm_amd.rerandomize_(net, 4321)
    if head_scale != 1.0:
        with torch.no_grad():
            getattr(net.out, '2').weight.mul_(head_scale)
            getattr(net.out, '2').bias.mul_(head_scale)
    return net


@pytest.mark.parametrize('ch,T', ATTN_SHAPES)
def test_oracle_attention_reproduces_f15(ch, T):
    f = golden('f15_attention_any')
    qkv = torch.from_numpy(f['ch%d_T%d_in' % (ch, T)].astype(np.float32))
    got = nets.qkv_attention(qkv).numpy()
    np.testing.assert_allclose(got, f['ch%d_T%d_out' % (ch, T)], rtol=0, atol=1e-6)


def test_mnist28_config_matches_the_reference_parameter_layout():
    f = golden('f15_unet_mnist28')
    p = dlpm_amd.load_config('mnist28')
    assert p['data']['image_size'] == 28 and p['data']['channels'] == 1
    net = dlpm_amd.init_model_by_parameter(p)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in f['keys']]
    for k, row in zip(sd.keys(), f['shapes']):
        assert tuple(sd[k].shape) == tuple(int(v) for v in row if v >= 0), k
    assert dlpm_amd.config.sample_shape(p) == [1, 28, 28]


def test_oracle_unet_forward_reproduces_f15_mnist28():
    f = golden('f15_unet_mnist28')
    net = mnist28_net()
    assert state_digest(net) == bytes(f['digest_final']).hex()
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    x = torch.from_numpy(f['x'])
    with torch.no_grad():
        y = nets.unet_forward(sd, x, torch.from_numpy(f['t']), 4)
        y2 = nets.unet_forward(sd, x, torch.from_numpy(f['t_same']), 4)
    assert y.shape == (2, 1, 28, 28)
    assert np.abs(y.numpy() - f['y']).max() < 1e-5
    assert np.abs(y2.numpy() - f['y_same_t']).max() < 1e-5


def test_oracle_reproduces_the_last_steps_of_f15_mnist28_trajectory():
    """The bounded T = 1000 reference sample() of the 28x28 net: the oracle re-runs the last 100 steps from the reference's own
    state 900, with both reference streams advanced to that point (as tests/test_oracle_golden.py does for the shipped nets)."""
    f = golden('f15_traj_unet_mnist28_clip_T1000')
    fin = f['final']
    inside = float((np.abs(fin) < 1).mean())
    assert inside >= 0.7 and float(f['sensitivity']) >= 0.4
    net = mnist28_net(float(f['head_scale']))
    assert state_digest(net) == bytes(f['digest']).hex()
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    T, alpha, ca, ce = f['meta']
    T, shape = int(T), [int(v) for v in f['shape']]
    streams = sampler.Streams(0, 0)
    g, bg, s_, bs = P.schedule(T, float(alpha))
    A = torch.stack([streams.skewed_levy(float(alpha), shape[0], float(ca)) for _ in range(T)])
    Sig = P.sigma_table(A, g, s_)
    streams.skewed_levy(float(alpha), shape[0], None)
    streams.randn(shape)                                           # x_T's draws
    k0 = 900
    for _ in range(k0):
        streams.randn(shape)                                       # the z of the steps already taken
    x = torch.from_numpy(np.asarray(f['state_900'], dtype=np.float32))
    with torch.no_grad():
        for k in range(k0, T - 1):
            i = T - 1 - k
            eps = nets.unet_forward(sd, x, torch.full((shape[0],), i, dtype=torch.int64).float() * (1.0 / T), 4)
            eps = P.model_eps(x, eps, i, 'EPSILON', True, None, g, bg, bs, Sig=Sig, A=A)
            x, _, _ = P.dlpm_step(x, eps, i, Sig, g, bs, streams.randn(shape))
    post = lambda v: P.generation_postprocess(torch.from_numpy(np.asarray(v)), True).numpy()
    err = float(np.abs(post(x.numpy()) - post(fin)).max())
    print('f15 mnist28 trajectory: oracle vs reference over the last 100 steps: post-processed pixels %.3g' % err)
    assert err < 1e-4


def _plan(size, mult, attn, mc=32, heads=4, B=8):
    L = _lib.lib()
    cfg = _lib.UNetConfig()
    cfg.in_channels, cfg.model_channels, cfg.out_channels = 1, mc, 1
    cfg.num_res_blocks, cfg.num_heads, cfg.image_size = 2, heads, size
    cfg.n_mult, cfg.n_attn = len(mult), len(attn)
    for i, m in enumerate(mult):
        cfg.channel_mult[i] = m
    for i, a in enumerate(attn):
        cfg.attention_resolutions[i] = a
    h = C.c_void_p()
    _lib.check(L.dlpm_unet_create(C.byref(cfg), C.byref(h)))
    try:
        return L.dlpm_unet_workspace_bytes(h, B), L.dlpm_unet_workspace_bytes(h, 2 * B)
    finally:
        L.dlpm_unet_destroy(h)


@pytest.mark.parametrize('size,mult,attn', [(28, [1, 2, 2], [2, 4]),          # mnist28.yml: attention at T = 196 / 49
                                            (28, [1, 2, 2], [1, 2, 4]),       # attention at T = 784 (head dim 8)
                                            (32, [1, 2, 2, 2], [1, 2, 4]),    # T = 1024
                                            (32, [1, 2, 2, 2, 2], [16]),      # 5 levels: attention at 2x2 (T = 4)
                                            (48, [1, 2, 2, 2], [2, 4]),       # 48 / 24 / 12 / 6: attention at T = 576 / 144
                                            (20, [1, 2, 2], [2, 4])])         # 20 / 10 / 5: attention at T = 100 / 25
def test_planner_takes_the_new_geometries(size, mult, attn):
    a, b = _plan(size, mult, attn)
    assert 0 < a < b < 2.2 * a, (a, b)
