"""Class-conditional UNets on the MI355X: forwards against the reference (F16) for every conv generation x GEMM pipe, label
locality, the same emb-row bits from the general forward / the uniform-t forward / the sampler (with and without the time table),
new labels in a captured graph, sharding, the bounded DLPM / DLIM trajectories of the reference's p_sample_loop / ddim_sample_loop
with model_kwargs={'y': y}, the chunked image dump and the CLI."""
import os
import struct

import numpy as np
import pytest
import torch
import yaml

from conftest import golden
import dlpm_amd
from dlpm_amd import _lib
from dlpm_amd.weights import rerandomize_, state_digest
from oracle import process as P

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GENERATIONS = ['auto', 'f4', 'f2', 'igemm']


def cond_net(name='mnist', head_scale=1.0):
    f = golden('f16_cond_' + name)
    in_ch, mc, heads, res, hw, K = (int(v) for v in f['cfg'])
    torch.manual_seed(1234)
    net = dlpm_amd.UNetModel(in_ch, mc, in_ch, res, [int(a) for a in f['attn']], channel_mult=[int(m) for m in f['mult']],
                             num_heads=heads, use_scale_shift_norm=True, num_classes=K)
    rerandomize_(net, 4321)
    if head_scale != 1.0:
        head = getattr(net.out, '2')          # the reference's out[2]
        with torch.no_grad():
            head.weight.mul_(head_scale)
            head.bias.mul_(head_scale)
        net.invalidate()
    return net, f


@pytest.mark.parametrize('gemm', ['bf16x3', 'f32'])
@pytest.mark.parametrize('gen', GENERATIONS)
@pytest.mark.parametrize('name', ['mnist', 'cifar_narrow'])
def test_conditional_forward_against_reference(name, gen, gemm):
    net, f = cond_net(name)
    assert state_digest(net) == bytes(f['digest_final']).hex()
    net.set_conv_policy(gen)
    net.set_gemm_policy(gemm)
    x, y = torch.from_numpy(f['x']).to(DEV), torch.from_numpy(f['y']).to(DEV)
    out = net(x, torch.from_numpy(f['t']).to(DEV), y).cpu().numpy()
    out2 = net(x, torch.from_numpy(f['t_same']).to(DEV), y).cpu().numpy()
    err = max(float(np.abs(out - f['out']).max()), float(np.abs(out2 - f['out_same_t']).max()))
    print('conditional %s forward (%s, %s): max |hip - reference| = %.3g' % (name, gen, gemm, err))
    assert err < 1e-4
    feats = net.get_feature_vectors(x, torch.from_numpy(f['t']).to(DEV), y)
    assert len(feats['down']) == len(net.input_blocks) and torch.isfinite(feats['middle']).all()


def test_label_locality_forward_and_sampler():
    """Labels y and y2 differ in two positions only: samples with the same label are bitwise equal, the others differ -- labels that
    were ignored, read with the wrong stride or shifted by one sample fail this."""
    net, _ = cond_net('mnist', head_scale=5.0)
    net.set_conv_policy('auto', 8)
    B = 8
    y = torch.tensor([0, 1, 2, 3, 4, 5, 6, 9])
    y2 = y.clone()
    y2[2], y2[5] = 7, 0
    same = (y == y2)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 1, 32, 32, generator=g).to(DEV)
    t = torch.rand(B, generator=g).to(DEV)
    a, b = net(x, t, y.to(DEV)).cpu(), net(x, t, y2.to(DEV)).cpu()
    for i in range(B):
        assert torch.equal(a[i], b[i]) == bool(same[i]), i

    def run(labels):
        m = dlpm_amd.GenerativeLevyProcess(1.7, DEV, 20, rescale_timesteps=True, seed=11)
        out = m.sample({'default': net}, [B, 1, 32, 32], 20, clamp_a=20, clamp_eps=200, clip_denoised=True,
                       model_kwargs={'y': labels}).cpu()
        m.close()
        return out
    a, b = run(y), run(y2)
    assert torch.isfinite(a).all()
    for i in range(B):
        assert torch.equal(a[i], b[i]) == bool(same[i]), i
    m = dlpm_amd.GenerativeLevyProcess(1.7, DEV, 20, rescale_timesteps=True, seed=11)
    with pytest.raises(IndexError):
        m.sample({'default': net}, [B, 1, 32, 32], 20, model_kwargs={'y': torch.full((B,), 10)})
    with pytest.raises(AssertionError, match='if and only if'):
        m.sample({'default': net}, [B, 1, 32, 32], 20)


def test_out_of_range_label_gives_a_nan_row_never_a_read():
    """The C entry point (UNetModel.forward refuses such labels first): a label outside [0, K) yields NaN for its sample only."""
    net, f = cond_net('mnist')
    x, t = torch.from_numpy(f['x']).to(DEV), torch.from_numpy(f['t']).to(DEV)
    y = torch.from_numpy(f['y']).to(DEV)
    want = net(x, t, y).cpu()
    bad = y.clone()
    bad[1], bad[4] = 10, -3
    h = net.native_handle(32)
    ws = net.workspace(x.shape[0], x.device)
    out = torch.empty_like(x)
    _lib.check(_lib.lib().dlpm_unet_forward_labels(h, x.data_ptr(), t.data_ptr(), bad.data_ptr(), out.data_ptr(), x.shape[0],
                                                  ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
    out = out.cpu()
    for i in range(x.shape[0]):
        if i in (1, 4):
            assert torch.isnan(out[i]).all(), i
        else:
            assert torch.equal(out[i], want[i]), i


@pytest.mark.parametrize('clip', [False, True])
def test_general_uniform_and_sampler_rows_have_the_same_bits(clip, monkeypatch):
    """A sample's emb row is the same whether the general forward (B rows of t), the uniform-t forward (one time-MLP row) or the
    sampler (its [T][4 mc] table, or no table: DLPM_NO_TIME_TABLE=1) computed it: the forwards agree bit for bit, and so do the
    trajectories of the native sampler (fused head update without clip, the update kernels with it) and of the Python loop around
    the general forward."""
    net, _ = cond_net('mnist', head_scale=5.0)
    net.set_conv_policy('auto', 6)
    B, T = 6, 12
    y = torch.tensor([3, 3, 0, 9, 1, 3])
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, 1, 32, 32, generator=g).to(DEV)
    t = torch.full((B,), 7 / T, device=DEV)
    yd = y.to(DEV)
    h = net.native_handle(32)
    ws = net.workspace(B, x.device)
    outs = []
    for fn in (_lib.lib().dlpm_unet_forward_labels, _lib.lib().dlpm_unet_forward_uniform_t_labels):
        o = torch.empty_like(x)
        _lib.check(fn(h, x.data_ptr(), t.data_ptr(), yd.data_ptr(), o.data_ptr(), B, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        outs.append(o.cpu())
    assert torch.equal(outs[0], outs[1])

    def run(native, table=True):
        if table:
            monkeypatch.delenv('DLPM_NO_TIME_TABLE', raising=False)
        else:
            monkeypatch.setenv('DLPM_NO_TIME_TABLE', '1')
        m = dlpm_amd.GenerativeLevyProcess(1.7, DEV, T, rescale_timesteps=True, seed=4)
        model = net if native else (lambda xx, tt, **kw: net(xx, tt, **kw))     # not a UNetModel: the Python loop
        out = m.sample({'default': model}, [B, 1, 32, 32], T, clamp_a=20, clamp_eps=200, clip_denoised=clip,
                       model_kwargs={'y': y}, get_sample_history=True)
        m.close()
        return out[1].cpu()
    graph, no_table, loop = run(True), run(True, table=False), run(False)
    assert torch.isfinite(graph).all()
    assert torch.equal(graph, no_table), 'time table and time path differ'
    assert torch.equal(graph, loop), 'native sampler and general forward differ'


def test_new_labels_replay_the_captured_graph():
    """dlpm_sampler_set_labels writes the buffer the graph reads: a second sample() on the same sampler (no new sampler, no recapture)
    equals a fresh sampler given those labels."""
    net, _ = cond_net('mnist', head_scale=5.0)
    net.set_conv_policy('auto', 6)
    B, T = 6, 10
    y1, y2 = torch.tensor([0, 1, 2, 3, 4, 5]), torch.tensor([9, 9, 2, 0, 4, 8])
    kw = dict(clamp_a=20, clamp_eps=200)
    m = dlpm_amd.GenerativeLevyProcess(1.7, DEV, T, rescale_timesteps=True, seed=2)
    a1 = m.sample({'default': net}, [B, 1, 32, 32], T, model_kwargs={'y': y1}, **kw).cpu()
    (key, ent), = m._samplers.items()
    a2 = m.sample({'default': net}, [B, 1, 32, 32], T, model_kwargs={'y': y2}, **kw).cpu()
    assert list(m._samplers) == [key] and m._samplers[key]['h'].value == ent['h'].value
    m.close()
    fresh = dlpm_amd.GenerativeLevyProcess(1.7, DEV, T, rescale_timesteps=True, seed=2)
    fresh.calls = 1                     # the Philox key of the second call
    b2 = fresh.sample({'default': net}, [B, 1, 32, 32], T, model_kwargs={'y': y2}, **kw).cpu()
    fresh.close()
    assert torch.isfinite(a2).all() and not torch.equal(a1, a2)
    assert torch.equal(a2, b2)


def test_whole_batch_equals_its_shards():
    net, _ = cond_net('mnist', head_scale=5.0)
    net.set_conv_policy('auto', 8)
    B, T = 7, 10
    y = torch.tensor([5, 0, 9, 9, 2, 7, 1])

    def run(lo, hi):
        m = dlpm_amd.GenerativeLevyProcess(1.7, DEV, T, rescale_timesteps=True, seed=9, sample_offset=lo)
        out = m.sample({'default': net}, [hi - lo, 1, 32, 32], T, clamp_a=20, clamp_eps=200, model_kwargs={'y': y[lo:hi]}).cpu()
        m.close()
        return out
    full = run(0, B)
    assert torch.equal(full, torch.cat([run(0, 3), run(3, 7)]))


@pytest.mark.parametrize('gen', ['auto', 'igemm'])
@pytest.mark.parametrize('tag', ['dlpm', 'dlim'])
def test_conditional_trajectories_against_reference(tag, gen):
    """The reference's p_sample_loop / ddim_sample_loop (clip_denoised, model_kwargs={'y': y}) of the MNIST-shaped net on its own CPU
    streams: recorded states within 1e-4 (relative to their scale) and post-processed pixels within 1e-4."""
    f = golden('f16_traj_cond_mnist_%s_clip' % tag)
    net, _ = cond_net('mnist', head_scale=float(f['head_scale']))
    assert state_digest(net) == bytes(f['digest']).hex()
    net.set_conv_policy(gen)
    T, alpha, ca, ce = f['meta']
    m = dlpm_amd.GenerativeLevyProcess(float(alpha), DEV, int(T), rescale_timesteps=True, rng='reference', seed=0)
    m.dlpm.gen_a.setParams(clamp_a=float(ca))
    m.dlpm.gen_eps.setParams(clamp_eps=float(ce))
    loop = m.ddim_sample_loop if tag == 'dlim' else m.p_sample_loop
    x, hist = loop(net, [int(v) for v in f['shape']], clip_denoised=True, model_kwargs={'y': torch.from_numpy(f['y'])},
                   get_sample_history=True)
    m.close()
    err_state = float(np.abs(hist[::int(f['every'])].cpu().numpy() - f['history_sub']).max())
    got = dlpm_amd.GenerationManager(None, None, True)._post(x).numpy()
    want = P.generation_postprocess(torch.from_numpy(f['final']), True).numpy()
    err = float(np.abs(got - want).max())
    print('conditional %s trajectory (%s): states %.3g, pixels %.3g (fixture sensitivity %.3g)'
          % (tag, gen, err_state, err, float(f['sensitivity'])))
    assert err_state < 1e-4 * max(1.0, float(np.abs(f['history_sub']).max()))
    assert err < 1e-4


def _dump(net, out, batch_size, labels):
    m = dlpm_amd.GenerativeLevyProcess(1.7, DEV, 8, rescale_timesteps=True, seed=6)
    gm = dlpm_amd.GenerationManager(m, dlpm_amd.ShapeProbe([1, 32, 32]), True, reverse_steps=8, clip_denoised=True, clamp_a=20,
                                    clamp_eps=200)
    ev = dlpm_amd.EvaluationManager(m, gm, None, is_image=True, gen_data_path=out, device_batch=0, verbose=False)
    r = ev.evaluate_model({'default': net}, data_to_generate=len(labels), batch_size=batch_size, class_labels=labels)
    m.close()
    return r


def test_chunked_dump_equals_unchunked(tmp_path):
    net, _ = cond_net('mnist', head_scale=5.0)
    net.set_conv_policy('auto', 8)
    labels = torch.tensor([4, 4, 0, 9, 1, 2, 3])
    a, b = str(tmp_path / 'chunked'), str(tmp_path / 'whole')
    _dump(net, a, 3, labels)
    _dump(net, b, 7, labels)
    files = sorted(os.listdir(a))
    assert files == sorted(['%d.png' % i for i in range(7)] + ['labels.npy'])
    assert files == sorted(os.listdir(b))
    for fn in files:
        with open(os.path.join(a, fn), 'rb') as fa, open(os.path.join(b, fn), 'rb') as fb:
            assert fa.read() == fb.read(), fn
    got = np.load(os.path.join(a, 'labels.npy'))
    assert got.dtype == np.int64 and np.array_equal(got, labels.numpy())


def test_cli_class_labels_cycle(tmp_path):
    p = dlpm_amd.load_config('mnist')
    p['model']['class_cond'] = True
    p['data']['num_classes'] = 10
    cfg = str(tmp_path / 'mnist_cond.yml')
    with open(cfg, 'w') as fh:
        yaml.safe_dump(p, fh)
    out = str(tmp_path / 'png')
    from dlpm_amd import cli
    cli.main(['--config', cfg, '--generate', '13', '--batch_size', '4', '--reverse_steps', '6', '--alpha', '1.7',
              '--synthetic_weights', '3', '--set_seed', '7', '--gen_data_path', out, '--class_labels', 'cycle'])
    files = sorted(os.listdir(out))
    assert files == sorted(['%d.png' % i for i in range(13)] + ['labels.npy']), files
    assert np.array_equal(np.load(os.path.join(out, 'labels.npy')), np.arange(13) % 10)
    for i in range(13):
        with open(os.path.join(out, '%d.png' % i), 'rb') as fh:
            head = fh.read(24)
        assert head[:8] == b'\x89PNG\r\n\x1a\n' and struct.unpack('>II', head[16:24]) == (32, 32)
    s = cli.main(['--config', cfg, '--generate', '3', '--batch_size', '2', '--reverse_steps', '6', '--synthetic_weights', '3',
                  '--class_labels', '4'])
    assert s.shape == (3, 1, 32, 32) and torch.isfinite(s).all()
