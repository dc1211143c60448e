"""UNet / MLP forward on the MI355X (through the C ABI handles) against the reference outputs in
tests/golden/f6_*.npz (weights rebuilt from seeds, pinned by digest) and against the oracle."""
import numpy as np
import pytest
import torch

from conftest import golden
import dlpm_amd
from oracle import nets
from test_host_mirror import UNETS, build_unet

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _stats(feats):
    rows = []
    for grp in ('down', 'up'):
        for f in feats[grp]:
            f = f.float().cpu()
            rows.append([f.mean().item(), f.abs().mean().item()] + f.flatten()[:4].tolist())
    f = feats['middle'].float().cpu()
    rows.append([f.mean().item(), f.abs().mean().item()] + f.flatten()[:4].tolist())
    return np.array(rows)


@pytest.mark.parametrize('name', ['tiny', 'tiny2', 'mnist', 'cifar'])
def test_unet_forward_matches_reference(name):
    f = golden('f6_unet_' + name)
    net, _ = build_unet(name)
    x, t = torch.from_numpy(f['x']).to(DEV), torch.from_numpy(f['t']).to(DEV)
    feats = net.get_feature_vectors(x, t)
    y = net(x, t).cpu().numpy()
    got_stats = _stats(feats)
    # bisecting aid: report the first block whose statistics drift
    bad = np.where(np.abs(got_stats - f['block_stats']).max(axis=1) > 1e-4)[0]
    assert bad.size == 0, 'first diverging block index: %d (of %d)\n%s\n%s' % (
        bad[0], len(got_stats), got_stats[bad[0]], f['block_stats'][bad[0]])
    # eps is O(0.1..1); ~60 fp32 layers deep: 1e-4 is the north-star tolerance, observed ~1e-5
    assert np.abs(y - f['y']).max() < 1e-4
    y2 = net(x, torch.from_numpy(f['t_same']).to(DEV)).cpu().numpy()
    assert np.abs(y2 - f['y_same_t']).max() < 1e-4


@pytest.mark.parametrize('declared', [2, 64, 256])
def test_cifar_unet_under_a_small_declared_batch_against_reference(declared):
    """Round 6: under a small DECLARED batch the CIFAR net's 128-channel-multiple F(4x4) layers run on 64- / 32-channel
    n-tiles and the launches that would still leave half the chip empty split their K loop over 2 / 4 / 8 grid copies (partial outputs +
    launch_splitk_reduce; conv_splitk.hip).  The reference's own output (f6_unet_cifar) within the usual 2e-5 for each declaration, a
    declaration is what decides (the SAME call under another declaration may differ in the last bits, under the same one it may not), and
    a sample's bits do not depend on the batch of the CALL."""
    f = golden('f6_unet_cifar')
    net, _ = build_unet('cifar')
    net.set_conv_policy('auto', declared)
    x, t = torch.from_numpy(f['x']).to(DEV), torch.from_numpy(f['t']).to(DEV)
    y = net(x, t)
    err = (y.cpu() - torch.from_numpy(f['y'])).abs().max().item()
    print('declared batch %d: max |hip - reference| = %.3g' % (declared, err))
    assert err < 2e-5
    assert torch.equal(net(x, t), y)
    xb = torch.cat([x, x.flip(0), 0.5 * x, x[:1]])
    tb = torch.cat([t, t.flip(0), t, t[:1]])
    yb = net(xb, tb)
    assert torch.equal(yb[:x.shape[0]], y) and torch.equal(yb[-1], y[0])
    net.set_conv_policy('auto', 0)


@pytest.mark.parametrize('env,bound', [({'DLPM_WINO_F4': '0'}, 1e-5), ({'DLPM_WINO_F4': '0', 'DLPM_NO_WINO': '1'}, 1e-5),
                                       ({}, 2e-5),
                                       ({'DLPM_NO_FUSED_BLOCKS': '1', 'DLPM_NO_HEAD_FUSED': '1'}, 2e-5), ({'DLPM_HEAD_F32': '1'}, 2e-5)],
                         ids=['winograd_f2x2_only', 'implicit_gemm_only', 'default_f4x4',
                              'round3_blocks_and_head', 'head_on_the_fp32_mfma'])
def test_unet_every_convolution_generation_against_reference(env, bound):
    """(Also the per-layer launches / GEMM + gather head the fused kernels replaced, and the one-pass head on the fp32 MFMA instead of
    the bf16 pipe with the exact three-plane split.)
    The kernel choice is read once per process, so each generation runs in a child process (tools/err_report.py):
    CIFAR UNet vs the reference's own output.  Observed: F(4x4) 5.1e-6 (round 4's interpolation points; 1.35e-5 with the textbook
    ones, when the bound here was 5e-5), F(2x2) 3e-6, implicit GEMM 4.4e-6."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    e = dict(os.environ)
    e.update(env)
    out = subprocess.run([sys.executable, os.path.join(root, 'tools', 'err_report.py')], env=e, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    errs = {m.group(1): float(m.group(2)) for m in re.finditer(r'(\w+)\s+max \|hip - reference\| = ([0-9.e+-]+)', out.stdout)}
    assert set(errs) == {'tiny', 'tiny2', 'mnist', 'cifar'}, out.stdout
    assert errs['cifar'] < bound, errs
    assert max(errs[k] for k in ('tiny', 'tiny2', 'mnist')) < 5e-6, errs   # no layer of these nets takes F(4x4)


def test_unet_tiny_every_block_against_reference_features():
    f = golden('f6_unet_tiny')
    net, _ = build_unet('tiny')
    x, t = torch.from_numpy(f['x']).to(DEV), torch.from_numpy(f['t']).to(DEV)
    feats = net.get_feature_vectors(x, t)
    for i, ft in enumerate(feats['down']):
        assert np.abs(ft.cpu().numpy() - f['feat_down_%d' % i]).max() < 5e-5, 'down %d' % i
    assert np.abs(feats['middle'].cpu().numpy() - f['feat_middle']).max() < 5e-5
    for i, ft in enumerate(feats['up']):
        assert np.abs(ft.cpu().numpy() - f['feat_up_%d' % i]).max() < 5e-5, 'up %d' % i


def test_unet_batch_tail_and_repeatability():
    """B not a multiple of any tile size; two calls give identical bits (no atomics on the path)."""
    net, _ = build_unet('tiny2')
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 1, 16, 16, generator=g)
    t = torch.rand(5, generator=g)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    with torch.no_grad():
        want = nets.unet_forward(sd, x, t, UNETS['tiny2']['heads'])
    a = net(x.to(DEV), t.to(DEV))
    b = net(x.to(DEV), t.to(DEV))
    assert torch.equal(a, b)
    assert (a.cpu() - want).abs().max().item() < 1e-4
    # batch-independence: sample 3 alone equals row 3 of the batch
    c = net(x[3:4].to(DEV), t[3:4].to(DEV))
    assert (c.cpu() - a.cpu()[3:4]).abs().max().item() < 1e-6


@pytest.mark.parametrize('name', ['tiny2', 'cifar'])
def test_unet_uniform_t_forward_is_bit_identical(name):
    """dlpm_unet_forward_uniform_t (the sampling loop's call: one shared timestep, time MLP + emb linears on one row,
    unet.py:147-150,336-338) against the general forward fed B equal timesteps, and against the reference output."""
    import ctypes as C
    from dlpm_amd import _lib
    f = golden('f6_unet_' + name)
    net, _ = build_unet(name)
    x = torch.from_numpy(f['x']).to(DEV)
    if x.shape[0] < 3:
        x = torch.cat([x, x.flip(0) * 0.5, x * 0.25])[:3].contiguous()
    B = x.shape[0]
    t = torch.full((B,), float(f['t_same'][0]), device=DEV)
    want = net(x, t)
    L, h = _lib.lib(), net.native_handle(x.shape[2])
    ws = net.workspace(B, x.device)
    got = torch.empty_like(want)
    _lib.check(L.dlpm_unet_forward_uniform_t(h, x.data_ptr(), t[:1].contiguous().data_ptr(), got.data_ptr(), B, ws.data_ptr(),
                                            ws.numel(), _lib.stream_ptr()))
    assert torch.equal(got, want)
    nb = f['x'].shape[0]
    assert np.abs(got[:nb].cpu().numpy() - f['y_same_t']).max() < 1e-4


@pytest.mark.parametrize('name,size,B,declared', [
    ('tiny2', 16, 5, None),     # the fused small-image ResBlocks and attention blocks
    ('mnist', 32, 2, None),     # the whole-image ResBlocks at 32x32 and 16x16
    ('wide', 16, 2, 2),         # a declared batch of 2: narrow n-tiles, split-K partial buffers, the general path
    ('mnist', 48, 3, None),     # levels of 48, 24, 12 and 6 pixels: F(4x4) with 3 blocks per row, the generic implicit GEMM
    ('tiny2', 20, 3, None),     # levels of 20, 10 and 5 pixels
])
def test_unet_forward_stays_inside_the_planned_workspace(name, size, B, declared):
    """The sized plan is the launched plan: dlpm_unet_workspace_bytes is a dry run of the very walk that launches, so a forward handed
    exactly `need` bytes leaves a guard region behind them untouched and gives the bits of net(x, t); 256 bytes (one arena granule)
    less is refused with the no-memory status before anything runs."""
    import ctypes as C
    from dlpm_amd import _lib
    net, _ = build_unet(name)
    if declared:
        net.set_conv_policy('auto', declared)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, UNETS[name]['in_ch'], size, size, generator=g).to(DEV)
    t = torch.rand(B, generator=g).to(DEV)
    want = net(x, t)
    L, h = _lib.lib(), net.native_handle(size)
    need = L.dlpm_unet_workspace_bytes(h, B)
    assert need > 0 and need % 256 == 0
    guard = 1 << 20
    buf = torch.empty(need + guard, dtype=torch.uint8, device=DEV)
    buf[need:] = 0xA5
    got = torch.full_like(want, float('nan'))
    _lib.check(L.dlpm_unet_forward(h, x.data_ptr(), t.data_ptr(), got.data_ptr(), B, buf.data_ptr(), need, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((buf[need:] == 0xA5).all())
    assert torch.equal(got, want)
    rc = L.dlpm_unet_forward(h, x.data_ptr(), t.data_ptr(), got.data_ptr(), B, buf.data_ptr(), need - 256, _lib.stream_ptr())
    assert rc == -5, rc                                            # DLPM_ERR_NOMEM
    assert torch.equal(got, want)                                  # ... and nothing was enqueued


def test_unet_zero_init_outputs_zero_and_state_dict_roundtrip():
    """Reference default init (zero_module) gives eps == 0 exactly; load_state_dict re-uploads."""
    torch.manual_seed(0)
    c = UNETS['tiny']
    net = dlpm_amd.UNetModel(c['in_ch'], c['mc'], c['in_ch'], c['res'], c['attn'], channel_mult=c['mult'],
                             num_heads=c['heads'], use_scale_shift_norm=True)
    x = torch.randn(2, 3, 16, 16).to(DEV)
    t = torch.rand(2).to(DEV)
    assert torch.count_nonzero(net(x, t)).item() == 0
    other, _ = build_unet('tiny')
    net.load_state_dict(other.state_dict())
    assert torch.equal(net(x, t), other(x, t)) and torch.count_nonzero(net(x, t)).item() > 0


def test_mlp_forward_matches_reference():
    f = golden('f6_mlp_forward')
    p = dlpm_amd.load_config('2d_data')
    torch.manual_seed(1)
    m = dlpm_amd.MLPModel(p)
    y = m(torch.from_numpy(f['x']).to(DEV), torch.from_numpy(f['t']).to(DEV)).cpu().numpy()
    np.testing.assert_allclose(y, f['y'], rtol=1e-5, atol=2e-6)
    # ragged batch (B % 4 != 0) against the oracle
    g = torch.Generator().manual_seed(2)
    x, t = torch.randn(13, 1, 2, generator=g) * 3, torch.rand(13, generator=g)
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    with torch.no_grad():
        want = nets.mlp_forward(sd, x, t)
    got = m(x.to(DEV), t.to(DEV)).cpu()
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=2e-6)


def test_error_paths():
    net, _ = build_unet('tiny')
    with pytest.raises(Exception, match='divisible'):
        net(torch.zeros(1, 3, 15, 15, device=DEV), torch.zeros(1, device=DEV))
    with pytest.raises(NotImplementedError):
        dlpm_amd.UNetModel(3, 32, 3, 1, [2], channel_mult=[1, 2], num_heads=4, use_scale_shift_norm=False)


def test_unet_64x64_against_oracle():
    """BASELINE configs[4] shape (64x64, attention at 16x16 = 256 tokens and 8x8), narrow width to keep
    the CPU oracle fast: mc=32, same block structure as the CIFAR net."""
    torch.manual_seed(11)
    net = dlpm_amd.UNetModel(3, 32, 3, 2, [4, 8, 16], channel_mult=[1, 2, 2, 2], num_heads=4, use_scale_shift_norm=True)
    dlpm_amd.rerandomize_(net, 12)
    g = torch.Generator().manual_seed(13)
    x, t = torch.randn(2, 3, 64, 64, generator=g), torch.rand(2, generator=g)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    with torch.no_grad():
        want = nets.unet_forward(sd, x, t, 4)
    got = net(x.to(DEV), t.to(DEV)).cpu()
    assert (got - want).abs().max().item() < 1e-4


def test_celeba64_unet_at_its_own_width_against_oracle():
    """BASELINE configs[4] net as configured (dlpm_amd/configs/celeba64.yml: the CIFAR architecture, mc = 128, at 64x64:
    attention over 256 and 64 tokens, F(4x4) Winograd layers at 64/32/16/8 pixels) against the CPU oracle, B = 2."""
    p = dlpm_amd.load_config('celeba64')
    torch.manual_seed(21)
    net = dlpm_amd.rerandomize_(dlpm_amd.init_model_by_parameter(p), 22)
    assert net.model_channels == 128
    g = torch.Generator().manual_seed(23)
    x, t = torch.randn(2, 3, 64, 64, generator=g), torch.rand(2, generator=g)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    with torch.no_grad():
        want = nets.unet_forward(sd, x, t, p['model']['num_heads'])
    got = net(x.to(DEV), t.to(DEV)).cpu()
    err = (got - want).abs().max().item()
    print('celeba64 net (mc=128, 64x64): max |hip - oracle| = %.3g (|y| max %.3g)' % (err, want.abs().max().item()))
    assert err < 1e-4


# The three head kernels that carry the update in their epilogue, by the profiler class of the launch, and a net that reaches each:
# the one-pass head wants 32- or 64-pixel rows (cifar), the GEMM + gather takes the 16-pixel ones (tiny2), and k_conv3x3_head is
# left with what neither MFMA head takes -- four output channels (tiny2's architecture on 4-channel images).
HEAD_OF = {'cifar': 'head_fused+update', 'tiny2': 'head_gather+update', 'tiny2_4ch': 'conv3x3_head+update'}


def _net_and_state(name):
    if name == 'tiny2_4ch':
        c = UNETS['tiny2']
        torch.manual_seed(1234)
        net = dlpm_amd.UNetModel(4, c['mc'], 4, c['res'], c['attn'], channel_mult=c['mult'], num_heads=c['heads'],
                                 use_scale_shift_norm=True)
        dlpm_amd.rerandomize_(net, 4321)
        return net, torch.randn(3, 4, 16, 16, generator=torch.Generator().manual_seed(5)).to(DEV)
    return build_unet(name)[0], torch.from_numpy(golden('f6_unet_' + name)['x']).to(DEV)


@pytest.mark.parametrize('name', ['tiny2', 'cifar', 'tiny2_4ch'])
@pytest.mark.parametrize('variant', ['philox', 'injected_z', 'history', 'dlim_unfused'])
def test_unet_forward_with_fused_update_is_bit_identical_to_the_pair(name, variant):
    """dlpm_unet_forward_update (the head convolution applies x <- (x - c_eps eps)/g + c_noise z in its epilogue,
    GenerativeLevyProcess.py:225-239) against dlpm_unet_forward_uniform_t followed by dlpm_update_f32: same bits, with
    in-kernel Philox noise, with injected normals, with a history row, and for a variant that takes the unfused pair.  One net
    per head kernel that carries the update (HEAD_OF); the fused call must have run that kernel."""
    import ctypes as C
    from dlpm_amd import _lib
    net, x0 = _net_and_state(name)
    x0 = torch.cat([x0, x0.flip(0) * 0.5, x0 * 0.25])[:3].contiguous()
    B, D, T, t = 3, x0[0].numel(), 7, 4
    g = torch.Generator(device='cpu').manual_seed(11)
    gam = (0.5 + torch.rand(T, generator=g)).to(DEV)
    c_eps, c_noise = torch.rand(T, B, generator=g).to(DEV), torch.rand(T, B, generator=g).to(DEV)
    c_noise[t, 1] = 0.0                                    # a sample whose noise coefficient is exactly zero
    bg, bs = torch.rand(T, generator=g).to(DEV) + 0.5, torch.rand(T, generator=g).to(DEV) + 0.1
    A = torch.rand(T, B, generator=g).to(DEV) + 0.5
    z = torch.randn(B, D, generator=g).to(DEV) if variant == 'injected_z' else None
    tvec = torch.full((B,), t / T, device=DEV)
    L, h = _lib.lib(), net.native_handle(x0.shape[2])
    ws = net.workspace(B, x0.device)
    st = _lib.stream_ptr()

    def args(x, t_dev, eps, hist_cell):
        a = _lib.UpdateArgs()
        a.x_dev, a.eps_dev, a.t_dev = x.data_ptr(), eps.data_ptr() if eps is not None else None, t_dev.data_ptr()
        a.z_dev = z.data_ptr() if z is not None else None
        a.g_dev, a.bg_dev, a.bs_dev = gam.data_ptr(), bg.data_ptr(), bs.data_ptr()
        a.c_eps_dev, a.c_noise_dev, a.A_dev = c_eps.data_ptr(), c_noise.data_ptr(), A.data_ptr()
        a.B, a.D, a.T = B, D, T
        a.flags = _lib.UPD_ADVANCE | (_lib.UPD_DLIM if variant == 'dlim_unfused' else 0)
        a.alpha, a.seed, a.sample_offset = 1.7, 1234, 40
        a.hist_pp = hist_cell.data_ptr() if hist_cell is not None else None
        return a

    outs = []
    for fused in (False, True):
        x = x0.clone()
        t_dev = torch.tensor([t], dtype=torch.int32, device=DEV)
        eps = torch.empty_like(x0)
        hist = torch.zeros(T, B, D, device=DEV) if variant == 'history' else None
        cell = torch.tensor([hist.data_ptr()], dtype=torch.int64, device=DEV) if hist is not None else None
        a = args(x, t_dev, eps, cell)
        if fused:
            _lib.check(L.dlpm_prof_enable(1))
            _lib.check(L.dlpm_unet_forward_update(h, x.data_ptr(), tvec.data_ptr(), C.byref(a), eps.data_ptr(), B, ws.data_ptr(),
                                                  ws.numel(), st))
            buf = C.create_string_buffer(1 << 16)
            _lib.check(L.dlpm_prof_report(buf, len(buf)))
            _lib.check(L.dlpm_prof_enable(0))
            ran = {line.split()[0] for line in buf.value.decode().strip().splitlines()}
            assert any(k.startswith(HEAD_OF[name]) for k in ran) == (variant != 'dlim_unfused'), sorted(ran)
        else:
            _lib.check(L.dlpm_unet_forward_uniform_t(h, x.data_ptr(), tvec.data_ptr(), eps.data_ptr(), B, ws.data_ptr(), ws.numel(), st))
            _lib.check(L.dlpm_update_f32(C.byref(a), st))
        torch.cuda.synchronize()
        assert int(t_dev.item()) == t - 1                  # DLPM_UPD_ADVANCE on both paths
        outs.append((x.cpu(), None if hist is None else hist.cpu()))
    assert torch.isfinite(outs[0][0]).all() and not torch.equal(outs[0][0], x0.cpu())
    assert torch.equal(outs[0][0], outs[1][0])
    if variant == 'history':
        assert torch.equal(outs[0][1], outs[1][1]) and torch.count_nonzero(outs[1][1][T - t]).item() > 0


@pytest.mark.parametrize('name', ['cifar', 'wide'])
def test_unet_gemm_policy_both_pipes_against_reference(name):
    """UNetModel.set_gemm_policy: the 1x1 and stride-2 convolutions on the bf16 pipe with split operands (the default) and
    on the fp32 MFMA, each against the reference's own output of the same net (unet.py:463-492).  The two are different
    kernels (the outputs differ in the last bits) of the same accuracy: the conv-generation tests hold the other
    convolutions fixed at F(2x2) here so that only the GEMM pipe moves."""
    f = golden('f6_unet_' + name)
    net, _ = build_unet(name)
    net.set_conv_policy('f2')
    x, t = torch.from_numpy(f['x']).to(DEV), torch.from_numpy(f['t']).to(DEV)
    err, outs = {}, {}
    for mode in ('f32', 'bf16x3', 'auto'):
        net.set_gemm_policy(mode)
        outs[mode] = net(x, t).cpu()
        err[mode] = np.abs(outs[mode].numpy() - f['y']).max()
    print('%s: |hip - reference| max  fp32 MFMA %.2e   bf16x3 %.2e' % (name, err['f32'], err['bf16x3']))
    assert torch.equal(outs['auto'], outs['bf16x3'])
    assert not torch.equal(outs['f32'], outs['bf16x3'])
    assert err['f32'] < 1e-5 and err['bf16x3'] < 1e-5
    assert err['bf16x3'] < 2 * err['f32'] + 1e-6


def test_integration_md_ctypes_stub_runs_as_written():
    """INTEGRATION.md section 2 shows the ctypes binding a maintainer of the reference would add (handles, struct layouts, the
    three calls that replace p_sample_loop).  The block is executed VERBATIM here -- a stale struct layout in the document (the
    round-3 text lacked SamplerConfig.mean_type) would read garbage or fail -- with the reference-shaped state_dict of the CIFAR net
    and a two-sample state as the names it leaves to the host (`reference_state_dict`, `x`, `t`)."""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    doc = open(os.path.join(root, 'INTEGRATION.md')).read()
    sec = doc[doc.index('## 2. The C ABI'):]
    code = re.search(r'```python\n(.*?)```', sec, re.S).group(1)
    net, _ = build_unet('cifar')
    x = torch.randn(2, 3, 32, 32, device=DEV)
    env = dict(reference_state_dict=net.state_dict(), x=x, t=torch.full((2,), 0.5, device=DEV))
    cwd = os.getcwd()
    os.chdir(root)                      # the stub loads 'dlpm_amd/lib/libdlpm_amd.so' relative to the repository root
    try:
        exec(compile(code, 'INTEGRATION.md', 'exec'), env)
    finally:
        os.chdir(cwd)
    torch.cuda.synchronize()
    eps, out = env['eps'], env['out']
    want = net(x, torch.full((2,), 0.5, device=DEV))
    assert torch.equal(eps, want)                                   # the stub's dlpm_unet_forward == the Python wrapper's
    assert out.shape == (2, 3, 32, 32) and bool(torch.isfinite(out).all())
    env['L'].dlpm_sampler_destroy(env['smp'])
    env['L'].dlpm_unet_destroy(env['net'])
