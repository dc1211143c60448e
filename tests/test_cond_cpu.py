"""Class-conditional UNets (num_classes = K, the reference's label_emb) on the host: the parameter container against the reference's
record (F16), the native handle's parameter list, the config switch, the forward's argument checks (all before any device work),
the C entry points' refusals that need no GPU, and the sharding of the labels over ranks."""
import ctypes as C
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import golden
import dlpm_amd
from dlpm_amd import _lib
from dlpm_amd.cli import class_labels
from dlpm_amd.dist import shard_range, sample_sharded
from dlpm_amd.method import _native_kwargs
from dlpm_amd.weights import rerandomize_, state_digest

NETS = ['mnist', 'cifar_narrow']


def cond_net(name, reseed=True):
    f = golden('f16_cond_' + name)
    in_ch, mc, heads, res, hw, K = (int(v) for v in f['cfg'])
    torch.manual_seed(1234)
    net = dlpm_amd.UNetModel(in_ch, mc, in_ch, res, [int(a) for a in f['attn']], channel_mult=[int(m) for m in f['mult']],
                             num_heads=heads, use_scale_shift_norm=True, num_classes=K)
    d0 = state_digest(net)
    if reseed:
        rerandomize_(net, 4321)
    return net, d0, f


def native_config(net, image_size=32):
    cfg = _lib.UNetConfig()
    cfg.in_channels, cfg.model_channels, cfg.out_channels = net.in_channels, net.model_channels, net.out_channels
    cfg.num_res_blocks, cfg.num_heads, cfg.image_size = net.num_res_blocks, net.num_heads, image_size
    cfg.n_mult = len(net.channel_mult)
    for i, m in enumerate(net.channel_mult):
        cfg.channel_mult[i] = m
    cfg.n_attn = len(net.attention_resolutions)
    for i, a in enumerate(net.attention_resolutions):
        cfg.attention_resolutions[i] = a
    return cfg


@pytest.mark.parametrize('name', NETS)
def test_conditional_container_equals_reference_record(name):
    net, d0, f = cond_net(name)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in f['keys']]
    assert list(sd.keys()).index('label_emb.weight') == 4          # right after time_embed.{0,2}.{weight,bias}
    for k, row in zip(sd.keys(), f['shapes']):
        assert tuple(sd[k].shape) == tuple(int(v) for v in row if v >= 0), k
    assert tuple(sd['label_emb.weight'].shape) == (int(f['cfg'][5]), 4 * int(f['cfg'][1]))
    assert d0 == bytes(f['digest_init']).hex()                     # default init under torch.manual_seed, label_emb included
    assert state_digest(net) == bytes(f['digest_final']).hex()     # and the fixtures' re-randomised weights


@pytest.mark.parametrize('name', NETS)
def test_native_parameter_list_equals_module_keys(name):
    net, _, _ = cond_net(name, reseed=False)
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.dlpm_unet_create_conditional(C.byref(native_config(net)), net.num_classes, C.byref(h)))
    try:
        assert L.dlpm_unet_num_classes(h) == net.num_classes
        got = []
        for i in range(L.dlpm_unet_num_params(h)):
            n = _lib.i64()
            got.append((L.dlpm_unet_param_key(h, i, C.byref(n)).decode(), n.value))
        assert got == [(k, v.numel()) for k, v in net.state_dict().items()]
    finally:
        L.dlpm_unet_destroy(h)
    # the unconditional handle of the same geometry: no label_emb, 0 classes
    h = C.c_void_p()
    _lib.check(L.dlpm_unet_create(C.byref(native_config(net)), C.byref(h)))
    try:
        assert L.dlpm_unet_num_classes(h) == 0
        assert L.dlpm_unet_num_params(h) == len(net.state_dict()) - 1
    finally:
        L.dlpm_unet_destroy(h)
    with pytest.raises(ValueError, match='num_classes'):
        _lib.check(L.dlpm_unet_create_conditional(C.byref(native_config(net)), 0, C.byref(h)))


def test_native_refusals_on_a_conditional_net():
    """Checked before any device work: the label-less forwards, the time-embedding table, the LIM sampler."""
    net, _, _ = cond_net('mnist', reseed=False)
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.dlpm_unet_create_conditional(C.byref(native_config(net)), 10, C.byref(h)))
    try:
        dummy = 16      # never dereferenced: every call below is refused on its arguments
        for fn in (L.dlpm_unet_forward, L.dlpm_unet_forward_uniform_t):
            with pytest.raises(ValueError, match='class-conditional'):
                _lib.check(fn(h, dummy, dummy, dummy, 2, dummy, 1 << 20, None))
        rc = L.dlpm_unet_time_embeddings(h, dummy, 4, dummy, dummy, 1 << 20, None)
        assert rc == -3, rc                                        # DLPM_ERR_UNSUPPORTED
        assert 'label' in L.dlpm_last_error().decode()
        cfg = _lib.SamplerConfig()
        cfg.unet, cfg.B, cfg.C, cfg.H, cfg.W, cfg.T, cfg.alpha = h, 2, 1, 32, 32, 11, 1.7
        cfg.clamp_a = cfg.clamp_eps = -1.0
        cfg.flags = _lib.SMP_LIM
        s = C.c_void_p()
        with pytest.raises(_lib.DlpmError, match='LIM'):
            _lib.check(L.dlpm_sampler_create(C.byref(cfg), C.byref(s)))
    finally:
        L.dlpm_unet_destroy(h)
    # labels handed to an unconditional net are refused the same way (the reference's assert, both directions)
    unc = dlpm_amd.UNetModel(1, 32, 1, 2, [2, 4], channel_mult=[1, 2, 2, 2], num_heads=4, use_scale_shift_norm=True)
    h = C.c_void_p()
    _lib.check(L.dlpm_unet_create(C.byref(native_config(unc)), C.byref(h)))
    try:
        with pytest.raises(ValueError, match='class-conditional'):
            _lib.check(L.dlpm_unet_forward_labels(h, 16, 16, 16, 16, 2, 16, 1 << 20, None))
    finally:
        L.dlpm_unet_destroy(h)


def test_config_switch_selects_a_conditional_net_and_shipped_configs_stay_unconditional():
    p = dlpm_amd.load_config('mnist')
    p['model']['class_cond'] = True
    p['data']['num_classes'] = 10
    net = dlpm_amd.init_model_by_parameter(p)
    assert net.num_classes == 10 and tuple(net.state_dict()['label_emb.weight'].shape) == (10, 4 * p['model']['model_channels'])
    p['data'].pop('num_classes')
    with pytest.raises(AssertionError, match='num_classes'):
        dlpm_amd.init_model_by_parameter(p)
    cfg_dir = os.path.join(os.path.dirname(dlpm_amd.__file__), 'configs')
    for fn in sorted(os.listdir(cfg_dir)):
        p = dlpm_amd.load_config(fn[:-4])
        assert not p['model'].get('class_cond', False), fn
        m = dlpm_amd.init_model_by_parameter(p)
        assert getattr(m, 'num_classes', None) is None, fn
        assert not any(k.startswith('label_emb') for k in m.state_dict()), fn


def test_forward_argument_checks_come_before_any_device_work():
    net, _, _ = cond_net('mnist', reseed=False)
    x, t = torch.zeros(3, 1, 32, 32), torch.zeros(3)         # CPU tensors: any device work would raise DlpmError instead
    with pytest.raises(AssertionError, match='if and only if'):
        net(x, t)
    with pytest.raises(AssertionError):
        net(x, t, torch.zeros(2, dtype=torch.int64))           # y.shape != (B,)
    for bad in ([0, 10, 1], [0, -1, 1]):
        with pytest.raises(IndexError):
            net(x, t, torch.tensor(bad))
    with pytest.raises(AssertionError, match='if and only if'):
        net.get_feature_vectors(x, t)
    with pytest.raises(IndexError):
        net.get_feature_vectors(x, t, torch.tensor([0, 1, 10]))
    with pytest.raises(_lib.DlpmError, match='no CPU fallback'):
        net(x, t, torch.tensor([0, 9, 3]))                     # valid arguments: only now the device is looked at
    unc = dlpm_amd.UNetModel(1, 32, 1, 2, [2, 4], channel_mult=[1, 2, 2, 2], num_heads=4, use_scale_shift_norm=True)
    with pytest.raises(AssertionError, match='if and only if'):
        unc(x, t, torch.tensor([0, 1, 2]))


def test_native_path_selection_and_cli_labels():
    net, _, _ = cond_net('mnist', reseed=False)
    unc = dlpm_amd.UNetModel(1, 32, 1, 2, [2, 4], channel_mult=[1, 2, 2, 2], num_heads=4, use_scale_shift_norm=True)
    y = torch.tensor([1, 2])
    assert _native_kwargs(net, {'y': y}) and not _native_kwargs(net, None) and not _native_kwargs(net, {'y': y, 'z': 1})
    assert _native_kwargs(unc, None) and _native_kwargs(unc, {}) and not _native_kwargs(unc, {'y': y})
    assert torch.equal(class_labels('cycle', 10, 23), torch.arange(23) % 10)
    assert torch.equal(class_labels('7', 10, 5), torch.full((5,), 7))
    assert class_labels(None, None, 5) is None
    for spec, K in (('10', 10), ('cycle', None), (None, 10)):
        with pytest.raises(SystemExit):
            class_labels(spec, K, 5)


class LabelMethod:
    """sample() returns a pure function of the GLOBAL sample index and of each sample's label (model_kwargs['y'])."""

    def __init__(self, offset):
        self.offset = offset

    def sample(self, models, shape, reverse_steps, model_kwargs=None, **kw):
        y = model_kwargs['y']
        assert y.shape == (shape[0],)
        idx = torch.arange(self.offset, self.offset + shape[0], dtype=torch.float32)
        return (idx + 1000 * y.float()).view(-1, 1, 1, 1) * torch.ones(shape) + reverse_steps


def _worker(rank, world, port, total, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        y = (torch.arange(total) * 7) % 10
        full = sample_sharded(lambda off: LabelMethod(off), None, [total, 1, 2, 2], 10, model_kwargs={'y': y})
        q.put((rank, full.clone()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('total', [8, 7])
def test_two_rank_sampling_slices_the_labels(total):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 2000) + total
    procs = [ctx.Process(target=_worker, args=(r, 2, port, total, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = LabelMethod(0).sample(None, [total, 1, 2, 2], 10, model_kwargs={'y': (torch.arange(total) * 7) % 10})
    assert shard_range(total, 1, 2)[0] > 0
    for rank, full in got:
        assert torch.equal(full, want), rank
