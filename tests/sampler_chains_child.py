"""Child process of test_gpu_sampler_chains.py: DLPM_SAMPLER_CHAINS is read once per process, so every setting samples in a
process of its own.  Runs every scenario of the tests with the setting it inherits and stores the final states, the chain count
the sampler reports and its capture counter in the .npz named on the command line."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import dlpm_amd
from dlpm_amd import _lib
from dlpm_amd.weights import rerandomize_

DEV = 'cuda'
T, ALPHA, STEPS = 9, 1.7, 8          # T - 1 = 8 reverse steps
KW = dict(clamp_a=10.0, clamp_eps=50.0)
BATCHES = (4, 5, 2)


def tiny(num_classes=None):
    """the 'tiny' UNet of the sampler tests (test_host_mirror.UNETS): 3 x 16 x 16 images"""
    torch.manual_seed(1234)
    net = dlpm_amd.UNetModel(3, 32, 3, 1, [2], channel_mult=[1, 2], num_heads=4, use_scale_shift_norm=True,
                             **({} if num_classes is None else {'num_classes': num_classes}))
    rerandomize_(net, 4321)
    return net


def handle_of(m):
    (ent,) = m._samplers.values()
    return ent['h']


def sample(net, B, offset=0, graph=True, seed=42, **kw):
    m = dlpm_amd.GenerativeLevyProcess(ALPHA, DEV, T, rescale_timesteps=True, seed=seed, sample_offset=offset, use_graph=graph)
    x = m.sample({'default': net}, [B, 3, 16, 16], T, **dict(KW, **kw)).cpu().numpy()
    L = _lib.lib()
    info = (L.dlpm_sampler_chains(handle_of(m)), L.dlpm_sampler_graph_captures(handle_of(m)))
    m.close()
    return x, info


def native(net, B, seed, offset):
    m = dlpm_amd.GenerativeLevyProcess(ALPHA, DEV, T, rescale_timesteps=True)
    return m, m._native_sampler(net, [B, 3, 16, 16], 0, 0.0, 10.0, 50.0, seed, offset)


def state(h, B):
    x = torch.empty(B, 3, 16, 16, device=DEV)
    _lib.check(_lib.lib().dlpm_sampler_copy_state(h, x.data_ptr(), _lib.stream_ptr()))
    return x


def main(out_path):
    L, st = _lib.lib(), _lib.stream_ptr()
    out = {}
    net = tiny()
    for B in BATCHES:
        net.set_conv_policy('auto', B)          # the declared dispatch batch of the whole call, for the shards too
        out['full_B%d' % B], info = sample(net, B)
        out['info_B%d' % B] = np.array(info)
        lo = B // 2
        out['shard_lo_B%d' % B] = sample(net, lo, 0)[0]
        out['shard_hi_B%d' % B] = sample(net, B - lo, lo)[0]
    net.set_conv_policy('auto', 4)
    out['eager_B4'] = sample(net, 4, graph=False)[0]

    # reseed and set_state under a live graph
    B = 4
    m0, h = native(net, B, 42, 0)
    _lib.check(L.dlpm_sampler_begin(h, st))
    _lib.check(L.dlpm_sampler_steps(h, STEPS, st))
    out['native_first'] = state(h, B).cpu().numpy()
    cap0, ver0 = L.dlpm_sampler_graph_captures(h), L.dlpm_unet_plan_version(net.native_handle(16))
    m1, f = native(net, B, 7, 3)                   # the fresh sampler the reseeded one must reproduce
    _lib.check(L.dlpm_sampler_begin(f, st))
    _lib.check(L.dlpm_sampler_steps(f, 3, st))
    x3 = state(f, B)
    _lib.check(L.dlpm_sampler_steps(f, STEPS - 3, st))
    out['fresh_reseeded'] = state(f, B).cpu().numpy()
    _lib.check(L.dlpm_sampler_reseed(h, 7, 3))
    _lib.check(L.dlpm_sampler_begin(h, st))
    _lib.check(L.dlpm_sampler_steps(h, STEPS, st))
    out['reseeded'] = state(h, B).cpu().numpy()
    _lib.check(L.dlpm_sampler_set_state(h, x3.data_ptr(), T - 1 - 3, st))      # resume the fresh trajectory after its third step
    _lib.check(L.dlpm_sampler_steps(h, STEPS - 3, st))
    out['resumed'] = state(h, B).cpu().numpy()
    out['reseed_counters'] = np.array([cap0, L.dlpm_sampler_graph_captures(h), ver0,
                                       L.dlpm_unet_plan_version(net.native_handle(16)), L.dlpm_sampler_chains(h)])
    m0.close()
    m1.close()

    # the variants that stay on one chain
    out['clip'], info = sample(net, 4, clip_denoised=True)
    out['info_clip'] = np.array(info)
    out['one'], info = sample(net, 1)
    out['info_one'] = np.array(info)
    cnet = tiny(num_classes=10)
    cnet.set_conv_policy('auto', 4)
    out['label'], info = sample(cnet, 4, model_kwargs={'y': torch.tensor([3, 0, 9, 3])})
    out['info_label'] = np.array(info)
    torch.cuda.synchronize()
    np.savez(out_path, **out)


if __name__ == '__main__':
    main(sys.argv[1])
