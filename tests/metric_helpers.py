"""What the tests of the device metrics (mmd, prd, wass) share: the toy model, the managers and the real samples of the end-to-end
tests, and the host buffer whose addresses the refusal tests hand to the C entry points."""
import numpy as np
import torch

import dlpm_amd


def toy():
    torch.manual_seed(1)
    return dlpm_amd.MLPModel(dlpm_amd.load_config('2d_data'))


def managers(shape=(1, 2), is_image=False, **kw):
    """(method, GenerationManager, EvaluationManager) of one evaluation; the defaults are the toy model's."""
    kw = kw or dict(reverse_steps=10)
    method = dlpm_amd.GenerativeLevyProcess(1.7, 'cuda', kw['reverse_steps'], rescale_timesteps=True, seed=9)
    gm = dlpm_amd.GenerationManager(method, dlpm_amd.ShapeProbe(list(shape)), is_image, **kw)
    return method, gm, dlpm_amd.EvaluationManager(method, gm, None, verbose=False, is_image=is_image)


def real_toy(N):
    return torch.randn([N + 8, 1, 2], generator=torch.Generator().manual_seed(41))


def buffers():
    """(a 64 KB host buffer, the first 256-byte aligned address inside it); the caller holds the buffer while it uses addresses."""
    buf = np.zeros(1 << 16, np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    return buf, base
