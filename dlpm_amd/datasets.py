"""The 2-D toy data distributions of bem/datasets (Distributions.py, Data.py, get_dataset) on the device: the real samples a 2-D config
is evaluated against, drawn from the config's own description instead of a data file (include/dlpm_amd_toy.h).

The four generation functions keep the reference's names and arguments and add `seed`, `first_index`, `stream`, `raw` and use `device`:
every random number is a Philox function of (seed, stream, global row, element), so the same call gives the same bits, and for the three
iid kinds (`gmm_2`, `gmm_grid`, `swiss_roll`) row i of a call is global row `first_index + i` whatever the chunking.  `sas_grid` assigns
its components in exact proportions of N, as the reference does, and is drawn whole.  `raw=` ([N, 2] float32) takes the place of the
draw: the normalisation and the quantile clamp then run on the caller's points.  The normalisation and the clamp act on the rows of the
call, as the reference's act on the array they are given.  There is no CPU fallback.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

KINDS = {'gmm_2': 0, 'gmm_grid': 1, 'swiss_roll': 2, 'sas_grid': 3}     # dlpm_toy_kind
STATUS_HIGH_NEGATIVE, STATUS_LOW_POSITIVE = 1, 2
STREAM_TRAIN, STREAM_TEST = 0, 1


def sas_grid_bounds(weights, n_samples):
    """int(idx) of Distributions.py:212-218: the source rows [bounds[k], bounds[k + 1]) belong to component k."""
    idx = np.cumsum(np.concatenate((np.array([0.0]), np.asarray(weights, np.float64)))) * n_samples
    return np.array([int(v) for v in idx], dtype=np.int64)


def _device(device):
    dev = torch.device('cuda' if device is None else device)
    if dev.type != 'cuda':
        raise _lib.DlpmError('the toy data distributions are drawn on the GPU; there is no CPU fallback (device=%s)' % (device,))
    return torch.device('cuda', torch.cuda.current_device()) if dev.index is None else dev


def draw(kind, n_samples, n=None, std=None, theta=1.0, weights=None, alpha=2.0, isotropic=False, seed=0, first_index=0, stream=0,
         device=None, return_perm=False):
    """Stage A: the raw [n_samples, 2] float32 points of `kind` on the device (`return_perm`: and sas_grid's source rows pi(p))."""
    if kind not in KINDS:
        raise ValueError('unknown toy distribution %r; available: %s' % (kind, sorted(KINDS)))
    if std is None:
        raise ValueError('std is required: the %s distribution has no default scale' % kind)
    n_samples = int(n_samples)
    grid = kind in ('gmm_grid', 'sas_grid')
    if grid and n is None:
        raise ValueError('n is required: %s is an n x n grid' % kind)
    a = _lib.ToyDrawArgs()
    a.kind, a.N, a.first_index, a.isotropic = KINDS[kind], n_samples, int(first_index), int(bool(isotropic))
    a.std, a.theta, a.data_alpha = float(std), float(1.0 if theta is None else theta), float(2.0 if alpha is None else alpha)
    a.seed, a.stream = int(seed) & (2 ** 64 - 1), int(stream)
    a.n_mixture = int(n) * int(n) if grid else 0
    w = None
    if kind != 'swiss_roll':
        if weights is None:
            weights = [0.5, 0.5] if kind == 'gmm_2' else [1 / (n * n) for _ in range(n * n)]
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        a.count, a.weights_host = len(w), w.ctypes.data
    if n_samples <= 0:                                 # (before any allocation; the library words the refusal)
        _lib.check(_lib.lib().dlpm_toy_draw_f32(C.byref(a), None))
    dev = _device(device)
    with torch.cuda.device(dev):
        out = torch.empty((n_samples, 2), dtype=torch.float32, device=dev)
        a.out_dev = out.data_ptr()
        keep = []
        if w is not None and np.all(np.isfinite(w)):
            if kind == 'sas_grid':
                keep.append(torch.from_numpy(sas_grid_bounds(w, n_samples)).to(dev))
                a.bounds_dev = keep[-1].data_ptr()
            else:
                keep.append(torch.from_numpy(np.cumsum(w)).to(dev))
                a.cum_dev = keep[-1].data_ptr()
        perm = None
        if return_perm:
            perm = torch.empty(n_samples, dtype=torch.int64, device=dev)
            a.perm_out_dev = perm.data_ptr()
        _lib.check(_lib.lib().dlpm_toy_draw_f32(C.byref(a), _lib.stream_ptr()))
    return (out, perm) if return_perm else out


def finish(x, normalize=False, torch_std=False, between_minus_1_1=False, quantile_cutoff=0.99, return_parts=False, check=True):
    """Stage B in place on the [N, 2] float32 device tensor `x`: (x - m) / s with the scalar moments of all 2 N values (`torch_std`:
    divisor 2 N - 1 as torch.std, else 2 N as numpy), then _between_minus_1_1_with_quantile.  A column whose high quantile is negative
    or whose low quantile is positive -- the reference's two asserts -- raises ValueError.  `return_parts`: (x, the 8 fp64 values m, s,
    hi0, lo0, c0, hi1, lo1, c1 on the host).  `check=False` returns (x, parts, the status word) instead of raising."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == 2 and x.is_contiguous(), (
        'finish takes a contiguous [N, 2] float32 device tensor, got %s %s' % (x.dtype, tuple(x.shape)))
    L, N = _lib.lib(), int(x.shape[0])
    with torch.cuda.device(x.device):
        need = L.dlpm_toy_workspace_bytes(N)
        if need < 0:
            _lib.check(int(need))
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        parts = torch.full((8,), float('nan'), dtype=torch.float64, device=x.device)
        status = torch.zeros(1, dtype=torch.int32, device=x.device)
        _lib.check(L.dlpm_toy_finish_f32(x.data_ptr(), N, int(bool(normalize)), int(bool(torch_std)), int(bool(between_minus_1_1)),
                                         float(quantile_cutoff), ws.data_ptr(), need, parts.data_ptr(), status.data_ptr(),
                                         _lib.stream_ptr()))
        bad = int(status.item()) if between_minus_1_1 else 0
    if not check:
        return x, parts.cpu(), bad
    if bad:
        what = [s for bit, s in ((STATUS_HIGH_NEGATIVE, 'a high quantile is negative'), (STATUS_LOW_POSITIVE, 'a low quantile is positive'))
                if bad & bit]
        raise ValueError('between_minus_1_1 assumes centred data (Distributions.py:97-98): ' + ' and '.join(what))
    return (x, parts.cpu()) if return_parts else x


def _sample(kind, torch_std, n_samples, alpha, n, std, theta, weights, device, normalize, isotropic, between_minus_1_1, quantile_cutoff,
            seed, first_index, raw, stream):
    if raw is not None:
        dev = _device(device)
        x = torch.as_tensor(raw)
        assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == 2 and x.shape[0] == n_samples, (
            'raw must be a float32 [%d, 2] array, got %s %s' % (n_samples, x.dtype, tuple(x.shape)))
        x = x.to(dev, copy=True).contiguous()
    else:
        x = draw(kind, n_samples, n=n, std=std, theta=theta, weights=weights, alpha=alpha, isotropic=isotropic, seed=seed,
                 first_index=first_index, stream=stream, device=device)
    if normalize or between_minus_1_1:
        finish(x, normalize=normalize, torch_std=torch_std, between_minus_1_1=between_minus_1_1, quantile_cutoff=quantile_cutoff)
    return x


def sample_2_gmm(n_samples, alpha=None, n=None, std=None, theta=1.0, weights=None, device=None, normalize=False, isotropic=False,
                 between_minus_1_1=False, quantile_cutoff=0.99, seed=0, first_index=0, raw=None, stream=0):
    """Two Gaussians at (+theta, 0) and (-theta, 0) (Distributions.py:119-144)."""
    return _sample('gmm_2', False, n_samples, alpha, n, std, theta, weights, device, normalize, isotropic, between_minus_1_1,
                   quantile_cutoff, seed, first_index, raw, stream)


def sample_grid_gmm(n_samples, alpha=None, n=None, std=None, theta=None, weights=None, device=None, normalize=False, isotropic=False,
                    between_minus_1_1=False, quantile_cutoff=0.99, seed=0, first_index=0, raw=None, stream=0):
    """n x n Gaussians at (i, j), not centred (Distributions.py:146-175)."""
    return _sample('gmm_grid', False, n_samples, alpha, n, std, theta, weights, device, normalize, isotropic, between_minus_1_1,
                   quantile_cutoff, seed, first_index, raw, stream)


def gen_swiss_roll(n_samples, alpha=None, n=None, std=None, theta=None, weights=None, device=None, normalize=False, isotropic=False,
                   between_minus_1_1=False, quantile_cutoff=0.99, seed=0, first_index=0, raw=None, stream=0):
    """The first and third coordinate of sklearn's make_swiss_roll, always normalised (Distributions.py:178-195)."""
    return _sample('swiss_roll', False, n_samples, alpha, n, std, theta, weights, device, True, isotropic, between_minus_1_1,
                   quantile_cutoff, seed, first_index, raw, stream)


def sample_grid_sas(n_samples, alpha=1.8, n=None, std=None, theta=1.0, weights=None, device=None, normalize=False, isotropic=False,
                    between_minus_1_1=False, quantile_cutoff=0.99, seed=0, first_index=0, raw=None, stream=0):
    """n x n symmetric alpha-stable clouds at (i, j) - (n / 2, n / 2) in exact proportions (Distributions.py:198-231)."""
    return _sample('sas_grid', True, n_samples, alpha, n, std, theta, weights, device, normalize, isotropic, between_minus_1_1,
                   quantile_cutoff, seed, first_index, raw, stream)


_SAMPLERS = {'gmm_2': sample_2_gmm, 'gmm_grid': sample_grid_gmm, 'swiss_roll': gen_swiss_roll, 'sas_grid': sample_grid_sas}
_GRID_KINDS = ('gmm_grid', 'sas_grid')
_ELSEWHERE = {'skewed_levy': 'dlpm_amd.process (DLPM.gen_a)', 'sas': 'dlpm_amd.process (DLPM.gen_eps)'}


class Generator:
    """The interface of the reference's wrapper class (bem/datasets/Data.py): Generator(operation, transform=None, *args, **kwargs)
    stores default arguments for one of the four generation functions, `setParams` changes them, `generate(...)` calls the function
    with the stored arguments overridden by the given ones and keeps the result, after `transform`, in `.samples`."""

    available_distributions = list(_SAMPLERS)

    def __init__(self, operation, transform=None, *args, **kwargs):
        if operation in _ELSEWHERE:
            raise NotImplementedError('the %s draws are not a data distribution here: see %s' % (operation, _ELSEWHERE[operation]))
        if operation not in _SAMPLERS:
            raise Exception('%r is not a toy distribution; choose one of %s' % (operation, ', '.join(_SAMPLERS)))
        self.generator = _SAMPLERS[operation]
        self.transform = transform if transform is not None else _identity
        self.args, self.kwargs, self.samples = tuple(args), dict(kwargs), None

    def setTransform(self, transform):
        self.transform = transform

    def setParams(self, *args, **kwargs):
        """Stored positional arguments are replaced slot by slot where a value other than None is given; keywords are added or replaced."""
        if not args and not kwargs:
            raise Exception('setParams was called without a parameter')
        stored = list(self.args)
        for slot, value in enumerate(args[:len(stored)]):
            if value is not None:
                stored[slot] = value
        self.args = tuple(stored)
        for key, value in kwargs.items():
            self.kwargs[key] = value

    def generate(self, *args, **kwargs):
        if not (args or kwargs or self.kwargs):
            raise Exception('generate needs parameters: none are stored and none are given')
        keywords = dict(self.kwargs)
        keywords.update(kwargs)
        positional = args if args else self.args
        self.samples = self.transform(self.generator(*positional, **keywords))
        return self.samples

    def __len__(self):
        return 0 if self.samples is None else len(self.samples)

    def __getitem__(self, idx):
        return self.samples[idx]


def _identity(x):
    return x


def get_dataset(p, device=None, seed=0):
    """The reference's get_dataset for a 2-D config: (train, test), each a [nsamples, 1, dim] float32 device tensor -- two draws of the
    distribution that `p['data']` describes, under the same seed and two different stream keys.  `dim` = 1 keeps the first coordinate."""
    d = p['data']
    kind = str(d['dataset']).lower()
    if kind not in _SAMPLERS:
        raise ValueError('data.dataset = %s is not available here: the 2-D distributions are %s; the image and toy-image loaders are '
                         'out of scope' % (d['dataset'], ', '.join(_SAMPLERS)))
    if d['dim'] not in (1, 2):
        raise ValueError('data.dim = %r: the toy distributions are 2-D, dim is 2, or 1 for the first coordinate alone' % (d['dim'],))
    missing = [k for k in ('n_mixture', 'std', 'nsamples') if d.get(k) is None]
    if missing:
        raise ValueError('data.%s missing from the config: the distribution is not described' % ', data.'.join(missing))
    settings = dict(std=d['std'], theta=d.get('theta'), weights=d.get('weights'), alpha=d.get('data_alpha'),
                    isotropic=d.get('isotropic', False), normalize=d.get('normalized', False),
                    between_minus_1_1=d.get('between_minus_1_1', False), quantile_cutoff=d.get('quantile_cutoff', 0.99))
    settings['n'] = d['n_mixture']
    if kind in _GRID_KINDS:                                                      # a grid has n x n components
        side = math.isqrt(int(d['n_mixture']))
        if side * side != d['n_mixture']:
            raise ValueError('data.n_mixture = %s is not a perfect square' % d['n_mixture'])
        settings['n'] = side
    gen = Generator(kind, device=device, seed=seed, **settings)
    splits = []
    for stream in (STREAM_TRAIN, STREAM_TEST):
        x = gen.generate(n_samples=d['nsamples'], stream=stream)                 # [nsamples, 2]
        splits.append(x[:, None, :d['dim']].contiguous())
    return tuple(splits)


class ToyLoader:
    """A minimal iterable loader over a [N, 1, dim] tensor: yields (data, y) batches in order, y the reference's zero labels.  It goes
    where the reference passes a torch DataLoader (GenerationManager's `dataloader`)."""

    def __init__(self, data, batch_size):
        assert batch_size > 0
        self.data, self.batch_size = data, int(batch_size)

    def __len__(self):
        return (len(self.data) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for first in range(0, len(self.data), self.batch_size):
            x = self.data[first:first + self.batch_size]
            yield x, torch.zeros(len(x), dtype=torch.float32, device=x.device)
