"""Sample-quality metrics on the device.  One is built: the multi-bandwidth Gaussian MMD of the reference
(bem/evaluate/mmd_loss.py:5-37, `MMD_loss(kernel_mul, kernel_num)(source, target)`, called at EvaluationManager.py:153).

    mmd(source, target) -> float                      dlpm_mmd_f32: tiled pairwise reduction, no n x n array
    MMD_loss(kernel_mul, kernel_num)(source, target)  drop-in for the reference's class: a 0-dim fp32 tensor

Inputs are float32 tensors or arrays [N, ...] (rows are flattened), on the host or the GPU; host inputs are copied once.
Unequal counts are allowed (the reference's broadcast raises on them): sum XX / n1^2 + sum YY / n2^2 - 2 sum XY / (n1 n2).
`wass`, the PRD precision / recall and FID / PRDC need packages and weights that are not available and are not built; neither are
the reference's unused get_MMD / MMDStatistic / MMD helpers."""
import numpy as np
import torch

from . import _lib

MAX_KERNELS = 16


def _points(a, name):
    t = torch.as_tensor(a)
    assert t.dtype == torch.float32, 'mmd takes float32 %s, got %s' % (name, t.dtype)
    assert t.dim() >= 1 and t.shape[0] >= 1 and t.numel() >= t.shape[0], 'mmd: %s needs at least one point, got shape %s' % (
        name, tuple(t.shape))
    return t.reshape(t.shape[0], -1)


def _check(source, target, kernel_mul, kernel_num, fix_sigma):
    x, y = _points(source, 'source'), _points(target, 'target')
    assert x.shape[1] == y.shape[1], 'mmd: source rows hold %d values, target rows %d' % (x.shape[1], y.shape[1])
    assert int(kernel_num) == kernel_num and 1 <= kernel_num <= MAX_KERNELS, 'mmd: kernel_num must be in [1, %d], got %r' % (
        MAX_KERNELS, kernel_num)
    assert kernel_mul > 0, 'mmd: kernel_mul must be positive, got %r' % (kernel_mul,)
    sigma = float(fix_sigma) if fix_sigma else 0.0          # the reference's `if fix_sigma:` -- None and 0 mean "from the data"
    assert sigma >= 0.0, 'mmd: fix_sigma must be positive, got %r' % (fix_sigma,)
    return x, y, float(kernel_mul), int(kernel_num), sigma


def mmd_device(source, target, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """The call itself, without a host synchronisation: a float64 [5] tensor on the GPU holding
    (mmd, bandwidth before the division by kernel_mul ** (kernel_num // 2), sum XX, sum YY, sum XY).
    Enqueued on the current stream; it can be captured in a torch.cuda.graph."""
    x, y, mul, num, sigma = _check(source, target, kernel_mul, kernel_num, fix_sigma)
    dev = x.device if x.is_cuda else (y.device if y.is_cuda else torch.device('cuda', torch.cuda.current_device()))
    x, y = x.to(dev).contiguous(), y.to(dev).contiguous()
    L = _lib.lib()
    n1, n2, D = x.shape[0], y.shape[0], x.shape[1]
    nbytes = L.dlpm_mmd_workspace_bytes(n1, n2, D)
    if nbytes < 0:
        _lib.check(int(nbytes))
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(5, dtype=torch.float64, device=dev)
        _lib.check(L.dlpm_mmd_f32(x.data_ptr(), n1, y.data_ptr(), n2, D, mul, num, sigma, ws.data_ptr(), nbytes, out.data_ptr(),
                                  _lib.stream_ptr()))
    return out


def mmd(source, target, kernel_mul=2.0, kernel_num=5, fix_sigma=None, return_parts=False):
    """MMD between two sample sets as a Python float.  `return_parts=True` returns (mmd, parts) with parts = {'bandwidth', 'xx', 'yy',
    'xy', 'n1', 'n2'}: the bandwidth before the ladder's division and the three quadrant sums of the kernel matrix, so that
    mmd == xx / n1**2 + yy / n2**2 - 2 * xy / (n1 * n2)."""
    out = mmd_device(source, target, kernel_mul, kernel_num, fix_sigma).cpu().numpy()
    if not return_parts:
        return float(out[0])
    n1, n2 = int(np.shape(source)[0]), int(np.shape(target)[0])
    return float(out[0]), {'bandwidth': float(out[1]), 'xx': float(out[2]), 'yy': float(out[3]), 'xy': float(out[4]), 'n1': n1, 'n2': n2}


class MMD_loss(torch.nn.Module):
    """bem/evaluate/mmd_loss.py:5-37: same constructor, same `fix_sigma` attribute (None until the caller sets it); the call returns a
    0-dim float32 tensor on the device of `source` (forward only: no gradient flows through it)."""

    def __init__(self, kernel_mul=2.0, kernel_num=5):
        super().__init__()
        self.kernel_num = kernel_num
        self.kernel_mul = kernel_mul
        self.fix_sigma = None

    def forward(self, source, target):
        out = mmd_device(source, target, self.kernel_mul, self.kernel_num, self.fix_sigma)[0].to(torch.float32)
        return out if torch.as_tensor(source).is_cuda else out.cpu()
