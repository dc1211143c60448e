"""Sample-quality metrics on the device.  Five are built: the multi-bandwidth Gaussian MMD of the reference
(bem/evaluate/mmd_loss.py:5-37, `MMD_loss(kernel_mul, kernel_num)(source, target)`, called at EvaluationManager.py:153), its PRD
precision / recall (bem/evaluate/prd_score.py, prd_legacy.py:6-16, called at EvaluationManager.py:157-168), its Wasserstein figure
(bem/evaluate/wasserstein.py:47-52 = pyemd.emd_samples, called at EvaluationManager.py:146-151) and PRDC FROM FEATURES: the
precision / recall / density / coverage of the `prdc` package's compute_prdc (the last line of bem/evaluate/fid_score.py:303-336),
which is k-nearest-neighbour geometry on two [N, F] arrays and needs no weights; and the FRECHET DISTANCE FROM FEATURES
(calculate_frechet_distance, fid_score.py:118-171, on np.mean / np.cov statistics), which is what FID is once the features exist.

    mmd(source, target) -> float                      dlpm_mmd_f32: tiled pairwise reduction, no n x n array
    MMD_loss(kernel_mul, kernel_num)(source, target)  drop-in for the reference's class: a 0-dim fp32 tensor
    kmeans(points, K) -> centres, labels, ...         dlpm_kmeans_f32: all run x init instances in one grid
    prd(eval_data, ref_data) -> precision, recall     dlpm_prd_f32: clustering, histograms, curve and F pair in one enqueue sequence
    compute_prd_from_embedding, compute_precision_recall_curve, prd_to_max_f_beta_pair, compute_f_beta
                                                      drop-ins under the reference's names and signatures
    wass(first, second, bins='auto') -> float         dlpm_wass_f32: histogram earth mover's distance in closed form
    compute_wasserstein_distance(data, gen_samples)   drop-in for the reference's function (its histogram branch)
    prdc(real, fake, nearest_k=5) -> dict             dlpm_prdc_f32: k-NN radii by streaming selection, fp64 distances
    compute_prdc(real_features, fake_features, nearest_k)   drop-in for the `prdc` package's function
    fd(real, fake) -> float                           dlpm_fd_f32: fp64 covariances on the MFMA, two Jacobi eigen-solves
    feature_statistics(features) -> mu, sigma         dlpm_fd_stats_f32: the device version of calculate_activation_statistics
    calculate_frechet_distance(mu1, sigma1, mu2, sigma2)    drop-in for the reference's function, dlpm_fd_from_stats_f64

Inputs are float32 tensors or arrays [N, ...] (rows are flattened), on the host or the GPU; host inputs are copied once.
Unequal counts are allowed (the reference's broadcast raises on them): sum XX / n1^2 + sum YY / n2^2 - 2 sum XY / (n1 n2).
Not built: any Inception forward -- the network needs weights nobody can ship; bring the features (`prdc`, `fd`,
`EvaluationManager.evaluate_prdc(features=...)`, `evaluate_fid(features=...)`).  Neither are the reference's
unused get_MMD / MMDStatistic / MMD helpers.  The `manual_compute` branch of compute_wasserstein_distance stays refused under that name; its
figure is `compute_w1_distance`:

    w1(first, second, ground='l1_mean') -> float      dlpm_w1_f32: exact optimal transport between equal-count point sets by an
                                                      integer auction
    compute_w1_distance(data, gen_samples, num_samples)   the manual_compute branch's figure

The reference has no figure that sees a tail; for the alpha-stable models this package is about there are two:

    tail(first, second, xi=0.95, levels=100, marginal='norm') -> dict   dlpm_tail_f32: MSLE between upper quantiles and the Hill
                                                      tail index of each set, on exact order statistics
    msle(real, gen, ...) -> float, hill_index(x, xi=0.95, marginal='norm') -> float"""
import numpy as np
import torch

from . import _lib

MAX_KERNELS = 16


def _rows(a, who, name):
    """Input `name` of the metric `who` as a float32 [N, D] tensor where it lives, rows flattened."""
    t = torch.as_tensor(a)
    assert t.dtype == torch.float32, '%s takes float32 %s, got %s' % (who, name, t.dtype)
    assert t.dim() >= 1 and t.shape[0] >= 1 and t.numel() >= t.shape[0], '%s: %s needs at least one point, got shape %s' % (
        who, name, tuple(t.shape))
    return t.reshape(t.shape[0], -1)


def _row_pair(who, a, name_a, b, name_b):
    x, y = _rows(a, who, name_a), _rows(b, who, name_b)
    assert x.shape[1] == y.shape[1], '%s: %s rows hold %d values, %s rows %d' % (who, name_a, x.shape[1], name_b, y.shape[1])
    return x, y


def _on_device(x, y):
    """(x, y, device): both contiguous on the GPU either of them is on, else on the current one.  Called after every refusal."""
    dev = x.device if x.is_cuda else (y.device if y.is_cuda else torch.device('cuda', torch.cuda.current_device()))
    return x.to(dev).contiguous(), y.to(dev).contiguous(), dev


def _workspace(nbytes, dev):
    """The answer of a *_workspace_bytes call as a uint8 tensor of that size on `dev`; a negative answer is its error code."""
    if nbytes < 0:
        _lib.check(int(nbytes))
    with torch.cuda.device(dev):
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _check(source, target, kernel_mul, kernel_num, fix_sigma):
    x, y = _row_pair('mmd', source, 'source', target, 'target')
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
    x, y, dev = _on_device(x, y)
    L = _lib.lib()
    n1, n2, D = x.shape[0], y.shape[0], x.shape[1]
    ws = _workspace(L.dlpm_mmd_workspace_bytes(n1, n2, D), dev)
    with torch.cuda.device(dev):
        out = torch.empty(5, dtype=torch.float64, device=dev)
        _lib.check(L.dlpm_mmd_f32(x.data_ptr(), n1, y.data_ptr(), n2, D, mul, num, sigma, ws.data_ptr(), ws.numel(), out.data_ptr(),
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


# ---------------------------------------------------------------------------------------------- PRD precision / recall
MAX_CLUSTERS = 256
MAX_WIDTH = 4096
KMEANS_TOL = 1e-4          # sklearn's default: rounds stop at a centre shift <= tol * mean per-feature variance
PRD_EPSILON = 1e-10        # compute_prd's default angle offset


def _prd_check(eval_data, ref_data, num_clusters, num_runs, n_init, max_iter):
    x, y = _row_pair('prd', eval_data, 'eval_data', ref_data, 'ref_data')
    assert x.shape[1] <= MAX_WIDTH, 'prd: rows of at most %d values, got %d' % (MAX_WIDTH, x.shape[1])
    n = x.shape[0] + y.shape[0]
    assert int(num_clusters) == num_clusters and 1 <= num_clusters <= min(MAX_CLUSTERS, n), (
        'prd: num_clusters must be in [1, min(%d, number of points = %d)], got %r' % (MAX_CLUSTERS, n, num_clusters))
    for v, name in ((num_runs, 'num_runs'), (n_init, 'n_init'), (max_iter, 'max_iter')):
        assert int(v) == v and v >= 1, 'prd: %s must be a positive integer, got %r' % (name, v)
    assert num_runs * n_init <= 65535, 'prd: num_runs * n_init must be at most 65535'
    return _on_device(x, y)


def _curve_check(num_angles, epsilon, beta):
    if not (int(num_angles) == num_angles and 3 <= num_angles <= 1e6):          # prd_score.py:78-81 raises ValueError on these
        raise ValueError('num_angles must be in [3, 1e6] but is %s.' % (num_angles,))
    if not 0 < epsilon < 0.1:
        raise ValueError('epsilon must be in (0, 0.1] but is %s.' % str(epsilon))
    if beta <= 0:
        raise ValueError('Given parameter beta %s must be positive.' % str(beta))


def _kmeans_device(x, y, dev, K, runs, n_init, max_iter, seed, tol, first_run):
    L = _lib.lib()
    n1, n2, D = x.shape[0], y.shape[0], x.shape[1]
    ws = _workspace(L.dlpm_prd_workspace_bytes(n1, n2, D, K, runs, n_init), dev)
    nbytes = ws.numel()
    with torch.cuda.device(dev):
        centres = torch.empty((runs, K, D), dtype=torch.float64, device=dev)
        labels = torch.empty((runs, n1 + n2), dtype=torch.uint8, device=dev)
        counts = torch.empty((runs, 2, K), dtype=torch.int32, device=dev)
        inertia = torch.empty(runs, dtype=torch.float64, device=dev)
        iters = torch.empty(runs, dtype=torch.int32, device=dev)
        conv = torch.empty(runs, dtype=torch.int32, device=dev)
        _lib.check(L.dlpm_kmeans_f32(x.data_ptr(), n1, y.data_ptr(), n2, D, K, runs, n_init, max_iter, float(tol), int(seed), first_run,
                                     ws.data_ptr(), nbytes, centres.data_ptr(), labels.data_ptr(), counts.data_ptr(), inertia.data_ptr(),
                                     iters.data_ptr(), conv.data_ptr(), _lib.stream_ptr()))
    return centres, labels, counts, inertia, iters, conv


def kmeans(points, K, n_init=10, max_iter=100, seed=0, runs=1, tol=KMEANS_TOL, first_run=0):
    """Full-batch k-means of float32 `points` [n >= 2, ...]: `runs` independent clusterings, each the best of `n_init` k-means++
    seedings (lowest inertia, lowest index on ties), all runs x inits advancing together on the device.  Returns numpy arrays
    (centres [runs, K, D] float64, labels [runs, n] uint8, inertia [runs] float64, iterations [runs], converged [runs] bool).
    Rounds stop at a centre shift <= tol * mean per-feature variance (sklearn's rule); `converged` is set where a round left
    every centre unchanged, i.e. every centre IS the mean of the points labelled with it (always reached with tol=0 and enough
    rounds).  Run r draws from (seed, first_run + r): it is the same whether computed alone or beside others."""
    pts = _rows(points, 'prd', 'points')
    assert pts.shape[0] >= 2, 'kmeans: needs at least two points, got %d' % pts.shape[0]
    assert tol >= 0, 'kmeans: tol must not be negative, got %r' % (tol,)
    assert int(first_run) == first_run and first_run >= 0, 'kmeans: first_run must be a non-negative integer, got %r' % (first_run,)
    h = pts.shape[0] // 2
    x, y, dev = _prd_check(pts[:h], pts[h:], K, runs, n_init, max_iter)
    centres, labels, counts, inertia, iters, conv = _kmeans_device(x, y, dev, int(K), int(runs), int(n_init), int(max_iter), seed, tol,
                                                                   int(first_run))
    return (centres.cpu().numpy(), labels.cpu().numpy(), inertia.cpu().numpy(), iters.cpu().numpy(), conv.cpu().numpy().astype(bool))


def _prd_run(eval_data, ref_data, num_clusters, num_angles, num_runs, n_init, max_iter, seed, centers, beta, epsilon, parts):
    _curve_check(num_angles, epsilon, beta)
    K, A = num_clusters, int(num_angles)
    if centers is not None:
        c = torch.as_tensor(centers)
        assert c.dtype == torch.float64 and c.dim() == 3, 'prd: centers must be float64 [runs, clusters, D], got %s %s' % (
            c.dtype, tuple(c.shape))
        num_runs, K, n_init = int(c.shape[0]), int(c.shape[1]), 1
    x, y, dev = _prd_check(eval_data, ref_data, K, num_runs, n_init, max_iter)
    K, R = int(K), int(num_runs)
    n1, n2, D = x.shape[0], y.shape[0], x.shape[1]
    L = _lib.lib()
    ws = _workspace(L.dlpm_prd_workspace_bytes(n1, n2, D, K, R, int(n_init)), dev)
    nbytes = ws.numel()
    with torch.cuda.device(dev):
        out = torch.empty(2 * A + 3, dtype=torch.float64, device=dev)
        extra = None
        if centers is not None:
            assert c.shape[2] == D, 'prd: centers hold %d values per row, the points %d' % (c.shape[2], D)
            c = c.to(dev).contiguous()
            labels = torch.empty((R, n1 + n2), dtype=torch.uint8, device=dev)
            counts = torch.empty((R, 2, K), dtype=torch.int32, device=dev)
            inertia = torch.empty(R, dtype=torch.float64, device=dev)
            _lib.check(L.dlpm_prd_histograms_f32(x.data_ptr(), n1, y.data_ptr(), n2, D, K, R, c.data_ptr(), ws.data_ptr(), nbytes,
                                                 labels.data_ptr(), counts.data_ptr(), inertia.data_ptr(), _lib.stream_ptr()))
            _lib.check(L.dlpm_prd_curve_f64(counts.data_ptr(), n1, n2, K, R, A, float(epsilon), float(beta), ws.data_ptr(), nbytes,
                                            out.data_ptr(), _lib.stream_ptr()))
            extra = (c, labels, counts)
        else:
            if parts:
                extra = (torch.empty((R, K, D), dtype=torch.float64, device=dev), torch.empty((R, n1 + n2), dtype=torch.uint8, device=dev),
                         torch.empty((R, 2, K), dtype=torch.int32, device=dev))
            ptrs = [t.data_ptr() for t in extra] if extra else [None, None, None]
            _lib.check(L.dlpm_prd_f32(x.data_ptr(), n1, y.data_ptr(), n2, D, K, R, int(n_init), int(max_iter), KMEANS_TOL, int(seed), A,
                                      float(epsilon), float(beta), ws.data_ptr(), nbytes, ptrs[0], ptrs[1], ptrs[2], out.data_ptr(),
                                      _lib.stream_ptr()))
    return out, extra


def prd_device(eval_data, ref_data, num_clusters=20, num_angles=1001, num_runs=10, n_init=10, max_iter=100, seed=0, centers=None,
               beta=8, epsilon=PRD_EPSILON):
    """The call itself, without a host synchronisation: a float64 [2 * num_angles + 3] tensor on the GPU holding precision[A],
    recall[A], max F_beta, max F_1/beta and the largest precision / recall of any run before clipping.  Enqueued on the current
    stream; it can be captured in a torch.cuda.graph."""
    return _prd_run(eval_data, ref_data, num_clusters, num_angles, num_runs, n_init, max_iter, seed, centers, beta, epsilon, False)[0]


def _raise_above_one(out):
    if float(out[-1]) > 1.001:                                     # prd_score.py:99-101
        raise ValueError('Detected value > 1.001, this should not happen.')


def prd(eval_data, ref_data, num_clusters=20, num_angles=1001, num_runs=10, n_init=10, max_iter=100, seed=0, centers=None,
        return_parts=False):
    """PRD curve of `eval_data` against `ref_data` (prd_score.py:139-191): (precision, recall), float64 arrays [num_angles].
    `centers` [runs, clusters, D] float64 skips the clustering (num_runs, num_clusters and n_init then come from its shape).
    `return_parts=True` adds a dict: 'centers' [R, K, D] float64, 'labels' [R, n1 + n2] uint8 (eval points first), 'eval_bins' and
    'ref_bins' [R, K] int32 counts, 'f_beta' = (max F_8, max F_1/8)."""
    out, extra = _prd_run(eval_data, ref_data, num_clusters, num_angles, num_runs, n_init, max_iter, seed, centers, 8, PRD_EPSILON,
                          return_parts)
    o = out.cpu().numpy()
    _raise_above_one(o)
    A = int(num_angles)
    if not return_parts:
        return o[:A], o[A:2 * A]
    counts = extra[2].cpu().numpy()
    return o[:A], o[A:2 * A], {'centers': extra[0].cpu().numpy(), 'labels': extra[1].cpu().numpy(), 'eval_bins': counts[:, 0],
                               'ref_bins': counts[:, 1], 'f_beta': (float(o[2 * A]), float(o[2 * A + 1]))}


def compute_prd_from_embedding(eval_data, ref_data, num_clusters=20, num_angles=1001, num_runs=10, enforce_balance=True):
    """prd_score.py:139-191 under its own name and signature.  ValueError on unequal counts unless enforce_balance=False; unequal
    counts then work, each set's histogram normalised by its own count."""
    if enforce_balance and len(eval_data) != len(ref_data):
        raise ValueError('The number of points in eval_data %d is not equal to the number of points in ref_data %d. To disable this '
                         'exception, set enforce_balance to False (not recommended).' % (len(eval_data), len(ref_data)))
    return prd(eval_data, ref_data, num_clusters=num_clusters, num_angles=num_angles, num_runs=num_runs)


def compute_precision_recall_curve(data, gen_samples, num_angles=201, num_clusters=20):
    """prd_legacy.py:6-11 under its own name and signature, argument order included: the REAL data goes in as `eval_data` and the
    generated samples as `ref_data` (so the reference's 'precision' figure is F_8 of that orientation).  Kept as it is, not "fixed":
    the figures are compared with the reference's."""
    n = len(data)
    data, gen = torch.as_tensor(data), torch.as_tensor(gen_samples)
    return compute_prd_from_embedding(data.reshape(n, -1), gen.reshape(n, -1), num_angles=num_angles, num_clusters=num_clusters)


def prd_to_max_f_beta_pair(precision, recall, beta=8):
    """prd_score.py:230-262 on the host (a few hundred values): (max F_beta, max F_1/beta) of a curve."""
    precision, recall = np.asarray(precision, np.float64), np.asarray(recall, np.float64)
    if not ((precision >= 0).all() and (precision <= 1).all()):
        raise ValueError('All values in precision must be in [0, 1].')
    if not ((recall >= 0).all() and (recall <= 1).all()):
        raise ValueError('All values in recall must be in [0, 1].')
    if beta <= 0:
        raise ValueError('Given parameter beta %s must be positive.' % str(beta))

    def f(b):
        return np.max((1 + b ** 2) * (precision * recall) / ((b ** 2 * precision) + recall + 1e-10))
    return f(beta), f(1 / beta)


def compute_f_beta(prec, rec):
    """prd_legacy.py:13-15."""
    a, b = prd_to_max_f_beta_pair(prec, rec)
    return np.array([a, b])


# ---------------------------------------------------------------------------------------------- Wasserstein (histogram EMD)
MAX_BINS = 1 << 20
_WASS_STATUS = {1: 'autodetected range is not finite', 2: 'supplied range is not finite',
                3: 'max must be larger than min in range parameter.', 4: 'Too many bins for data range'}


def _wass_check(first, second, bins, range, max_bins):
    x, y = _row_pair('wass', first, 'first', second, 'second')
    assert int(max_bins) == max_bins and 1 <= max_bins <= MAX_BINS, 'wass: max_bins must be in [1, %d], got %r' % (MAX_BINS, max_bins)
    if isinstance(bins, str):
        if bins != 'auto':
            raise ValueError('%r is not a built estimator for `bins`: \'auto\' or an integer' % (bins,))
        nb = 0
    else:
        nb = int(bins)
        if nb != bins:
            raise TypeError('`bins` must be an integer or \'auto\'')
        if nb < 1:
            raise ValueError('`bins` must be positive, when an integer')             # numpy's own refusal
        assert nb <= max_bins, 'wass: %d bins, max_bins is %d' % (nb, max_bins)
    lo, hi, has = 0.0, 0.0, 0
    if range is not None:
        lo, hi = (float(v) for v in range)
        has = 1
    return x, y, nb, has, lo, hi, int(max_bins)


def _wass_run(first, second, bins, range, max_bins, parts):
    x, y, nb, has, lo, hi, max_bins = _wass_check(first, second, bins, range, max_bins)
    x, y, dev = _on_device(x, y)
    L = _lib.lib()
    n1, n2, D = x.shape[0], y.shape[0], x.shape[1]
    ws = _workspace(L.dlpm_wass_workspace_bytes(n1, n2, D, max_bins), dev)
    with torch.cuda.device(dev):
        out = torch.empty(12, dtype=torch.float64, device=dev)
        hist = torch.empty((2, max_bins), dtype=torch.int32, device=dev) if parts else None
        _lib.check(L.dlpm_wass_f32(x.data_ptr(), n1, y.data_ptr(), n2, D, nb, has, lo, hi, max_bins, ws.data_ptr(), ws.numel(),
                                   hist.data_ptr() if parts else None, out.data_ptr(), _lib.stream_ptr()))
    return out, hist


def wass_device(first, second, bins='auto', range=None, max_bins=MAX_BINS):
    """The call itself, without a host synchronisation: a float64 [12] tensor on the GPU holding (wass, bins, lo, hi, bin width, q25,
    q75, the four order statistics, status).  status != 0 (a non-finite value or range, more than max_bins bins) leaves wass NaN;
    `wass` raises numpy's ValueError on it.  Enqueued on the current stream; it can be captured in a torch.cuda.graph."""
    return _wass_run(first, second, bins, range, max_bins, False)[0]


def wass(first, second, bins='auto', range=None, return_parts=False):
    """pyemd.emd_samples(first, second, bins=bins, range=range) with its defaults (Euclidean distance between bin centres, normalised
    histograms) as a Python float: both arrays flattened, np.histogram's bins over the pooled range, and the 1-D earth mover's
    distance between the two histograms.  `bins`: an integer or 'auto' (numpy's rule on the pooled values).  `range`: None (pooled
    min / max) or (lo, hi); values outside are dropped.  ValueError as numpy for non-finite data or a bad range.
    `return_parts=True` returns (wass, parts) with parts = {'bins', 'lo', 'hi', 'width', 'q25', 'q75', 'order_stats' (float32 [4]: the
    sorted pooled values at ranks floor / ceil of the 75 % and of the 25 % point), 'hist_first', 'hist_second' (int32 [bins])};
    q25, q75 and order_stats are None unless bins='auto'.  Under 'auto' the call reserves room for as many bins as there are values
    (at least 1024) and repeats itself with 2^20 for the rare set that needs more."""
    if isinstance(bins, str):
        # 'auto': numpy's count is not known before the call.  Room for as many bins as there are values (at least 1024) keeps the
        # workspace, the returned histograms and the LDS of the histogram pass small at the toy sizes; the rare set that needs more
        # (a tiny IQR in a wide range) is run again with the full 2^20
        max_bins = min(MAX_BINS, max(1024, 1 << (torch.as_tensor(first).numel() + torch.as_tensor(second).numel() - 1).bit_length()))
    else:
        max_bins = max(int(bins), 1)
    out, hist = _wass_run(first, second, bins, range, max_bins, return_parts)
    o = out.cpu().numpy()
    status = int(o[11])
    if status == 4 and max_bins < MAX_BINS:
        out, hist = _wass_run(first, second, bins, range, MAX_BINS, return_parts)
        o = out.cpu().numpy()
        status = int(o[11])
    if status:
        raise ValueError(_WASS_STATUS[status] + ' (wass)')
    if not return_parts:
        return float(o[0])
    nb, auto = int(o[1]), isinstance(bins, str)
    h = hist[:, :nb].cpu().numpy()
    return float(o[0]), {'bins': nb, 'lo': float(o[2]), 'hi': float(o[3]), 'width': float(o[4]), 'q25': float(o[5]) if auto else None,
                         'q75': float(o[6]) if auto else None, 'order_stats': o[7:11].astype(np.float32) if auto else None,
                         'hist_first': h[0], 'hist_second': h[1]}


def compute_wasserstein_distance(data, gen_samples, manual_compute=False, num_samples=-1, distance='euclidean', normalized=True,
                                 bins='auto', _range=None):
    """bem/evaluate/wasserstein.py:15-52 under its own name and signature, quirks included: the default num_samples=-1 slices
    `[:-1]`, so the LAST sample of each set is left out, and the generated samples go in first.  Kept as they are, not "fixed": the
    figures are compared with the reference's.  Not built: manual_compute=True (a general 2N x 2N transport problem), a
    callable or other `distance`, normalized=False."""
    if manual_compute:
        raise NotImplementedError('compute_wasserstein_distance: manual_compute=True is a general 2N x 2N transport problem; only the '
                                  'histogram form is built here (DESIGN 8) -- metrics.compute_w1_distance gives that branch\'s figure')
    if distance != 'euclidean':
        raise NotImplementedError('compute_wasserstein_distance: only distance=\'euclidean\' between bin centres is built (DESIGN 8)')
    if not normalized:
        raise NotImplementedError('compute_wasserstein_distance: normalized=False is not built (DESIGN 8)')
    return wass(gen_samples[:num_samples], data[:num_samples], bins=bins, range=_range)


# ---------------------------------------------------------------------------------------------- exact W1 (integer auction)
W1_MAX_POINTS = 32768
W1_MAX_WIDTH = 4096
W1_GROUNDS = {'l1_mean': _lib.W1_L1_MEAN, 'euclidean': _lib.W1_EUCLIDEAN}
W1_TAIL_THRESHOLD = 4              # rounds with at most this many bidders run in the one-workgroup kernel: the best of {0, 4, 16, 64}
#                                    at N = 1024 and 4096 in every configuration of profiles/w1
W1_ROUNDS_COEF, W1_ROUNDS_POWER = 15, 1.25   # the most rounds seen at n points stay below 15 n^1.25 for n = 256 ... 8192 (profiles/w1)


def w1_default_max_rounds(n):
    """The cap on the auction's rounds when none is given: 16 x the largest round count measured at that n, which over n = 256 ...
    8192 grows like n^1.25 (15 153 rounds at 256, 1 165 974 at 8192; at most 15 n^1.25 everywhere in profiles/w1), so
    16 * 15 * max(n, 64)^1.25.  A guard against a spin, not a tuning value; nothing beyond 8192 points has been measured."""
    return int(16 * W1_ROUNDS_COEF * max(int(n), 64) ** W1_ROUNDS_POWER)


def _w1_check(first, second, ground, max_rounds, tail_threshold):
    x, y = _row_pair('w1', first, 'first', second, 'second')
    assert x.shape[0] == y.shape[0], 'w1: equal counts needed, got %d and %d points (compute_w1_distance cuts both to the shorter)' % (
        x.shape[0], y.shape[0])
    assert x.shape[0] <= W1_MAX_POINTS, 'w1: at most %d points, got %d' % (W1_MAX_POINTS, x.shape[0])
    assert x.shape[1] <= W1_MAX_WIDTH, 'w1: rows of at most %d values, got %d' % (W1_MAX_WIDTH, x.shape[1])
    if ground not in W1_GROUNDS:
        raise ValueError('w1: ground must be one of %s, got %r' % (sorted(W1_GROUNDS), ground))
    n = x.shape[0]
    max_rounds = w1_default_max_rounds(n) if max_rounds is None else max_rounds
    tail_threshold = W1_TAIL_THRESHOLD if tail_threshold is None else tail_threshold
    assert int(max_rounds) == max_rounds and max_rounds >= 1, 'w1: max_rounds must be a positive integer, got %r' % (max_rounds,)
    assert int(tail_threshold) == tail_threshold and tail_threshold >= 0, 'w1: tail_threshold must be a non-negative integer, got %r' % (
        tail_threshold,)
    return x, y, W1_GROUNDS[ground], int(max_rounds), int(tail_threshold)


def _w1_run(first, second, ground, max_rounds, tail_threshold):
    """w1_device and the cap on the rounds that the call ran under."""
    x, y, g, max_rounds, tail_threshold = _w1_check(first, second, ground, max_rounds, tail_threshold)
    x, y, dev = _on_device(x, y)
    L = _lib.lib()
    n, D = x.shape
    ws = _workspace(L.dlpm_w1_workspace_bytes(n, D), dev)
    with torch.cuda.device(dev):
        out = torch.empty(8, dtype=torch.float64, device=dev)
        perm = torch.empty(n, dtype=torch.int32, device=dev)
        prices = torch.empty(n, dtype=torch.int64, device=dev)
        _lib.check(L.dlpm_w1_f32(x.data_ptr(), y.data_ptr(), n, D, g, max_rounds, tail_threshold, ws.data_ptr(), ws.numel(),
                                 perm.data_ptr(), prices.data_ptr(), out.data_ptr(), _lib.stream_ptr()))
    return out, perm, prices, max_rounds


def w1_device(first, second, ground='l1_mean', max_rounds=None, tail_threshold=None):
    """The call itself: (out, perm, prices) on the GPU -- out float64 [8] = W, the integer optimum, the scale exponent e, rounds,
    phases, cmax, status, rounds run by the one-workgroup kernel; perm int32 [n] (row perm[i] of `second` is matched with row i of
    `first`); prices int64 [n].  status 1 (a non-finite input value) and 2 (max_rounds reached) leave W NaN.  No synchronisation
    beyond the call's own: it is enqueued on the current stream but NOT graph-capturable, since the host reads the device's header
    once per batch of rounds."""
    return _w1_run(first, second, ground, max_rounds, tail_threshold)[:3]


def w1(first, second, ground='l1_mean', return_parts=False):
    """The exact Wasserstein-1 distance between two sets of n float32 points (rows flattened), every point of mass 1 / n, as a Python
    float: (1 / n) min over permutations s of sum_i c(first_i, second_s(i)) with c = mean_d |a_d - b_d| (ground='l1_mean', the cost
    of the reference's manual_compute branch) or the Euclidean distance (ground='euclidean').  The assignment is exactly optimal for
    the costs rounded to 24-bit integers; the figure is the fp64 cost of that assignment, so 0 <= w1 - optimum <= 2^-e.
    ValueError on a non-finite input value, RuntimeError if the round cap is reached.
    `return_parts=True` returns (w1, parts) with parts = {'perm' int32 [n], 'prices' int64 [n], 'rounds', 'phases', 'scale_exponent',
    'cmax', 'integer_cost'}."""
    out, perm, prices, max_rounds = _w1_run(first, second, ground, None, None)
    o = out.cpu().numpy()
    if int(o[6]) == 1:
        raise ValueError('w1: a non-finite value in the input')
    if int(o[6]) == 2:
        raise RuntimeError('w1: the auction has not ended within the cap of max_rounds = %d rounds' % max_rounds)
    if not return_parts:
        return float(o[0])
    return float(o[0]), {'perm': perm.cpu().numpy(), 'prices': prices.cpu().numpy(), 'rounds': int(o[3]), 'phases': int(o[4]),
                         'scale_exponent': int(o[2]), 'cmax': float(o[5]), 'integer_cost': int(o[1])}


def compute_w1_distance(data, gen_samples, num_samples=-1):
    """The figure of the reference's compute_wasserstein_distance(data, gen_samples, manual_compute=True, num_samples=...)
    (bem/evaluate/wasserstein.py:23-46): N = min of the two counts, or num_samples when it is not -1; the first N rows of each set;
    one bin of mass 1 / N per point and the mean absolute difference as ground distance -- `w1(..., ground='l1_mean')`."""
    n = min(len(data), len(gen_samples)) if num_samples == -1 else int(num_samples)
    assert 1 <= n <= min(len(data), len(gen_samples)), 'compute_w1_distance: num_samples = %r with %d and %d points' % (
        num_samples, len(data), len(gen_samples))
    return w1(data[:n], gen_samples[:n], ground='l1_mean')


# ---------------------------------------------------------------------------------------------- tail figures (upper-quantile MSLE, Hill index)
TAIL_MARGINALS = {'norm': _lib.TAIL_NORM, 'abs': _lib.TAIL_ABS}
TAIL_MAX_LEVELS = 65536


def _tail_check(first, second, xi, levels, marginal):
    x, y = _row_pair('tail', first, 'first', second, 'second')
    if marginal not in TAIL_MARGINALS:
        raise ValueError('tail: marginal must be one of %s, got %r' % (sorted(TAIL_MARGINALS), marginal))
    assert x.shape[0] >= 2 and y.shape[0] >= 2, 'tail: at least 2 samples a set, got %d and %d' % (x.shape[0], y.shape[0])
    assert 0.5 <= xi < 1.0, 'tail: xi must be in [0.5, 1), got %r' % (xi,)
    assert int(levels) == levels and 1 <= levels <= TAIL_MAX_LEVELS, 'tail: levels must be in [1, %d], got %r' % (TAIL_MAX_LEVELS, levels)
    return x, y, float(xi), int(levels), TAIL_MARGINALS[marginal]


def _tail_run(first, second, xi, levels, marginal, parts):
    x, y, xi, K, m = _tail_check(first, second, xi, levels, marginal)
    x, y, dev = _on_device(x, y)
    L = _lib.lib()
    n1, n2, D = x.shape[0], y.shape[0], x.shape[1]
    ws = _workspace(L.dlpm_tail_workspace_bytes(n1, n2, D, m, xi, K), dev)
    with torch.cuda.device(dev):
        out = torch.empty(8, dtype=torch.float64, device=dev)
        q = torch.empty((2, K), dtype=torch.float64, device=dev) if parts else None
        _lib.check(L.dlpm_tail_f32(x.data_ptr(), n1, y.data_ptr(), n2, D, m, xi, K, ws.data_ptr(), ws.numel(),
                                   q.data_ptr() if parts else None, out.data_ptr(), _lib.stream_ptr()))
    return out, q


def tail_device(first, second, xi=0.95, levels=100, marginal='norm'):
    """The call itself, without a host synchronisation: a float64 [8] tensor on the GPU holding (msle, Hill index of `first`, Hill
    index of `second`, k and the threshold s[r0] of `first`, k and s[r0] of `second`, status).  status 1 (a non-finite value) leaves
    the figures NaN, status 2 (a quantile or a threshold <= 0) the affected ones.  Enqueued on the current stream; it can be captured
    in a torch.cuda.graph."""
    return _tail_run(first, second, xi, levels, marginal, False)[0]


def tail(first, second, xi=0.95, levels=100, marginal='norm', return_parts=False):
    """The tail figures of two float32 sample sets (rows flattened, unequal counts allowed) as a dict {'msle', 'tail_index_first',
    'tail_index_second'}.  Each set becomes a vector of non-negative values: marginal='norm' the Euclidean norm of every
    sample, 'abs' |x| of every scalar, as `wass` flattens.  `msle` is the mean squared difference of the logarithms of their quantiles
    at the `levels` levels xi + (1 - xi) j / levels, j = 0 .. levels - 1 (numpy's 'linear' quantiles; the maximum itself is left out);
    `tail_index_*` the Hill estimate k / sum_{i > r0} log(s[i] / s[r0]) on the k = N - 1 - r0 largest values of a set, r0 = min(floor(xi
    (N - 1)), N - 2).  The order statistics are exact (radix select, exact sort), every sum runs in a fixed order: same inputs, same bits.

    Ties are handled: a tail that is one repeated value has index +inf.  That is what a CLAMP looks like -- GenerationManager._post
    clamps 2-D samples to +-6 and data.quantile_cutoff < 1 clamps the real set -- so choose xi below the clamped fraction.
    ValueError on a non-finite value.  Where a quantile or a threshold is <= 0 (no logarithm) the affected figures are NaN.
    `return_parts=True` adds 'k' (2 ints), 'thresholds' (the two s[r0]) and 'quantiles' (float64 [2, levels])."""
    out, q = _tail_run(first, second, xi, levels, marginal, return_parts)
    o = out.cpu().numpy()
    if int(o[7]) == 1:
        raise ValueError('tail: a non-finite value in the input')
    res = {'msle': float(o[0]), 'tail_index_first': float(o[1]), 'tail_index_second': float(o[2])}
    if return_parts:
        res.update(k=(int(o[3]), int(o[5])), thresholds=(float(o[4]), float(o[6])), quantiles=q.cpu().numpy())
    return res


def msle(real, gen, xi=0.95, levels=100, marginal='norm'):
    """The upper-quantile mean squared logarithmic error of `tail` alone, as a Python float."""
    return tail(real, gen, xi, levels, marginal)['msle']


def hill_index(x, xi=0.95, marginal='norm'):
    """The Hill tail index of one set (`tail`'s tail_index_first), as a Python float."""
    return tail(x, x, xi, 1, marginal)['tail_index_first']


# ---------------------------------------------------------------------------------------------- PRDC (k-NN precision / recall / density / coverage)
MAX_NEAREST_K = 32


def f_1(a, b):
    """EvaluationManager.py:215-225: 2 a b / (a + b), or 0 when a + b is 0 (f_1_pr of precision / recall, f_1_dc of density / coverage)."""
    return 2 * a * b / (a + b) if a + b > 0 else 0.


def _prdc_check(who, real, fake, nearest_k):
    x, y = _row_pair(who, real, 'real', fake, 'fake')
    assert int(nearest_k) == nearest_k and 1 <= nearest_k <= MAX_NEAREST_K, '%s: nearest_k must be an integer in [1, %d], got %r' % (
        who, MAX_NEAREST_K, nearest_k)
    assert nearest_k < min(x.shape[0], y.shape[0]), '%s: nearest_k = %d needs more than %d points in both sets, got %d and %d' % (
        who, nearest_k, nearest_k, x.shape[0], y.shape[0])
    return x, y, int(nearest_k)


def prdc_device(real, fake, nearest_k=5, return_radii=False):
    """The call itself, without a host synchronisation: (out, counts) on the GPU -- out float64 [8] = precision, recall, density,
    coverage, f_1_pr, f_1_dc, status, reserved; counts int64 [4] = precision hits, recall hits, density pair count, coverage hits.
    status 1 (a non-finite input value) leaves the six figures NaN.  `return_radii=True` returns (out, counts, radii_real [n1],
    radii_fake [n2]), float64: the distance of every point to its nearest_k-th neighbour within its own set.  Enqueued on the
    current stream; it can be captured in a torch.cuda.graph."""
    x, y, k = _prdc_check('prdc', real, fake, nearest_k)
    x, y, dev = _on_device(x, y)
    L = _lib.lib()
    n1, n2, D = x.shape[0], y.shape[0], x.shape[1]
    ws = _workspace(L.dlpm_prdc_workspace_bytes(n1, n2, D, k), dev)
    with torch.cuda.device(dev):
        out = torch.empty(8, dtype=torch.float64, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        rr = torch.empty(n1, dtype=torch.float64, device=dev) if return_radii else None
        rf = torch.empty(n2, dtype=torch.float64, device=dev) if return_radii else None
        _lib.check(L.dlpm_prdc_f32(x.data_ptr(), n1, y.data_ptr(), n2, D, k, ws.data_ptr(), ws.numel(), rr.data_ptr() if return_radii else None,
                                   rf.data_ptr() if return_radii else None, counts.data_ptr(), out.data_ptr(), _lib.stream_ptr()))
    return (out, counts, rr, rf) if return_radii else (out, counts)


def prdc(real, fake, nearest_k=5, return_parts=False, return_radii=False):
    """precision, recall, density and coverage (Kynkaanniemi et al. 2019, Naeem et al. 2020; the `prdc` package) of `fake` rows
    against `real` rows as a dict of Python floats.  With k = nearest_k: the radius of a point is its distance to its k-th nearest
    neighbour within its own set (the (k+1)-th smallest of its row of distances, itself included); precision = share of fake points
    inside some real ball, recall = share of real points inside some fake ball, density = number of (real ball, fake point)
    incidences / (k n_fake), coverage = share of real points whose nearest fake point lies inside their own ball; every comparison
    strict.  Distances are fp64; rows of more than 16 values go through the centred Gram form, where ties are those of fp64 rounding,
    not of exact arithmetic.  ValueError on a non-finite input value.
    `return_parts=True` returns (dict, parts) with parts = {'counts': int64 [4] (precision hits, recall hits, density pair count,
    coverage hits), 'n1', 'n2', 'nearest_k'}, and with `return_radii=True` also 'radii_real' [n1] and 'radii_fake' [n2], float64."""
    res = prdc_device(real, fake, nearest_k, return_radii=return_parts and return_radii)
    o = res[0].cpu().numpy()
    if int(o[6]):
        raise ValueError('prdc: a non-finite value in the input')
    figures = {'precision': float(o[0]), 'recall': float(o[1]), 'density': float(o[2]), 'coverage': float(o[3])}
    if not return_parts:
        return figures
    parts = {'counts': res[1].cpu().numpy(), 'n1': int(np.shape(real)[0]), 'n2': int(np.shape(fake)[0]), 'nearest_k': int(nearest_k)}
    if return_radii:
        parts['radii_real'], parts['radii_fake'] = res[2].cpu().numpy(), res[3].cpu().numpy()
    return figures, parts


def compute_prdc(real_features, fake_features, nearest_k):
    """The `prdc` package's compute_prdc under its own name and keyword names: dict(precision, recall, density, coverage) of two
    [N, F] feature arrays.  float32 or float64 arrays or tensors; float64 is rounded to float32 ONCE on the way in (the package
    works on whatever it is given; the distances themselves are fp64 here as there)."""
    def f32(a, name):
        t = torch.as_tensor(a)
        assert t.dtype in (torch.float32, torch.float64), 'compute_prdc takes float32 or float64 %s, got %s' % (name, t.dtype)
        return t.to(torch.float32)
    real, fake = f32(real_features, 'real_features'), f32(fake_features, 'fake_features')
    _prdc_check('compute_prdc', real, fake, nearest_k)
    return prdc(real, fake, nearest_k=nearest_k)


# ---------------------------------------------------------------------------------------------- Frechet distance from features
MAX_FEATURES = 4096
FD_MAX_SWEEPS = 60


def _fd_rows(who, a, name):
    x = _rows(a, who, name)
    assert x.shape[0] >= 2, '%s: a covariance needs at least 2 rows, %s has %d' % (who, name, x.shape[0])
    assert x.shape[1] <= MAX_FEATURES, '%s: rows of at most %d values, %s has %d (bring an embedding: features=)' % (
        who, MAX_FEATURES, name, x.shape[1])
    return x


def _fd_check(who, real, fake):
    x, y = _fd_rows(who, real, 'real'), _fd_rows(who, fake, 'fake')
    assert x.shape[1] == y.shape[1], '%s: real rows hold %d values, fake rows %d' % (who, x.shape[1], y.shape[1])
    return x, y


def _fd_raise(o):
    if int(o[5]) == 1:
        raise ValueError('fd: a non-finite value in the input')
    if int(o[5]) == 2:
        raise RuntimeError('fd: a Jacobi solve still rotated in sweep %d (sweeps %d and %d)' % (FD_MAX_SWEEPS, int(o[6]), int(o[7])))


def fd_device(real, fake):
    """The call itself: a float64 [8] tensor on the GPU holding (fd, |mu1 - mu2|^2, tr sigma1, tr sigma2, tr (sigma1 sigma2)^1/2, status,
    sweeps of the eigen-solve of sigma1, sweeps of the eigen-solve of K).  status 1 (a non-finite input value) leaves the five figures
    NaN; status 2: a solve still rotated in its 60th sweep.  Enqueued on the current stream, but NOT graph-capturable: the host reads
    the device's rotation counter once per Jacobi sweep, so the call waits on the stream."""
    x, y = _fd_check('fd', real, fake)
    x, y, dev = _on_device(x, y)
    L = _lib.lib()
    n1, n2, F = x.shape[0], y.shape[0], x.shape[1]
    ws = _workspace(L.dlpm_fd_workspace_bytes(n1, n2, F), dev)
    with torch.cuda.device(dev):
        out = torch.empty(8, dtype=torch.float64, device=dev)
        _lib.check(L.dlpm_fd_f32(x.data_ptr(), n1, y.data_ptr(), n2, F, ws.data_ptr(), ws.numel(), out.data_ptr(), _lib.stream_ptr()))
    return out


def _feature_statistics(x, dev):
    L = _lib.lib()
    n, F = x.shape
    ws = _workspace(L.dlpm_fd_workspace_bytes(n, n, F), dev)
    with torch.cuda.device(dev):
        mu = torch.empty(F, dtype=torch.float64, device=dev)
        sigma = torch.empty((F, F), dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(L.dlpm_fd_stats_f32(x.data_ptr(), n, F, ws.data_ptr(), ws.numel(), mu.data_ptr(), sigma.data_ptr(), status.data_ptr(),
                                       _lib.stream_ptr()))
    return mu, sigma, status


def feature_statistics(features):
    """(mu [F], sigma [F, F]), float64 tensors on the GPU: np.mean(features, axis=0) and np.cov(features, rowvar=False) of float32
    `features` [N >= 2, ...] (rows flattened, at most 4096 values) -- the device version of calculate_activation_statistics
    (fid_score.py:173-193) without its network.  sigma is symmetric bit for bit.  ValueError on a non-finite input value."""
    x = _fd_rows('feature_statistics', features, 'features')
    x, _, dev = _on_device(x, x)
    mu, sigma, status = _feature_statistics(x, dev)
    if int(status.cpu()[0]):
        raise ValueError('feature_statistics: a non-finite value in the input')
    return mu, sigma


def _from_stats(mu1, sigma1, mu2, sigma2, dev):
    L = _lib.lib()
    F = mu1.shape[0]
    ws = _workspace(L.dlpm_fd_workspace_bytes(2, 2, F), dev)
    with torch.cuda.device(dev):
        out = torch.empty(8, dtype=torch.float64, device=dev)
        _lib.check(L.dlpm_fd_from_stats_f64(mu1.data_ptr(), sigma1.data_ptr(), mu2.data_ptr(), sigma2.data_ptr(), F, ws.data_ptr(), ws.numel(),
                                            out.data_ptr(), _lib.stream_ptr()))
    return out


def fd(real, fake, return_parts=False):
    """Frechet distance between the Gaussians fitted to the float32 rows `real` [n1 >= 2, ...] and `fake` [n2 >= 2, ...] (flattened,
    at most 4096 values) as a Python float: |mu1 - mu2|^2 + tr sigma1 + tr sigma2 - 2 tr (sigma1 sigma2)^1/2, in fp64 on the device.
    It is not clamped: as in the reference it may come out slightly negative for (nearly) equal sets.  ValueError on a non-finite
    input value, RuntimeError if an eigen-solve has not converged in 60 sweeps.
    `return_parts=True` returns (fd, parts) with parts = {'mu1', 'sigma1', 'mu2', 'sigma2' (float64 device tensors), 'mean_term',
    'tr_sigma1', 'tr_sigma2', 'tr_sqrt', 'sweeps' (of the two solves), 'n1', 'n2'}; the figure is the same bits either way."""
    if not return_parts:
        o = fd_device(real, fake).cpu().numpy()
        _fd_raise(o)
        return float(o[0])
    x, y = _fd_check('fd', real, fake)
    x, y, dev = _on_device(x, y)
    mu1, sigma1, st1 = _feature_statistics(x, dev)
    mu2, sigma2, st2 = _feature_statistics(y, dev)
    if int(st1.cpu()[0]) or int(st2.cpu()[0]):
        raise ValueError('fd: a non-finite value in the input')
    o = _from_stats(mu1, sigma1, mu2, sigma2, dev).cpu().numpy()
    _fd_raise(o)
    return float(o[0]), {'mu1': mu1, 'sigma1': sigma1, 'mu2': mu2, 'sigma2': sigma2, 'mean_term': float(o[1]), 'tr_sigma1': float(o[2]),
                         'tr_sigma2': float(o[3]), 'tr_sqrt': float(o[4]), 'sweeps': (int(o[6]), int(o[7])), 'n1': int(x.shape[0]),
                         'n2': int(y.shape[0])}


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """fid_score.py:118-171 under its own name and argument names, on the device: float64 arrays or tensors mu [F], sigma [F, F]
    (symmetric; F <= 4096), returns a Python float.  `eps` is accepted and unused: the reference adds it to both diagonals when
    fractional_matrix_power of the (nearly) singular product sigma1 sigma2 comes out non-finite; the symmetric form used here
    (eigenvalues of sigma1^1/2 sigma2 sigma1^1/2) has no such branch and no imaginary parts.  ValueError / RuntimeError as `fd`."""
    def f64(a, name, dims):
        t = torch.as_tensor(a)
        assert t.dtype == torch.float64, 'calculate_frechet_distance takes float64 %s, got %s' % (name, t.dtype)
        t = t.reshape(1) if (dims == 1 and t.dim() == 0) else t
        t = t.reshape(1, 1) if (dims == 2 and t.dim() < 2 and t.numel() == 1) else t
        assert t.dim() == dims, 'calculate_frechet_distance: %s must have %d dimension(s), got shape %s' % (name, dims, tuple(t.shape))
        return t
    m1, s1, m2, s2 = f64(mu1, 'mu1', 1), f64(sigma1, 'sigma1', 2), f64(mu2, 'mu2', 1), f64(sigma2, 'sigma2', 2)
    assert m1.shape == m2.shape, 'Training and test mean vectors have different lengths'                # the reference's own words
    assert s1.shape == s2.shape, 'Training and test covariances have different dimensions'
    F = m1.shape[0]
    assert s1.shape == (F, F), 'calculate_frechet_distance: sigma must be [%d, %d], got %s' % (F, F, tuple(s1.shape))
    assert 1 <= F <= MAX_FEATURES, 'calculate_frechet_distance: at most %d features, got %d' % (MAX_FEATURES, F)
    dev = next((t.device for t in (m1, s1, m2, s2) if t.is_cuda), None) or torch.device('cuda', torch.cuda.current_device())
    m1, s1, m2, s2 = (t.to(dev).contiguous() for t in (m1, s1, m2, s2))
    o = _from_stats(m1, s1, m2, s2, dev).cpu().numpy()
    _fd_raise(o)
    return float(o[0])
