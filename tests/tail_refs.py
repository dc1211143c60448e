"""Host mirror of the tail figures (include/dlpm_amd_tail.h) in numpy, the authority for their definition, and the
error bound the device is held to.  Everything the device adds in a fixed order is added here in the same order:

  * marginal 'norm': v_i = float32(sqrt(sum_d float64(x_id)^2)), d ascending from 0.0, every product and sum rounded on its own;
    'abs': |x| of every scalar of the flattened set;
  * levels u_j = xi + ((1 - xi) * j) / K in fp64, numpy's 'linear' quantile on the sorted fp32 values taken as fp64;
  * msle: the K terms (log q_x - log q_y)^2 added one after the other, j ascending, then divided by K;
  * Hill: r0 = min(floor(xi (N - 1)), N - 2), k = N - 1 - r0; the k ratios log s[i] - log s[r0] (i = r0 + 1 ...) are cut into RUNS =
    1024 runs of ceil(k / 1024) consecutive ranks, each run added in rank order from 0.0, the runs then added in order; k / sum.

Status 1: a non-finite marginal value, every figure NaN.  Status 2: a quantile <= 0 (msle NaN) or a threshold s[r0] <= 0 (that set's
Hill index NaN)."""
import math

import numpy as np

RUNS = 1024
MARGINALS = ('norm', 'abs')


def marginal_values(x, marginal):
    x = np.asarray(x, np.float32)
    x = x.reshape(x.shape[0], -1)
    if marginal == 'abs':
        return np.abs(x).reshape(-1)
    assert marginal == 'norm', marginal
    acc = np.zeros(x.shape[0], np.float64)
    for d in range(x.shape[1]):                       # sequential over d, vectorised over the rows
        v = x[:, d].astype(np.float64)
        acc = acc + v * v
    with np.errstate(over='ignore', invalid='ignore'):
        return np.sqrt(acc).astype(np.float32)


def r0_of(N, xi):
    return min(math.floor(xi * (N - 1)), N - 2)


def levels_of(xi, K):
    j = np.arange(K, dtype=np.float64)
    return xi + ((1.0 - xi) * j) / K


def quantiles(s, u):
    """numpy's 'linear' rule, written out: s sorted fp32, u fp64 levels."""
    N = len(s)
    h = u * np.float64(N - 1)
    lo = np.minimum(np.floor(h).astype(np.int64), N - 1)
    hi = np.minimum(lo + 1, N - 1)
    a, b = s[lo].astype(np.float64), s[hi].astype(np.float64)
    return a + (h - lo.astype(np.float64)) * (b - a)


def sequential_sum(terms):
    acc = np.float64(0.0)
    for t in terms:
        acc = acc + t
    return acc


def hill_sum(ratios):
    """The k log ratios in RUNS runs of ceil(k / RUNS) consecutive ranks, each from 0.0 in rank order; then the runs in order."""
    k = len(ratios)
    per = -(-k // RUNS)
    padded = np.zeros(RUNS * per, np.float64)         # x + 0.0 == x for the non-negative partial sums
    padded[:k] = ratios
    padded = padded.reshape(RUNS, per)
    part = np.zeros(RUNS, np.float64)
    for t in range(per):
        part = part + padded[:, t]
    return sequential_sum(part)


def hill(s, xi):
    """(index, k, s[r0], the sum S) of one sorted set; NaN index for a threshold <= 0."""
    N = len(s)
    r0 = r0_of(N, xi)
    k = N - 1 - r0
    if not s[r0] > 0:
        return math.nan, k, s[r0], math.nan
    S = hill_sum(np.log(s[r0 + 1:].astype(np.float64)) - np.log(np.float64(s[r0])))
    with np.errstate(divide='ignore'):
        return float(np.float64(k) / S), k, s[r0], float(S)


def mirror(x, y, xi=0.95, levels=100, marginal='norm'):
    """dict: msle, hill (2), k (2), threshold (float32, 2), status, quantiles [2, K], and for the bound: log_max (L), mean_abs_d,
    hill_sum (2)."""
    v = [marginal_values(x, marginal), marginal_values(y, marginal)]
    K = int(levels)
    nan = math.nan
    k = [len(a) - 1 - r0_of(len(a), xi) for a in v]
    if not all(np.isfinite(a).all() for a in v):
        return {'msle': nan, 'hill': [nan, nan], 'k': k, 'threshold': [np.float32(nan)] * 2, 'status': 1,
                'quantiles': np.full((2, K), nan), 'log_max': nan, 'mean_abs_d': nan, 'hill_sum': [nan, nan]}
    s = [np.sort(a) for a in v]
    u = levels_of(xi, K)
    q = np.stack([quantiles(a, u) for a in s])
    hills = [hill(a, xi) for a in s]
    status = 0
    msle, mean_abs_d = nan, nan
    L = float(np.abs(np.log(q[q > 0])).max()) if (q > 0).any() else nan       # over the quantiles that have a logarithm
    if (q > 0).all():
        logs = np.log(q)
        d = logs[0] - logs[1]
        msle = float(sequential_sum(d * d) / np.float64(K))
        mean_abs_d = float(np.abs(d).mean())
    else:
        status = 2
    if any(math.isnan(h[0]) for h in hills):
        status = 2
    return {'msle': msle, 'hill': [h[0] for h in hills], 'k': k, 'threshold': [h[2] for h in hills], 'status': status, 'quantiles': q,
            'log_max': L, 'mean_abs_d': mean_abs_d, 'hill_sum': [h[3] for h in hills]}


# ------------------------------------------------------------------------------------------ the error bound
# ocml's and numpy's fp64 log are within 1 ulp, the interpolation rounds twice.  With L = max |log q| over both sets and all levels a
# log difference d_j carries at most delta = 2^-50 max(1, L): 4 x the 2^-52 (2 L + 3) the roundings add up to.
def delta(L):
    return 2.0 ** -50 * max(1.0, L)


def msle_bound(m):
    """|msle_dev - msle_ref| <= 2 mean|d| delta + delta^2 + 2^-50 msle_ref."""
    dl = delta(m['log_max'])
    return 2.0 * m['mean_abs_d'] * dl + dl * dl + 2.0 ** -50 * m['msle']


def hill_rel_bound(m, which):
    """Relative deviation of a Hill index: k delta / S + 2^-50, S the sum of its k log ratios."""
    return m['k'][which] * delta(m['log_max']) / m['hill_sum'][which] + 2.0 ** -50
