"""What the CPU and GPU tests of the toy data distributions share: the F23 cases, a NumPy restatement of stage B (the device's
arithmetic: fp64 moments of the fp32 points, one rounding; torch.quantile's nearest ranks in fp32; the clamp in fp32), and the bound of
DESIGN 3.16 on the normalised values."""
import numpy as np

KINDS = ['gmm_2', 'gmm_grid', 'swiss_roll', 'sas_grid']
SIZES = (64, 257, 1000)
U = 2.0 ** -24                       # half an ulp of fp32, relative

# sas_grid's reference moments are torch fp32 sums, for which no clean bound exists: the largest deviation of the
# device's arithmetic from the reference over the three F23 cases is 0.382 B (2.4e-7 absolute), B the bound below, measured 2026-10-18;
# the tests hold it to 4 x that, the margin for torch's summation order changing between versions.
SAS_MEASURED = 0.382
SAS_MARGIN = 4.0


def np_normalize(raw, torch_std):
    """((x - m) / s rounded once to fp32, m, s) with the fp64 moments of the fp32 points, divisor 2 N - 1 for torch's std."""
    x = raw.astype(np.float64)
    m, s = x.mean(), x.std(ddof=1 if torch_std else 0)
    return ((x - m) / s).astype(np.float32), m, s


def norm_bound(kind, out, x, m, s):
    """|device - reference| per element.  The reference rounds fp64 points x to (x - m) / s once; the device sees fl32(x), so its
    moments move by at most u (|m| + s) each (u = 2^-24: |fl32(x) - x| <= u |x|, and mean |x| <= sqrt(m^2 + s^2) <= |m| + s), and each
    side rounds its result once:  u (2 |out|  +  |x| / s  +  (|m| + s) / s  +  |out| (|m| + s) / s)
                                = u (3 |out| + (|x| + |m|) / s + 1 + |out| |m| / s),  first order; 2^-20 covers the second."""
    out, x = np.abs(np.asarray(out, np.float64)), np.abs(np.asarray(x, np.float64))
    b = U * (3 * out + (x + abs(m)) / s + 1 + out * abs(m) / s) * (1 + 2.0 ** -20)
    return b * (SAS_MARGIN * SAS_MEASURED if kind == 'sas_grid' else 1.0)


def nearest_ranks(q, N):
    """torch.quantile(x, q, interpolation='nearest') on an fp32 tensor: q and q * (N - 1) in fp32, round half to even."""
    return (int(np.rint(np.float32(q) * np.float32(N - 1))), int(np.rint(np.float32(1 - q) * np.float32(N - 1))))


def np_between(x, q):
    """(_between_minus_1_1_with_quantile(x, q) in fp32, the status word, (hi, lo, c) per column)."""
    x = np.asarray(x, np.float32)
    srt = np.sort(x, axis=0)
    rh, rl = nearest_ranks(q, len(x))
    hi, lo = srt[rh], srt[rl]
    status = (1 if (hi < 0).any() else 0) | (2 if (lo > 0).any() else 0)
    c = np.maximum(np.abs(hi), np.abs(lo)).astype(np.float32)
    with np.errstate(divide='ignore', invalid='ignore'):
        out = (np.clip(x, -c, c) / c).astype(np.float32)
    return out, status, (hi, lo, c)
