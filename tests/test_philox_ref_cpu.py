"""Pins the host mirror of the device's Philox draws (tests/philox_ref.py); no GPU.

1. Philox4x32-10 against the Random123 known answers.
2. The condition under which cms64 may stand in for cms_mp: 1e-8 relative (1e-7 at alpha = 1.99), tails included.
3. The law of the mirror's a draws (Levy at alpha = 1, scipy's levy_stable quantiles otherwise) and of its normals.
4. The judges of tests/test_gpu_draws.py refuse each of nine wrong kernels at that file's own inputs."""
import math

import numpy as np
import pytest
import scipy.stats

import philox_ref as R
from philox_ref import ALPHAS, OFFSETS, SEED


def hexwords(w):
    return ' '.join('%08x' % int(x) for x in w)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 at 10 rounds."""
    ones = 0xFFFFFFFF
    assert hexwords(R.philox4x32_10(0, 0, 0, 0, 0)) == '6627e8d5 e169c58d bc57ac4c 9b00dbd8'
    assert hexwords(R.philox4x32_10(ones, ones, ones, ones, 0xFFFFFFFFFFFFFFFF)) == '408f276d 41c83b0e a20bc7c6 6d5451fd'
    got = R.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0x299F31D0A4093822)      # key words a4093822 299f31d0
    assert hexwords(got) == 'd16cfe09 94fdcceb 5001e420 24126ea1'
    # vectorised: an array of counters gives the same words, and `words` lays the counter out as documented
    c0 = np.array([0, ones, 0x243F6A88], dtype=np.uint64)
    assert int(R.philox4x32_10(c0, 0, 0, 0, 0)[0][0]) == 0x6627E8D5
    w = R.words(0x299F31D0A4093822, (0x85A308D3 << 32) | 0x243F6A88, 0x13198A2E, 0x44, 0x037073)
    assert hexwords(w) == 'd16cfe09 94fdcceb 5001e420 24126ea1'


def test_uniforms_stay_inside_the_unit_interval_and_round_as_the_device_does():
    top = np.uint64(0xFFFFFFFF)
    u, v = R.uniforms53((top, top, np.uint64(0), np.uint64(0)))
    # above 2^52 the `+ 0.5` of a double rounds to even, so the one largest of the 2^53 values gives 1.0 (uniforms53's docstring)
    assert u == 1.0 and v == 2.0 ** -54
    u, v = R.uniforms53((top, np.uint64(0xFFFFF7FF), np.uint64(1 << 11), np.uint64(1 << 11)))
    assert u == 1.0 - 2.0 ** -52 and v == (2.0 ** 32 + 1.5) * 2.0 ** -53
    # the 24-bit uniforms: exact midpoints below 2^23, rounded to even above, the largest exactly 1.0
    w = tuple(np.uint64(x << 8) for x in (0, (1 << 23) - 1, (1 << 23) + 1, (1 << 24) - 1))
    u24 = R.uniforms24(w)
    assert all(x.dtype == np.float32 for x in u24)
    assert float(u24[0]) == 2.0 ** -25 and float(u24[1]) == ((1 << 23) - 0.5) * 2.0 ** -24
    assert float(u24[2]) == ((1 << 23) + 2) * 2.0 ** -24 and float(u24[3]) == 1.0


@pytest.mark.parametrize('alpha', ALPHAS)
def test_cms64_meets_its_condition_against_mpmath(alpha):
    """200 plain draws and the 32 tail draws of tail_offsets.  A condition on the inputs of the GPU tests, not a measurement:
    the figure printed is the reference's own error (at most 2.8e-9, 7.2e-9 at alpha = 1.99, when this was written)."""
    g = np.concatenate([np.arange(200), R.tail_offsets(SEED, 0, R.P_A, 0)]).astype(np.uint64)
    U, V = R.a_uniforms(SEED, g, 0, R.P_A)
    err = R.rel_err_vs_mp(R.cms64(alpha, U, V), R.cms_mp(alpha, U, V))
    print('alpha %g: max |cms64 - cms_mp| / cms_mp = %.3g' % (alpha, err))
    assert err <= (R.COND_199 if alpha >= 1.99 else R.COND)


def test_tail_offsets_are_the_extremes():
    offs = np.array(R.tail_offsets(SEED, 0, R.P_A, 0), dtype=np.uint64)
    assert offs.shape == (32,) and offs.max() < 1 << 22
    U, V = R.a_uniforms(SEED, offs, 0, R.P_A)
    # of 2^22 uniforms the 8 smallest lie below 8 / 2^22 with all but vanishing probability (a Gamma(8) tail beyond 4 x its mean)
    lim = 32.0 / (1 << 22)
    assert U[:8].max() < lim and U[8:16].min() > 1 - lim and V[16:24].max() < lim and V[24:].min() > 1 - lim


def mirror_a(alpha, n):
    U, V = R.a_uniforms(SEED, np.arange(n, dtype=np.uint64), 0, R.P_A)
    return R.cms64(alpha, U, V)


def test_mirror_a_is_levy_at_alpha_one():
    a = mirror_a(1.0, 1 << 18)
    p = scipy.stats.kstest(a, scipy.stats.levy(scale=2 * math.cos(math.pi / 4) ** 2).cdf).pvalue
    print('KS p-value against Levy: %.3g' % p)
    assert p > 1e-3


@pytest.mark.parametrize('alpha', [1.5, 1.7, 1.9])
def test_mirror_a_has_the_stable_quantiles(alpha):
    n = 1 << 18
    a = mirror_a(alpha, n)
    qs = np.array([0.01, 0.1, 0.5, 0.9, 0.99, 0.999])
    x = scipy.stats.levy_stable.ppf(qs, alpha / 2, 1, loc=0, scale=R.cms_scale(alpha))
    share = (a[None, :] < x[:, None]).mean(axis=1)
    sig = np.abs(share - qs) / np.sqrt(qs * (1 - qs) / n)
    print('alpha %g: share below the quantiles off by %s binomial sigma' % (alpha, np.round(sig, 2)))
    assert sig.max() < 5
    # the chosen tail draws lie where no quantile test of a few thousand draws reaches: beyond the 0.999 quantile, by orders
    Ut, Vt = R.a_uniforms(SEED, np.array(R.tail_offsets(SEED, 0, R.P_A, 0), dtype=np.uint64), 0, R.P_A)
    assert R.cms64(alpha, Ut, Vt).max() > 100 * x[-1]


def test_mirror_normals_are_standard():
    n = 1 << 18                                                     # quads: 2^20 normals
    z = R.normal4(SEED, np.arange(n, dtype=np.uint64), 0, R.P_STEP_Z, 7).ravel()
    m = z.size
    assert abs(z.mean()) < 5 / math.sqrt(m) and abs(z.var() - 1) < 5 * math.sqrt(2.0 / m)
    assert abs((z ** 4).mean() - 3) < 5 * math.sqrt(96.0 / m)       # Var z^4 = 105 - 9
    assert scipy.stats.kstest(z, 'norm').pvalue > 1e-3
    # the lanes of a quad, and neighbouring quads, are uncorrelated
    z4 = z.reshape(n, 4)
    c = np.corrcoef(z4.T)
    assert np.abs(c - np.eye(4)).max() < 5 / math.sqrt(n)


# ---------------------------------------------------------------- the judges refuse wrong kernels
def a_case(alpha, offset, mut=None, purpose=R.P_A, elem=False):
    """The inputs of test_gpu_draws' a cases (T = 3, B = 4, D = 5 for the element form) and what a kernel with `mut` would return."""
    T, B, D = 3, 4, 5
    g = (np.int64(offset) + np.arange(B)).astype(np.uint64)
    if elem:
        gi, w2, w3 = np.broadcast_arrays(g[None, :, None], np.arange(D)[None, None, :], np.arange(T)[:, None, None])
    else:
        gi, w2, w3 = np.broadcast_arrays(g[None, :], np.arange(T)[:, None], 0)
    U, V = R.a_uniforms(SEED, gi, w2, purpose, w3)
    Um, Vm = R.a_uniforms(SEED, gi, w2, purpose, w3, mut=mut)
    return R.cms64(alpha, Um, Vm, mut=mut).astype(np.float32), U, V


def z_case(offset, D, t, mut=None):
    g = (np.int64(offset) + np.arange(3)).astype(np.uint64)
    return R.normals(SEED, g, D, R.P_STEP_Z, t, mut=mut).astype(np.float32), R.normals(SEED, g, D, R.P_STEP_Z, t)


def test_the_judges_accept_the_mirror_itself():
    for alpha in ALPHAS:
        for off in OFFSETS:
            got, U, V = a_case(alpha, off)
            R.judge_a(got, alpha, U, V)
            R.judge_a(np.minimum(got, np.float32(10.0)), alpha, U, V, clamp=10.0)
        got, U, V = a_case(alpha, 0)
        R.judge_a(got[0, :2], alpha, U[0, :2], V[0, :2], mp=True)
    got, ref = z_case(OFFSETS[1], 5, 2)
    assert R.judge_z(got, ref) < 1e-6


@pytest.mark.parametrize('mut', ['swap_words', 'nine_rounds'])
def test_wrong_philox_rounds_are_refused(mut):
    """Words 1 and 3 exchanged move only the low 21 bits of U and V, 2^-32 relative, which no fp32 a can show: that mistake is
    the normals' to catch (it exchanges the angles of the two Box-Muller pairs); a missing round is caught by both."""
    for alpha in ALPHAS:
        got, U, V = a_case(alpha, 0, mut)
        if mut == 'swap_words':
            assert R.judge_a(got, alpha, U, V) < 2.0 ** -24
            continue
        with pytest.raises(AssertionError):
            R.judge_a(got, alpha, U, V)
    got, ref = z_case(0, 5, 2, mut)
    with pytest.raises(AssertionError):
        R.judge_z(got, ref)


def test_an_unshifted_step_is_refused():
    got, ref = z_case(0, 5, 2, 'step_unshifted')
    with pytest.raises(AssertionError):
        R.judge_z(got, ref)
    got, U, V = a_case(1.7, 0, 'step_unshifted', purpose=R.P_A_ELEM, elem=True)
    with pytest.raises(AssertionError):
        R.judge_a(got[1:], 1.7, U[1:], V[1:])          # rows t >= 1: at t = 0 there is nothing to shift


def test_a_dropped_high_word_is_refused_where_the_index_crosses_2_32():
    off = OFFSETS[1]
    assert off + 1 < 1 << 32 <= off + 2
    got, U, V = a_case(1.7, off, 'no_high_word')
    R.judge_a(got[:, :2], 1.7, U[:, :2], V[:, :2])     # below 2^32 the high word is zero either way
    with pytest.raises(AssertionError):
        R.judge_a(got[:, 2:], 1.7, U[:, 2:], V[:, 2:])
    got, ref = z_case(off, 5, 2, 'no_high_word')
    assert R.judge_z(got[:2], ref[:2]) < 1e-6
    with pytest.raises(AssertionError):
        R.judge_z(got[2:], ref[2:])


@pytest.mark.parametrize('mut', ['lane_reversed', 'sin_cos'])
@pytest.mark.parametrize('D', [2, 3, 4, 5, 8])
def test_wrong_lanes_are_refused(mut, D):
    got, ref = z_case(0, D, 2, mut)
    with pytest.raises(AssertionError):
        R.judge_z(got, ref)


@pytest.mark.parametrize('mut', ['th0', 'scale_exponent', 'w_from_u'])
@pytest.mark.parametrize('alpha', ALPHAS)
def test_a_wrong_cms_map_is_refused(mut, alpha):
    for off in OFFSETS:
        got, U, V = a_case(alpha, off, mut)
        with pytest.raises(AssertionError):
            R.judge_a(got, alpha, U, V)
