"""Host mirror of every Philox-keyed draw the device makes: NumPy, mpmath and SciPy only.

Every random number of the device is documented as a pure function of (seed, global sample, row / element, purpose, step)
through Philox4x32-10.  This module restates that function from the headers' words and the counter layout of DESIGN 3.18, so
that the device can be judged element by element:

    counter = (gidx lo, gidx hi, word2, purpose | word3 << 8),  key = the 64-bit seed (low word first)

    a draws   U, V = two 53-bit uniforms from the word pairs (x, y) and (z, w); a = cms(alpha, U, V)
    normals   four 24-bit uniforms, two Box-Muller pairs; element e of a sample takes lane e & 3 of quad e >> 2

Options named `mut` exist for tests/test_philox_ref_cpu.py alone: each applies one deliberate mistake to a copy of the mirror,
which the judges below have to refuse."""
import functools

import mpmath
import numpy as np

MASK = np.uint64(0xFFFFFFFF)
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)

# purposes (the counter layout table of DESIGN 3.18)
P_A, P_INIT_A, P_INIT_Z, P_STEP_Z, P_A_ELEM, P_INIT_A_ELEM = 1, 2, 3, 4, 5, 6
P_LOSS_T, P_LOSS_A, P_LOSS_A_ELEM, P_LOSS_Z = 7, 8, 9, 10
P_LIM_T, P_LIM_A, P_LIM_Z = 11, 12, 13
P_TWO_RV_A, P_TWO_RV_A_ELEM, P_TWO_RV_Z = 18, 19, 20

# what tests/test_gpu_draws.py launches with, and tests/test_philox_ref_cpu.py turns the mutations loose on
SEED = 0x0123456789ABCDEF                # a non-zero high word
OFFSETS = (0, (1 << 32) - 2)             # a batch of 3 or 4 at the second straddles the boundary of the counter's low word
ALPHAS = (1.2, 1.5, 1.7, 1.8, 1.9, 1.99)

# The hardware v_log_f32 / v_sin_f32 / v_cos_f32 / v_sqrt_f32 carry no stated accuracy, so the bound on a normal is measured:
# the largest |z_dev - z_ref| over every case of tests/test_gpu_draws.py against the float64 mirror was Z_MEASURED (2026-10-19,
# MI355X); the tests hold 4 x that, the margin for other counters reaching other arguments of those approximations, and never more
# than Z_CAP: a normal further off would spend the project's 1e-4 pixel contract by itself (a counter mistake moves z by O(1)).
Z_MEASURED = 7.95e-7
Z_MARGIN = 4.0
Z_CAP = 1e-4
Z_BOUND = min(Z_MARGIN * Z_MEASURED, Z_CAP)

A_ULP = 2.0 ** -23           # |got - cms_mp| <= one fp32 ulp: 2^-24 for the cast, 1e-8 for the fp64 evaluation, the rest for the device's libm
A_ULP_199 = 2.0 ** -22       # alpha = 1.99: cos(pi alpha / 4) is 8e-3, the map is that much worse conditioned
COND, COND_199 = 1e-8, 1e-7  # the condition cms64 keeps against cms_mp (test_philox_ref_cpu.py), added where cms64 is the reference


def philox4x32_10(c0, c1, c2, c3, key, rounds=10):
    """Philox4x32 (Salmon et al., SC'11), vectorised: four uint64 arrays holding 32-bit counter words, a 64-bit key whose low
    word is key word 0.  Returns the four output words as uint64 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & MASK for c in (c0, c1, c2, c3)))
    key = int(key)
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64(key >> 32)
    for _ in range(rounds):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def words(seed, gidx, word2, purpose, word3=0, mut=None):
    """The four Philox words of one draw: counter (gidx lo, gidx hi, word2, purpose | word3 << 8), key seed."""
    gidx = np.asarray(gidx).astype(np.uint64)            # an int64 sample_offset + b, taken as the device takes it
    hi = gidx >> np.uint64(32)
    if mut == 'no_high_word':
        hi = hi * np.uint64(0)
    w3 = np.asarray(word3, dtype=np.uint64)
    last = np.uint64(purpose) | (w3 if mut == 'step_unshifted' else (w3 << np.uint64(8)))
    out = philox4x32_10(gidx, hi, word2, last, seed, rounds=9 if mut == 'nine_rounds' else 10)
    if mut == 'swap_words':
        out = (out[0], out[3], out[2], out[1])           # words 1 and 3 exchanged
    return out


def uniforms53(w):
    """U from words (x, y) and V from (z, w): ((hi << 21) ^ (lo >> 11) + 0.5) / 2^53 in float64, the device's three operations.
    Never 0.  From 2^52 on the sum needs 54 bits and rounds to even, so the single largest 53-bit value gives exactly 1.0 (one
    draw in 2^53; DESIGN 3.18 says what the map makes of it)."""
    s = 2.0 ** -53
    u = (((w[0] << np.uint64(21)) ^ (w[1] >> np.uint64(11))).astype(np.float64) + 0.5) * s
    v = (((w[2] << np.uint64(21)) ^ (w[3] >> np.uint64(11))).astype(np.float64) + 0.5) * s
    return u, v


def uniforms24(w):
    """The four 24-bit uniforms of the normals, ((float)(w >> 8) + 0.5f) * 2^-24 computed in np.float32 as the device computes
    them.  For w >> 8 >= 2^23 the sum needs 25 bits and `+ 0.5f` ROUNDS (to even): the uniforms there are not the midpoints, and
    the largest, w >> 8 = 2^24 - 1, becomes u = 1.0 exactly, so r = sqrt(-2 ln 1) = 0 and both normals of the pair are +-0.  The
    mirror reproduces that; it is part of the documented function, one draw in 2^24."""
    return tuple(((x >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24) for x in w)


def normal4(seed, gidx, quad, purpose, step=0, mut=None):
    """The four N(0,1) of one quad, float64[..., 4]: Box-Muller in float64 on the float32 uniforms.  r = sqrt(-2 ln u0) gives
    (r cos 2 pi u1, r sin 2 pi u1) as lanes 0 and 1; the pair (u2, u3) gives lanes 2 and 3."""
    u = [x.astype(np.float64) for x in uniforms24(words(seed, gidx, quad, purpose, step, mut=mut))]
    out = []
    for a, b in ((u[0], u[1]), (u[2], u[3])):
        r, ang = np.sqrt(-2.0 * np.log(a)), 2.0 * np.pi * b
        out += [r * np.sin(ang), r * np.cos(ang)] if mut == 'sin_cos' else [r * np.cos(ang), r * np.sin(ang)]
    return np.stack(out, axis=-1)


def normals(seed, gidx, D, purpose, step=0, mut=None):
    """z[len(gidx), D]: element e of sample gidx[i] is lane e & 3 of quad e >> 2, on every route."""
    gidx = np.asarray(gidx).reshape(-1, 1)
    nq = (D + 3) // 4
    z4 = normal4(seed, gidx, np.arange(nq, dtype=np.uint64).reshape(1, -1), purpose, step, mut=mut)     # [n, nq, 4]
    if mut == 'lane_reversed':
        z4 = z4[..., ::-1]
    return z4.reshape(gidx.shape[0], nq * 4)[:, :D]


def cms_scale(alpha, mut=None):
    return 2.0 * np.cos(np.pi * alpha / 4.0) ** ((1.0 if mut == 'scale_exponent' else 2.0) / alpha)


def cms64(alpha, U, V, mut=None):
    """Chambers-Mallows-Stuck in NumPy float64: the S1 map with beta = 1, stability a = alpha / 2, angle th = pi (U - 1/2),
    W = -ln V standard exponential, times the scale 2 cos(pi alpha / 4)^(2 / alpha).  For bulk use; cms_mp is the reference."""
    U, V = np.asarray(U, np.float64), np.asarray(V, np.float64)
    a = alpha / 2.0
    zeta = np.tan(np.pi * a / 2.0)
    th0 = np.arctan(zeta) / a * (1.0 + 1e-6 if mut == 'th0' else 1.0)
    W = -np.log(U if mut == 'w_from_u' else V)
    th = np.pi * U - np.pi / 2.0
    lead = W / (np.cos(th) / np.tan(a * (th0 + th)) + np.sin(th))
    core = (np.cos(a * th) + np.sin(a * th) * np.tan(th) - zeta * (np.sin(a * th) - np.cos(a * th) * np.tan(th))) / W
    return lead * core ** (1.0 / a) * cms_scale(alpha, mut)


def cms_mp(alpha, U, V):
    """The same map at 60 digits on the double inputs, in the closed form it takes for beta = 1 (th0 = pi / 2, so
    a (th0 + th) = a pi U and cos th = sin pi U):
        sin(a pi U) / (cos(a pi / 2) sin(pi U))^(1/a) * (sin((1 - a) pi U) / W)^((1 - a) / a) * scale
    -- another arrangement than cms64's, so the two share no cancellation.  Returns mpmath numbers."""
    out = []
    with mpmath.workdps(60):
        a = mpmath.mpf(alpha) / 2
        scale = 2 * mpmath.cos(mpmath.pi * mpmath.mpf(alpha) / 4) ** (2 / mpmath.mpf(alpha))
        for u, v in zip(np.ravel(U), np.ravel(V)):
            u, W = mpmath.mpf(float(u)), -mpmath.log(mpmath.mpf(float(v)))
            x = mpmath.sin(a * mpmath.pi * u) / (mpmath.cos(a * mpmath.pi / 2) * mpmath.sin(mpmath.pi * u)) ** (1 / a)
            out.append(x * (mpmath.sin((1 - a) * mpmath.pi * u) / W) ** ((1 - a) / a) * scale)
    return out


def rel_err_vs_mp(x, ref):
    """max |x - ref| / |ref| of float64 values against mpmath references, evaluated at 60 digits."""
    with mpmath.workdps(60):
        return float(max(abs((mpmath.mpf(float(v)) - r) / r) for v, r in zip(np.ravel(x), ref)))


def a_uniforms(seed, gidx, word2, purpose, word3=0, mut=None):
    return uniforms53(words(seed, gidx, word2, purpose, word3, mut=mut))


@functools.lru_cache(maxsize=None)
def tail_offsets(seed, word2, purpose, word3, n=1 << 22, k=8):
    """Scans the sample indices [0, n) on the host and returns the k with the smallest U, the k with the largest U, the k with
    the smallest V and the k with the largest V (a tuple of 4 k ints): where the tests launch, so the tails are chosen, not hoped for."""
    us, vs = [], []
    for lo in range(0, n, 1 << 20):
        u, v = a_uniforms(seed, np.arange(lo, min(n, lo + (1 << 20)), dtype=np.uint64), word2, purpose, word3)
        us.append(u)
        vs.append(v)
    u, v = np.concatenate(us), np.concatenate(vs)
    pick = [np.argsort(u)[:k], np.argsort(u)[-k:], np.argsort(v)[:k], np.argsort(v)[-k:]]
    return tuple(int(i) for i in np.concatenate(pick))


def judge_a(got, alpha, U, V, clamp=-1.0, mp=False, mut=None):
    """A device a (float32) against the mirror of its uniforms: |got - ref| <= 2^-23 |ref| against cms_mp (2^-22 at alpha = 1.99);
    against cms64 its condition (1e-8, 1e-7 at 1.99) is added.  A clamped draw is min(max(ref, 0), clamp) under the same bound,
    and exactly the clamp wherever the reference exceeds it by more than the bound.  Raises AssertionError; returns the largest
    relative error measured."""
    got = np.asarray(got, np.float64).ravel()
    wide = alpha >= 1.99
    bound = (A_ULP_199 if wide else A_ULP) + (0.0 if mp else (COND_199 if wide else COND))
    if mp:
        assert mut is None
        ref = cms_mp(alpha, U, V)
        unclamped = np.array([float(r) for r in ref])
        if clamp >= 0:
            ref = [min(max(r, mpmath.mpf(0)), mpmath.mpf(clamp)) for r in ref]
        raw = np.array([float(r) for r in ref])
        err = np.array([rel_err_vs_mp([g], [r]) for g, r in zip(got, ref)])
    else:
        unclamped = cms64(alpha, U, V, mut=mut).ravel()
        raw = np.minimum(np.maximum(unclamped, 0.0), clamp) if clamp >= 0 else unclamped
        err = np.abs(got - raw) / np.abs(raw)
    assert got.shape == raw.shape
    assert np.all(np.isfinite(got)) and np.all(err <= bound), 'a draw off by %.3g relative (bound %.3g) at alpha %g' % (err.max(), bound, alpha)
    if clamp >= 0:
        over = unclamped > clamp * (1 + bound)
        assert np.array_equal(got[over], np.full(over.sum(), np.float64(np.float32(clamp))))
    return float(err.max())


def judge_z(got, ref, scale=1.0):
    """Device normals against the float64 mirror: max |got - scale ref| <= scale Z_BOUND.  Returns the maximum (in units of scale)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = float(np.abs(got - scale * ref).max()) / scale
    assert np.all(np.isfinite(got)) and err <= Z_BOUND, 'a normal off by %.3g (bound %.3g)' % (err, Z_BOUND)
    return err
