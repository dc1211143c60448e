"""Every Philox draw of the device, element by element, against the host mirror (tests/philox_ref.py).

Each entry point is given tables that make its output BE the draw (x = eps = 0, coefficient tables of ones, injected a of one),
so nothing has to be divided back out:
  * a draws against cms64 (NumPy float64), the chosen tail draws against cms_mp (60 digits): one fp32 ulp;
  * normals against the float64 Box-Muller of the device's own float32 uniforms: philox_ref.Z_BOUND;
  * integers, fp32 results of correctly rounded operations, values at a clamp, alpha = 2: bit for bit;
  * every kernel dlpm_update_f32 / dlpm_lim_update_f32 can route to gives the same z(seed, sample, element, t): bit for bit.
Seed with a non-zero high word; sample offsets 0, 2^32 - 2 (the batch straddles the low word of the counter) and the host-chosen
tail offsets.  Each test prints the maxima it measured."""
import ctypes as C

import numpy as np
import pytest
import torch

import philox_ref as R
from dlpm_amd import _lib
from oracle import process as P
from philox_ref import ALPHAS, OFFSETS, SEED

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T_SDE = 0.9946


def L():
    return _lib.lib()


def st():
    return _lib.stream_ptr()


def ones(*shape):
    return torch.ones(*shape, device=DEV)


def gidx(offset, B):
    return (np.int64(offset) + np.arange(B, dtype=np.int64)).astype(np.uint64)


def misaligned(n):
    """n floats on the device starting 4 bytes past a 16-byte boundary (the base stays alive through the view)."""
    v = torch.zeros(n + 4, device=DEV)[1:1 + n]
    assert v.data_ptr() % 16 == 4
    return v


def key_pair(offset):
    return torch.tensor([SEED, offset], dtype=torch.int64, device=DEV)       # the bits of {uint64 seed, int64 offset}


# ---------------------------------------------------------------- 1. the a draws of the sampler
def levy(T, B, alpha, clamp, offset, D=None):
    A = torch.full((T, B) if D is None else (T, B, D), float('nan'), device=DEV)
    if D is None:
        _lib.check(L().dlpm_skewed_levy_philox_f32(A.data_ptr(), T, B, alpha, clamp, SEED, offset, st()))
    else:
        _lib.check(L().dlpm_skewed_levy_elem_philox_f32(A.data_ptr(), T, B, D, alpha, clamp, SEED, offset, st()))
    return A.cpu().numpy()


def levy_uniforms(T, B, offset, D=None):
    g = gidx(offset, B)
    if D is None:
        return R.a_uniforms(SEED, g[None, :], np.arange(T)[:, None], R.P_A)
    return R.a_uniforms(SEED, g[None, :, None], np.arange(D)[None, None, :], R.P_A_ELEM, np.arange(T)[:, None, None])


@pytest.mark.parametrize('elem', [False, True], ids=['per_sample', 'per_element'])
@pytest.mark.parametrize('alpha', ALPHAS)
def test_sampler_a_draws_match_the_mirror_to_one_ulp(alpha, elem):
    T, B, D = 3, 4, (5 if elem else None)
    # the tail draw of a batch launched at a tail offset is A[0, 0] (row 0) or A[1, 0, 2] (row 1, element 2): what was scanned
    tails = R.tail_offsets(SEED, 2, R.P_A_ELEM, 1) if elem else R.tail_offsets(SEED, 0, R.P_A, 0)
    at = (1, 0, 2) if elem else (0, 0)
    for clamp in (-1.0, 10.0):
        bulk = tail = 0.0
        for off in OFFSETS + tails:
            got = levy(T, B, alpha, clamp, off, D)
            U, V = levy_uniforms(T, B, off, D)
            bulk = max(bulk, R.judge_a(got, alpha, U, V, clamp))
            if off in tails:
                tail = max(tail, R.judge_a(got[at], alpha, U[at], V[at], clamp, mp=True))
        print('a %s alpha %g clamp %g: max relative error %.3g against cms64, %.3g at the 32 tail draws against cms_mp'
              % ('per element' if elem else 'per sample', alpha, clamp, bulk, tail))


def test_alpha_two_gives_the_constant():
    for D in (None, 5):
        for clamp in (-1.0, 10.0):
            assert (levy(3, 4, 2.0, clamp, OFFSETS[1], D) == 2.0).all()


# ---------------------------------------------------------------- 2. x_T
def init_state(B, D, alpha, clamp_eps, offset, elem):
    x = torch.full((B, D), float('nan'), device=DEV)
    fn = L().dlpm_init_state_elem_philox_f32 if elem else L().dlpm_init_state_philox_f32
    _lib.check(fn(x.data_ptr(), B, D, alpha, clamp_eps, 1.0, SEED, offset, st()))
    return x.cpu().numpy()


def judge_scaled(got, a, z, clamp=-1.0):
    """got = clamp(fl(sqrt_f32(a) z)): the normal's own bound times sqrt(a), plus 2^-22 relative for the fp32 cast of a, the fp32
    root (1 ulp allowed) and the product; beyond the clamp by more than that, exactly the clamp.  Returns the largest error in
    units of sqrt(a)."""
    got = np.asarray(got, np.float64)
    sa = np.sqrt(a)
    ref = sa * z
    tol = sa * R.Z_BOUND + 2.0 ** -22 * np.abs(ref)
    want = np.clip(ref, -clamp, clamp) if clamp >= 0 else ref
    err = np.abs(got - want)
    assert np.all(np.isfinite(got)) and np.all(err <= tol), 'off by %.3g sqrt(a)' % (err / sa).max()
    if clamp >= 0:
        over = np.abs(ref) > clamp + tol
        assert np.array_equal(got[over], np.sign(ref[over]) * np.float64(np.float32(clamp)))
    return float((err / sa).max())


@pytest.mark.parametrize('elem', [False, True], ids=['per_sample', 'per_element'])
@pytest.mark.parametrize('D', [1, 3, 4, 5, 8])
def test_x_T_is_clamped_sqrt_a_times_z(D, elem):
    B = 3
    purpose = R.P_INIT_A_ELEM if elem else R.P_INIT_A
    tails = R.tail_offsets(SEED, 0, purpose, 0, 1 << 20, 2)              # of sample b = 0 (element 0)
    worst = 0.0
    for alpha in (1.2, 1.7, 1.99, 2.0):
        for clamp in (-1.0, 2.0):
            for off in OFFSETS + tails:
                g = gidx(off, B)
                z = R.normals(SEED, g, D, R.P_INIT_Z)
                if alpha == 2.0:
                    a = np.full((B, D), 2.0)
                elif elem:
                    a = R.cms64(alpha, *R.a_uniforms(SEED, g[:, None], np.arange(D)[None, :], purpose))
                else:
                    a = np.broadcast_to(R.cms64(alpha, *R.a_uniforms(SEED, g, 0, purpose))[:, None], (B, D))
                a = a.astype(np.float32).astype(np.float64)                # a0 is a float on the device
                worst = max(worst, judge_scaled(init_state(B, D, alpha, clamp, off, elem), a, z, clamp))
    print('x_T D=%d %s: max |x_T - sqrt(a) z| / sqrt(a) = %.3g' % (D, 'per element' if elem else 'per sample', worst))


# ---------------------------------------------------------------- 3. the step normals: every route of dlpm_update_f32
STEP_T, TABLE_T = 3, 5


def update(B, D, t=STEP_T, flags=0, eta=0.0, offset=0, key_dev=False, misalign=False, tabs=None, T=TABLE_T):
    """dlpm_update_f32 on x = eps = 0.  tabs None: every table is ones, so that the output is z(seed, sample, element, t) itself
    on every route (the DLIM step with eta = 1: sigma_t = bs = 1, mean coefficient (1 - 1)^(1/alpha) = 0).  Returns (x, t after)."""
    elem = bool(flags & _lib.UPD_ELEMENTWISE)
    n = B * D
    x = misaligned(n) if misalign else torch.zeros(n, device=DEV)
    eps = torch.zeros(n, device=DEV)
    td = torch.tensor([t], dtype=torch.int32, device=DEV)
    sched = ones(T)
    ce, cn, A = tabs if tabs is not None else (ones(T, n if elem else B),) * 3
    kd = key_pair(offset) if key_dev else None
    a = _lib.UpdateArgs()
    a.x_dev, a.eps_dev, a.t_dev = x.data_ptr(), eps.data_ptr(), td.data_ptr()
    a.g_dev = a.bg_dev = a.bs_dev = sched.data_ptr()
    a.c_eps_dev, a.c_noise_dev, a.A_dev = ce.data_ptr(), cn.data_ptr(), A.data_ptr()
    a.B, a.D, a.T, a.flags, a.dlim_eta, a.alpha = B, D, T, flags, eta, 1.7
    if key_dev:
        a.seed, a.sample_offset, a.key_dev = 0xDEAD, 77, kd.data_ptr()       # the fields a key on the device overrides
    else:
        a.seed, a.sample_offset = SEED, offset
    _lib.check(L().dlpm_update_f32(C.byref(a), st()))
    torch.cuda.synchronize()
    return x.cpu().numpy().reshape(B, D), int(td.item())


CANON_B, CANON_D = 3, 4 * 769
_canon = {}


def canon(offset, t=STEP_T):
    """z(SEED, offset + b, e, t) for b < 3, e < 3076 as k_update_rows draws it (two trips of its three-quad loop): what every
    other route has to reproduce bit for bit.  test_rows_route_matches_the_mirror judges it against the host."""
    if (offset, t) not in _canon:
        _canon[(offset, t)] = update(CANON_B, CANON_D, t, offset=offset)[0]
    return _canon[(offset, t)]


@pytest.mark.parametrize('offset', OFFSETS)
def test_rows_route_matches_the_mirror(offset):
    ref = R.normals(SEED, gidx(offset, CANON_B), CANON_D, R.P_STEP_Z, STEP_T)
    err = R.judge_z(canon(offset), ref)
    print('step normals, k_update_rows B=3 D=3076 offset %d: max |z - mirror| = %.3g' % (offset, err))
    # another step is another draw; D = 4 (one quad) and D = 4 * 257 (the second slot live for thread 0 only) are the same function
    assert not np.array_equal(canon(offset, 2)[:, :64], canon(offset)[:, :64])
    R.judge_z(canon(offset, 2), R.normals(SEED, gidx(offset, CANON_B), CANON_D, R.P_STEP_Z, 2))
    for D in (4, 4 * 257):
        assert np.array_equal(update(3, D, offset=offset)[0], canon(offset)[:, :D])


ROUTES = {
    # name: (D, flags, eta, misalign) at B = 3
    'vec_clip_15_quads': (20, _lib.UPD_CLIP, 0.0, False),
    'vec_clip_1200_quads': (1600, _lib.UPD_CLIP, 0.0, False),            # two blocks, a partly filled third slot
    'vec_dlim_15_quads': (20, _lib.UPD_DLIM, 1.0, False),
    'vec_dlim_1200_quads': (1600, _lib.UPD_DLIM, 1.0, False),
    'scalar_D2': (2, 0, 0.0, False),
    'scalar_D3': (3, 0, 0.0, False),
    'scalar_D5': (5, 0, 0.0, False),
    'scalar_D8_misaligned': (8, 0, 0.0, True),
    'scalar_D5_clip': (5, _lib.UPD_CLIP, 0.0, False),
    'scalar_D5_dlim': (5, _lib.UPD_DLIM, 1.0, False),
    'elem_vec_D8': (8, _lib.UPD_ELEMENTWISE, 0.0, False),
    'elem_vec_D1600': (1600, _lib.UPD_ELEMENTWISE, 0.0, False),
    'elem_scalar_D5': (5, _lib.UPD_ELEMENTWISE, 0.0, False),
    'elem_scalar_D8_misaligned': (8, _lib.UPD_ELEMENTWISE, 0.0, True),
    'elem_vec_dlim_D8': (8, _lib.UPD_ELEMENTWISE | _lib.UPD_DLIM, 1.0, False),
    'rows_D8': (8, 0, 0.0, False),
}


@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('route', ROUTES)
def test_every_update_route_draws_the_same_normals(route, offset):
    """Bit for bit against k_update_rows' draw (itself judged against the mirror), with the key in the arguments and on the device;
    UPD_ADVANCE moves t_dev after the draw and changes nothing else."""
    D, flags, eta, mis = ROUTES[route]
    want = canon(offset)[:, :D]
    got, t_after = update(3, D, flags=flags, eta=eta, offset=offset, misalign=mis)
    assert t_after == STEP_T and np.array_equal(got, want)
    got, t_after = update(3, D, flags=flags | _lib.UPD_ADVANCE, eta=eta, offset=offset, misalign=mis, key_dev=True)
    assert t_after == STEP_T - 1 and np.array_equal(got, want)


def test_vector_route_grid_stride_second_trip():
    """B D / 4 = 2049 * 1024 quads: 1024 past the 2 Mi that 2048 blocks x 256 threads x 4 slots cover in one trip, so thread i < 1024
    comes round again.  The one large case (two 34 MB tensors); the batch starts at 2^32 - 2, so 2047 samples have a high word."""
    B, D, off = 2049, 4096, OFFSETS[1]
    got, _ = update(B, D, flags=_lib.UPD_CLIP, offset=off)
    assert np.array_equal(got[:CANON_B, :CANON_D], canon(off))
    err = R.judge_z(got, R.normals(SEED, gidx(off, B), D, R.P_STEP_Z, STEP_T))
    print('step normals, k_update<vec> B=2049 D=4096 (8.4 M normals): max |z - mirror| = %.3g' % err)


@pytest.mark.parametrize('route', ROUTES)
def test_t_equal_one_draws_no_noise(route):
    """With the tables dlpm_coeff_tables_f32 makes (c_noise[1] = 0; the DLIM and per-element kernels test t themselves) the state
    stays 0 at t = 1, while at t = 2 the same call gives fl(c_noise z)."""
    D, flags, eta, mis = ROUTES[route]
    B, T, alpha = 3, TABLE_T, 1.7
    elem = bool(flags & _lib.UPD_ELEMENTWISE)
    n = B * D if elem else B
    g, bg, s, bs = (v.to(DEV) for v in P.schedule(T, alpha))
    A = ones(T, n)
    ce, cn = torch.empty_like(A), torch.empty_like(A)
    _lib.check(L().dlpm_coeff_tables_f32(A.data_ptr(), g.data_ptr(), s.data_ptr(), bs.data_ptr(), T, n, ce.data_ptr(), cn.data_ptr(), None, st()))
    assert (cn[1] == 0).all() and (cn[2] > 0).all()
    got, _ = update(B, D, t=1, flags=flags, eta=eta, misalign=mis, tabs=(ce, cn, A))
    assert (got == 0).all()
    got, _ = update(B, D, t=2, flags=flags, eta=eta, misalign=mis, tabs=(ce, cn, A))
    c2 = np.float32(1.0) if flags & _lib.UPD_DLIM else cn[2].cpu().numpy().reshape(B, -1)    # DLIM: eta bs[t-1] sqrt(A), bs = A = 1 here
    assert np.array_equal(got, c2 * canon(0, 2)[:, :D])


def test_update_refuses_a_timestep_count_beyond_24_bits():
    """purpose | t << 8 would wrap: refused before any launch, state and t_dev untouched."""
    for T in (1 << 24, (1 << 24) + 5):
        x, eps = torch.full((8,), 7.0, device=DEV), torch.zeros(8, device=DEV)
        td = torch.tensor([1], dtype=torch.int32, device=DEV)
        tab = ones(4)
        a = _lib.UpdateArgs()
        a.x_dev, a.eps_dev, a.t_dev = x.data_ptr(), eps.data_ptr(), td.data_ptr()
        a.g_dev = a.bg_dev = a.bs_dev = a.c_eps_dev = a.c_noise_dev = a.A_dev = tab.data_ptr()
        a.B, a.D, a.T, a.flags, a.seed = 1, 8, T, _lib.UPD_ADVANCE, SEED
        with pytest.raises(ValueError, match='24 bits'):
            _lib.check(L().dlpm_update_f32(C.byref(a), st()))
        torch.cuda.synchronize()
        assert (x == 7.0).all() and int(td.item()) == 1
        b = _lib.LimUpdateArgs()
        td = torch.tensor([T - 1], dtype=torch.int32, device=DEV)            # step index (T - 1) - t = 0
        b.x_dev, b.eps_dev, b.t_dev = x.data_ptr(), eps.data_ptr(), td.data_ptr()
        b.tmp_dev = b.cx_dev = b.cs_dev = b.cn_dev = tab.data_ptr()
        b.B, b.D, b.T, b.flags, b.clamp_eps, b.seed = 1, 8, T, _lib.UPD_ADVANCE, -1.0, SEED
        with pytest.raises(ValueError, match='24 bits'):
            _lib.check(L().dlpm_lim_update_f32(C.byref(b), st()))
        torch.cuda.synchronize()
        assert (x == 7.0).all() and int(td.item()) == T - 1


# ---------------------------------------------------------------- 4. the LIM update
def lim_update(B, D, t, T=TABLE_T, with_A=False, clamp=-1.0, ode=False, offset=0, key_dev=False, misalign=False, advance=False):
    """dlpm_lim_update_f32 on x = eps = 0.  The noise coefficient is 1 at the step's own table index (T - 1) - t and 2 everywhere
    else, A (when given) 4 there and 9 elsewhere: the output is z, or clamp(2 z), exactly when the tables are read at
    (T - 1) - t while the counter carries t."""
    n, i = B * D, (T - 1) - t
    x = misaligned(n) if misalign else torch.zeros(n, device=DEV)
    eps = torch.zeros(n, device=DEV)
    td = torch.tensor([t], dtype=torch.int32, device=DEV)
    one, cn, A = ones(T - 1), 2.0 * ones(T - 1), 9.0 * ones(T - 1, B)
    cn[i], A[i] = 1.0, 4.0
    kd = key_pair(offset) if key_dev else None
    a = _lib.LimUpdateArgs()
    a.x_dev, a.eps_dev, a.t_dev = x.data_ptr(), eps.data_ptr(), td.data_ptr()
    a.tmp_dev = a.cx_dev = a.cs_dev = one.data_ptr()
    a.cn_dev, a.A_dev = cn.data_ptr(), A.data_ptr() if with_A else None
    a.B, a.D, a.T, a.clamp_eps = B, D, T, clamp
    a.flags = (_lib.UPD_DLIM if ode else 0) | (_lib.UPD_ADVANCE if advance else 0)
    if key_dev:
        a.seed, a.sample_offset, a.key_dev = 0xDEAD, 77, kd.data_ptr()
    else:
        a.seed, a.sample_offset = SEED, offset
    _lib.check(L().dlpm_lim_update_f32(C.byref(a), st()))
    torch.cuda.synchronize()
    return x.cpu().numpy().reshape(B, D), int(td.item())


LIM_ROUTES = {
    # name: (D, misalign): both widths, and both block sizes (fewer than 256 work items per row: 64 threads, else 256)
    'vec_64_threads': (8, False),
    'vec_256_threads': (4 * 257, False),
    'scalar_64_threads': (5, False),
    'scalar_256_threads': (257, False),
    'scalar_D8_misaligned': (8, True),
}


@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('route', LIM_ROUTES)
def test_lim_update_draws_the_step_normals(route, offset):
    """The LIM update keys its normals as the DLPM update does -- (sample, quad, purpose 4 | t << 8) -- while its tables run the
    other way (index (T - 1) - t): bit for bit k_update_rows' draw at every t, scaled by sqrt(a) and clamped when A is given;
    the ODE flag draws nothing."""
    D, mis = LIM_ROUTES[route]
    for t in (1, 2, STEP_T, TABLE_T - 1):
        want = canon(offset, t)[:, :D]
        got, t_after = lim_update(3, D, t, offset=offset, misalign=mis)
        assert t_after == t and np.array_equal(got, want), t
    got, t_after = lim_update(3, D, STEP_T, offset=offset, misalign=mis, key_dev=True, advance=True)
    z = canon(offset)[:, :D]
    assert t_after == STEP_T - 1 and np.array_equal(got, z)
    assert np.array_equal(lim_update(3, D, STEP_T, with_A=True, offset=offset, misalign=mis)[0], np.float32(2.0) * z)
    got = lim_update(3, D, STEP_T, with_A=True, clamp=1.0, offset=offset, misalign=mis)[0]
    assert np.array_equal(got, np.clip(np.float32(2.0) * z, -1.0, 1.0))
    assert np.array_equal(lim_update(3, D, STEP_T, clamp=1.0, offset=offset, misalign=mis)[0], z)     # no A: no clamp (the Gaussian case)
    assert (lim_update(3, D, STEP_T, with_A=True, ode=True, offset=offset, misalign=mis)[0] == 0).all()


# ---------------------------------------------------------------- 5. the held-out DLPM loss
def loss_elements(B, D, T, alpha, offset=0, outer=1, inner=1, clamp_a=-1.0, elem=False, a_one=False):
    """dlpm_loss_elements_f32 with x0 = 0 and bg = bs = 1: x_t = fl(sqrt(a) z).  a_one injects a = 1, so that x_t is z itself.
    Returns (t[B], a[outer, B(, D)], x_t[outer * inner, B, D])."""
    Rr = outer * inner
    x0, tab = torch.zeros(B, D, device=DEV), ones(T)
    x_in, eps, x_t = (torch.full((Rr * B, D), float('nan'), device=DEV) for _ in range(3))
    t = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    shape = (outer, B, D) if elem else (outer, B)
    a_in, a_out = ones(*shape), torch.full(shape, float('nan'), device=DEV)
    a = _lib.LossArgs()
    a.x0_dev, a.bg_dev, a.bs_dev, a.a_dev = x0.data_ptr(), tab.data_ptr(), tab.data_ptr(), a_in.data_ptr() if a_one else None
    a.x_in_dev, a.eps_dev, a.x_t_dev, a.t_out_dev, a.a_out_dev = x_in.data_ptr(), eps.data_ptr(), x_t.data_ptr(), t.data_ptr(), a_out.data_ptr()
    a.B, a.D, a.T, a.outer, a.inner, a.flags = B, D, T, outer, inner, _lib.LOSS_ELEMENTWISE if elem else 0
    a.alpha, a.clamp_a, a.seed, a.sample_offset = alpha, clamp_a, SEED, offset
    _lib.check(L().dlpm_loss_elements_f32(C.byref(a), st()))
    torch.cuda.synchronize()
    assert torch.equal(x_in, x_t) and torch.equal(eps, x_t)                 # no input scaling; (x_t - 0) / 1
    return t.cpu().numpy(), a_out.cpu().numpy(), x_t.cpu().numpy().reshape(Rr, B, D)


@pytest.mark.parametrize('T', [2, 100, 1000])
def test_loss_timesteps_are_exact(T):
    B = 64
    for off in OFFSETS:
        t, _, _ = loss_elements(B, 4, T, 1.7, offset=off)
        x = R.words(SEED, gidx(off, B), 0, R.P_LOSS_T)[0]
        want = 1 + ((x * np.uint64(T - 1)) >> np.uint64(32)).astype(np.int64)
        assert np.array_equal(t, want) and want.min() >= 1 and want.max() <= T - 1
    assert T == 2 or len(np.unique(t)) > 1


@pytest.mark.parametrize('elem', [False, True], ids=['per_sample', 'per_element'])
@pytest.mark.parametrize('alpha', ALPHAS)
def test_loss_a_draws_match_the_mirror_to_one_ulp(alpha, elem):
    """a per (sample, r mod outer), or per (sample, element, r mod outer): cms.h's evaluation, tails included."""
    B, outer, inner = 4, 3, 2
    tails = R.tail_offsets(SEED, 0, R.P_LOSS_A, 0)                          # of a[0, 0]: replica 0 of sample b = 0
    for D in (3, 8):
        for clamp in (-1.0, 10.0):
            bulk = tail = 0.0
            for off in OFFSETS + (() if elem else tails):
                _, got, _ = loss_elements(B, D, 50, alpha, off, outer, inner, clamp, elem)
                g = gidx(off, B)
                if elem:
                    U, V = R.a_uniforms(SEED, g[None, :, None], np.arange(D)[None, None, :], R.P_LOSS_A_ELEM, np.arange(outer)[:, None, None])
                else:
                    U, V = R.a_uniforms(SEED, g[None, :], 0, R.P_LOSS_A, np.arange(outer)[:, None])
                bulk = max(bulk, R.judge_a(got, alpha, U, V, clamp))
                if off in tails:
                    tail = max(tail, R.judge_a(got[0, 0], alpha, U[0, 0], V[0, 0], clamp, mp=True))
            print('loss a %s alpha %g D %d clamp %g: max relative error %.3g against cms64, %.3g at the tail draws against cms_mp'
                  % ('per element' if elem else 'per sample', alpha, D, clamp, bulk, tail))
    assert (loss_elements(B, 3, 50, 2.0, OFFSETS[1], outer, inner, 10.0, elem)[1] == 2.0).all()


@pytest.mark.parametrize('elem', [False, True], ids=['per_sample', 'per_element'])
def test_loss_normals_are_keyed_by_sample_and_replica(elem):
    B, outer, inner = 4, 3, 2
    for off in OFFSETS:
        _, _, z8 = loss_elements(B, 8, 50, 1.7, off, outer, inner, elem=elem, a_one=True)
        _, _, z3 = loss_elements(B, 3, 50, 1.7, off, outer, inner, elem=elem, a_one=True)
        assert np.array_equal(z3, z8[:, :, :3])                               # the scalar route: lane e & 3 of quad e >> 2
        ref = np.stack([R.normals(SEED, gidx(off, B), 8, R.P_LOSS_Z, r) for r in range(outer * inner)])
        err = R.judge_z(z8, ref)
        print('loss normals offset %d: max |z - mirror| = %.3g' % (off, err))
        # with a drawn, x_t = fl(sqrt(a) z) with the a of replica r mod outer
        _, a, xt = loss_elements(B, 8, 50, 1.7, off, outer, inner, elem=elem)
        a = a.astype(np.float64).reshape(outer, B, -1)
        judge_scaled(xt, np.broadcast_to(np.concatenate([a] * inner), xt.shape), ref)


# ---------------------------------------------------------------- 6. the held-out LIM loss
def lim_loss_elements(B, D, alpha, offset=0, clamp_eps=-1.0):
    x0 = torch.zeros(B, D, device=DEV)
    out = {k: torch.full((B, D), float('nan'), device=DEV) for k in ('x_t', 'score', 'e')}
    out.update({k: torch.full((B,), float('nan'), device=DEV) for k in ('t', 'a')})
    a = _lib.LimLossArgs()
    a.x0_dev, a.x_t_dev, a.score_dev, a.tvec_out_dev = x0.data_ptr(), out['x_t'].data_ptr(), out['score'].data_ptr(), out['t'].data_ptr()
    a.a_out_dev, a.e_out_dev = out['a'].data_ptr(), out['e'].data_ptr()
    a.B, a.D, a.alpha, a.clamp_eps, a.t_max, a.seed, a.sample_offset = B, D, alpha, clamp_eps, T_SDE, SEED, offset
    _lib.check(L().dlpm_lim_loss_elements_f32(C.byref(a), st()))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('offset', OFFSETS)
def test_lim_loss_draws(offset):
    B = 64
    g = gidx(offset, B)
    f32 = np.float32
    u24 = (R.words(SEED, g, 0, R.P_LIM_T)[0] >> np.uint64(8)).astype(f32) * f32(2.0 ** -24)
    t_want = u24 * f32(T_SDE - 1e-5) + f32(1e-5)                               # float32 arrays: one rounded product, one rounded sum
    assert t_want.dtype == np.float32
    z3 = None
    for D in (8, 3):
        r = lim_loss_elements(B, D, 2.0, offset)                               # alpha = 2: e is z, a is not drawn
        assert np.array_equal(r['t'], t_want) and (r['a'] == 1.0).all()
        ref = R.normals(SEED, g, D, R.P_LIM_Z)
        err = R.judge_z(r['e'], ref)
        print('LIM-loss normals D=%d offset %d: max |z - mirror| = %.3g' % (D, offset, err))
        z3 = r['e'] if D == 8 else z3
        assert D == 8 or np.array_equal(r['e'], z3[:, :3])
        for alpha in ALPHAS:
            for clamp in (-1.0, 2.0):
                r = lim_loss_elements(B, D, alpha, offset, clamp)
                assert np.array_equal(r['t'], t_want)
                U, V = R.a_uniforms(SEED, g, 0, R.P_LIM_A)
                R.judge_a(r['a'], alpha, U, V)                                  # gen_sas: a itself is never clamped
                judge_scaled(r['e'], np.broadcast_to(r['a'].astype(np.float64)[:, None], (B, D)), ref, clamp)


# ---------------------------------------------------------------- 7. the two-rv elements
def two_rv(B, D, t, alpha, offset=0, clamp_a=-1.0, elem=False, inject=False, T=TABLE_T):
    """dlpm_two_rv_elements_f32 with x0 = 0 and a schedule of ones.  inject: a0 = 0 and a1 = 1, so Sigma'_t = 1 and x_t is z itself."""
    x0, tab = torch.zeros(B, D, device=DEV), ones(T)
    td = torch.tensor(t, dtype=torch.int32, device=DEV)
    shape = (B, D) if elem else (B,)
    x_t, a0o, a1o = (torch.full(s, float('nan'), device=DEV) for s in ((B, D), shape, shape))
    a0, a1 = torch.zeros(shape, device=DEV), ones(*shape)
    a = _lib.TwoRvArgs()
    a.x0_dev, a.t_dev = x0.data_ptr(), td.data_ptr()
    a.g_dev = a.bg_dev = a.s_dev = a.bs_dev = tab.data_ptr()
    if inject:
        a.a0_dev, a.a1_dev = a0.data_ptr(), a1.data_ptr()
    a.x_t_dev, a.a0_out_dev, a.a1_out_dev = x_t.data_ptr(), a0o.data_ptr(), a1o.data_ptr()
    a.B, a.D, a.T, a.flags = B, D, T, _lib.LOSS_ELEMENTWISE if elem else 0
    a.alpha, a.clamp_a, a.seed, a.sample_offset = alpha, clamp_a, SEED, offset
    _lib.check(L().dlpm_two_rv_elements_f32(C.byref(a), st()))
    torch.cuda.synchronize()
    return x_t.cpu().numpy(), a0o.cpu().numpy(), a1o.cpu().numpy()


@pytest.mark.parametrize('elem', [False, True], ids=['per_sample', 'per_element'])
@pytest.mark.parametrize('offset', OFFSETS)
def test_two_rv_draws(offset, elem):
    B, t = 4, [1, 2, 4, 1]
    one = np.array(t) == 1
    g = gidx(offset, B)
    for D in (8, 3):
        ref = R.normals(SEED, g, D, R.P_TWO_RV_Z)
        z, a0, a1 = two_rv(B, D, t, 1.7, offset, elem=elem, inject=True)
        err = R.judge_z(z, ref)
        print('two-rv normals D=%d offset %d: max |z - mirror| = %.3g' % (D, offset, err))
        assert (a0 == 0).all() and (a1 == 1).all()
        for alpha in ALPHAS:
            for clamp in (-1.0, 10.0):
                x_t, a0, a1 = two_rv(B, D, t, alpha, offset, clamp, elem)
                if elem:
                    uv = [R.a_uniforms(SEED, g[:, None], np.arange(D)[None, :], R.P_TWO_RV_A_ELEM, which) for which in (0, 1)]
                else:
                    uv = [R.a_uniforms(SEED, g, 0, R.P_TWO_RV_A, which) for which in (0, 1)]
                assert (a0[one] == 0).all()                                      # zeroed where t == 1
                R.judge_a(a0[~one], alpha, uv[0][0][~one], uv[0][1][~one], clamp)
                R.judge_a(a1, alpha, uv[1][0], uv[1][1], clamp)
                # Sigma'_t = fl(fl(1 a1) + fl(1 fl(1 a0))) with the schedule of ones
                sig = (a1 + a0).astype(np.float64).reshape(B, -1)
                judge_scaled(x_t, np.broadcast_to(sig, (B, D)), ref)
        x_t, a0, a1 = two_rv(B, D, t, 2.0, offset, 10.0, elem)
        assert (a0[~one] == 2.0).all() and (a0[one] == 0).all() and (a1 == 2.0).all()
