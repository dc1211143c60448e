"""The toy net's lane kernels on the MI355X (dlpm_amd/csrc/mlp.hip) against the mirrors of tests/mlp_lane_refs.py.

k_mlp_forward: every architecture of ARCHS x ROWS against the float64 mirror with torch's fp32 forward as the yardstick, into a
NaN-filled buffer whose tail has to stay NaN; a row depends on nothing but itself, bit for bit.

k_mlp_sample and k_mlp_tp_table through dlpm_mlp_sample_steps_f32 called directly: its draws are a route of the step normals (bit
for bit dlpm_update_f32's, and the host mirror's within philox_ref.Z_BOUND); steps accumulate in order; ONE step, teacher-forced,
against the float64 step under mlp_lane_refs.step_bound; a whole trajectory judged step by step from the device's own states;
rows are independent of the batch; the table follows T on a live handle; the refusals; and the wiring through
GenerativeLevyProcess.sample at F = 1, 3, 4.  Each test prints the figures it measured (profiles/mlp_lane/README.md)."""
import numpy as np
import pytest
import torch

import dlpm_amd
from dlpm_amd import _lib
import mlp_general_refs as G
import mlp_lane_refs as R
import philox_ref
from test_gpu_draws import key_pair, update

pytestmark = pytest.mark.gpu
DEV = 'cuda'
# err_dev <= K * err_torch32, both relative L2 errors against the float64 mirror; the kernels' __expf SiLU, their k order and
# their butterfly LayerNorm sums are not torch's.  K is the worst ratio measured on the GPU over ARCHS x ROWS for the forward and
# over LOOP_ARCHS x t for the one step (profiles/mlp_lane/README.md), doubled and rounded up to a power of two -- the rule
# tests/test_gpu_train.py and tests/test_gpu_mlp_general.py state for theirs.
K = 16.0
SPARE = 7                              # rows (forward) or samples (loop) of NaN past the end of every output buffer
ERR_UNSUPPORTED = -3


def L():
    return _lib.lib()


def forward_raw(net, x, t):
    """dlpm_mlp_forward into a NaN-filled buffer with SPARE rows to spare: (the rows, the tail)."""
    rows, nf = x.shape[0], x.shape[2]
    out = torch.full((rows + SPARE, 1, nf), float('nan'), dtype=torch.float32, device=DEV)
    xd, td = x.to(DEV).contiguous(), t.to(DEV).contiguous()
    _lib.check(L().dlpm_mlp_forward(net.native_handle(), xd.data_ptr(), td.data_ptr(), out.data_ptr(), rows, _lib.stream_ptr()))
    out = out.cpu()
    return out[:rows], out[rows:]


def loop_rc(net, x, ce, cn, g, T, t_start, nsteps, offset=0, key_dev=False):
    """dlpm_mlp_sample_steps_f32 on a copy of x [B, 1, F] inside a NaN-filled buffer of B + SPARE samples.  With key_dev the key is
    read from the device, and the arguments carry a seed and an offset it has to override.  Returns (status, state, tail)."""
    B, F = x.shape[0], x.shape[2]
    buf = torch.full((B + SPARE, 1, F), float('nan'), dtype=torch.float32, device=DEV)
    buf[:B] = x.to(DEV)
    ced, cnd, gd = (v.to(DEV, torch.float32).contiguous() for v in (ce, cn, g))
    assert ced.shape == (T, B) and cnd.shape == (T, B) and gd.shape == (T,)
    kd = key_pair(offset) if key_dev else None
    args = (0xDEAD, 77, kd.data_ptr()) if key_dev else (R.SEED, offset, None)
    rc = L().dlpm_mlp_sample_steps_f32(net.native_handle(), buf.data_ptr(), ced.data_ptr(), cnd.data_ptr(), gd.data_ptr(), T, B, t_start,
                                       nsteps, *args, _lib.stream_ptr())
    torch.cuda.synchronize()
    buf = buf.cpu()
    return rc, buf[:B], buf[B:]


def loop(*a, **k):
    rc, state, tail = loop_rc(*a, **k)
    _lib.check(rc)
    assert torch.isnan(tail).all() and torch.isfinite(state).all()
    return state


def draw_tables(T, B):
    """Tables that make the state after one step from x = 0 the step's z itself: c_eps = 0, g = 1, c_noise = 1."""
    return torch.zeros(T, B), torch.ones(T, B), torch.ones(T)


# ------------------------------------------------------------------------------------------ k_mlp_forward
def judge(tag, got, want64, err32):
    assert torch.isfinite(got).all(), tag
    e = G.rel_l2(got, want64)
    print('%s err_dev %.3e err_torch32 %.3e ratio %.2f' % (tag, e, err32, e / err32))
    assert e <= K * err32, (tag, e, err32)
    np.testing.assert_allclose(got.double().numpy(), want64.numpy(), rtol=R.RTOL, atol=R.ATOL)


@pytest.mark.parametrize('arch', R.ARCHS, ids=R.arch_id)
def test_forward_against_the_float64_mirror(arch):
    x, t, y64, _, err32 = R.forward_batch(arch)
    net = R.net_of(arch)
    for rows in R.ROWS:
        got, tail = forward_raw(net, x[:rows], t[:rows])
        assert torch.isnan(tail).all(), (arch, rows)                 # nobody writes past row `rows`
        judge('forward %s rows %d' % (R.arch_id(arch), rows), got, y64[:rows], err32)


@pytest.mark.parametrize('arch', [(3, 1, 7), (2, 4, 32)], ids=R.arch_id)
def test_a_forward_row_depends_on_nothing_but_itself(arch):
    """Four rows share a wave and its LDS tile as one float4: each row alone equals, bit for bit, the row inside the batch, inside
    the reversed batch (another slot of the float4), and inside a batch whose other rows are 1e30 and NaN; two calls agree."""
    rows = 13
    x, t = (v[:rows] for v in R.forward_batch(arch)[:2])
    net = R.net_of(arch)
    whole, _ = forward_raw(net, x, t)
    assert torch.isfinite(whole).all() and torch.equal(forward_raw(net, x, t)[0], whole)
    assert torch.equal(forward_raw(net, x.flip(0), t.flip(0))[0].flip(0), whole)
    poison = torch.where(torch.arange(rows) % 2 == 0, torch.tensor(1e30), torch.tensor(float('nan')))
    for i in range(rows):
        assert torch.equal(forward_raw(net, x[i:i + 1], t[i:i + 1])[0][0], whole[i]), i
        xp, tp = poison.reshape(-1, 1, 1).expand_as(x).clone(), poison.clone()
        xp[i], tp[i] = x[i], t[i]
        assert torch.equal(forward_raw(net, xp, tp)[0][i], whole[i]), i


# ------------------------------------------------------------------------------------------ the loop's draws
DRAW_T, DRAW_STEP, DRAW_B = 6, 3, 9
DRAW_ARCH = {a[0]: a for a in reversed(R.LOOP_ARCHS)}          # F -> the first loop case with that many features


@pytest.mark.parametrize('offset', R.OFFSETS)
@pytest.mark.parametrize('F', [1, 2, 3, 4])
def test_the_loops_draws_are_a_route_of_the_step_normals(F, offset):
    """x = 0, c_eps = 0, g = 1, c_noise = 1, one step: the state is z(seed, sample, component, t) -- the bits dlpm_update_f32 draws
    at D = F on the same key and t (its scalar routes at F = 1, 2, 3, its vector route at 4), with the key in the arguments and on
    the device; the host mirror's within Z_BOUND; another t is another draw."""
    net, B = R.net_of(DRAW_ARCH[F]), DRAW_B
    x = torch.zeros(B, 1, F)
    tabs = draw_tables(DRAW_T, B)
    want, _ = update(B, F, t=DRAW_STEP, offset=offset, T=DRAW_T)
    got = loop(net, x, *tabs, DRAW_T, DRAW_STEP, 1, offset=offset).numpy().reshape(B, F)
    assert np.array_equal(got, want)
    on_dev = loop(net, x, *tabs, DRAW_T, DRAW_STEP, 1, offset=offset, key_dev=True).numpy().reshape(B, F)
    assert np.array_equal(on_dev, want)
    err = philox_ref.judge_z(got, R.step_normals(offset, B, F, DRAW_STEP))
    print('loop draws F=%d offset %d: max |z - mirror| = %.3g' % (F, offset, err))
    other = loop(net, x, *tabs, DRAW_T, DRAW_STEP - 1, 1, offset=offset).numpy().reshape(B, F)
    assert (other != got).all()
    philox_ref.judge_z(other, R.step_normals(offset, B, F, DRAW_STEP - 1))
    assert np.array_equal(other, update(B, F, t=DRAW_STEP - 1, offset=offset, T=DRAW_T)[0])


@pytest.mark.parametrize('F', [1, 2, 3, 4])
def test_steps_accumulate_in_order(F):
    """Three steps from t = 4 on the same tables: the float32 sum, taken in step order, of the three single-step draws."""
    net, B, T, off = R.net_of(DRAW_ARCH[F]), DRAW_B, DRAW_T, R.OFFSETS[1]
    x = torch.zeros(B, 1, F)
    tabs = draw_tables(T, B)
    z = [loop(net, x, *tabs, T, t, 1, offset=off).numpy() for t in (4, 3, 2)]
    assert z[0].dtype == np.float32
    want = (z[0] + z[1]) + z[2]
    assert np.array_equal(loop(net, x, *tabs, T, 4, 3, offset=off).numpy(), want)


@pytest.mark.parametrize('arch', R.LOOP_ARCHS, ids=R.arch_id)
def test_one_launch_of_n_steps_is_n_launches_of_one(arch):
    T, B, off = 6, 9, R.OFFSETS[1]
    net = R.net_of(arch)
    x, ce, cn, g = R.loop_inputs(arch, T, B)
    whole = loop(net, x, ce, cn, g, T, T - 1, T - 1, offset=off)
    s = x
    for t in range(T - 1, 0, -1):
        s = loop(net, s, ce, cn, g, T, t, 1, offset=off)
    assert torch.equal(s, whole) and not torch.equal(whole, x)
    _, same, _ = loop_rc(net, x, ce, cn, g, T, T - 1, 0, offset=off)            # no step: no change
    assert torch.equal(same, x)


# ------------------------------------------------------------------------------------------ one step against float64
def judge_step(tag, got, sd, x, t, T, ce, cn, g, z):
    """|got - step64| <= step_bound elementwise; prints err_dev, err_torch32 (step32, the same step on torch's fp32 forward) and
    their ratio.  Returns the ratio."""
    x64, eps64, zz = R.step64(sd, x, t, T, ce, cn, g, z)
    x32, _ = R.step32(sd, x, t, T, ce, cn, g, z)
    bound = R.step_bound(x, t, ce, cn, g, eps64, zz)
    err = (got.double() - x64).abs()
    e, e32 = G.rel_l2(got, x64), G.rel_l2(x32, x64)
    print('%s err_dev %.3e err_torch32 %.3e ratio %.2f, %.3f of the bound' % (tag, e, e32, e / e32, float((err / bound).max())))
    assert torch.isfinite(got).all() and (err <= bound).all(), (tag, float((err / bound).max()))
    return e / e32


@pytest.mark.parametrize('arch', R.LOOP_ARCHS, ids=R.arch_id)
def test_one_step_against_the_float64_step(arch):
    """Teacher-forced at t = 5, 3, 1 of T = 6 (B = 9: three blocks, the last with three dead waves), and at t = 1 with
    c_noise[1] = 0, where no draw is made."""
    T, B, off = 6, 9, R.OFFSETS[1]
    net, sd = R.net_of(arch), R.sd_of(arch)
    x, ce, cn, g = R.loop_inputs(arch, T, B)
    cn0 = cn.clone()
    cn0[1] = 0
    for t, c in ((5, cn), (3, cn), (1, cn), (1, cn0)):
        got = loop(net, x, ce, c, g, T, t, 1, offset=off)
        tag = 'one step %s t %d%s' % (R.arch_id(arch), t, ' no noise' if c is cn0 else '')
        ratio = judge_step(tag, got, sd, x, t, T, ce, c, g, R.step_normals(off, B, arch[0], t))
        assert ratio <= K, tag


def test_a_whole_trajectory_one_step_at_a_time():
    """All 11 steps of T = 12 as single-step calls, each judged against the float64 step from the device's own previous state."""
    arch, T, B, off = (3, 1, 7), 12, 5, R.OFFSETS[0]
    net, sd = R.net_of(arch), R.sd_of(arch)
    x, ce, cn, g = R.loop_inputs(arch, T, B)
    for t in range(T - 1, 0, -1):
        got = loop(net, x, ce, cn, g, T, t, 1, offset=off)
        judge_step('trajectory %s t %d' % (R.arch_id(arch), t), got, sd, x, t, T, ce, cn, g, R.step_normals(off, B, arch[0], t))
        x = got


# ------------------------------------------------------------------------------------------ independence of rows, the table
@pytest.mark.parametrize('arch', [(3, 1, 7), (2, 4, 32)], ids=R.arch_id)
def test_a_loop_row_depends_on_nothing_but_itself(arch):
    """Row b of a B = 9 call is the B = 1 call at sample_offset + b on that sample's table columns, bit for bit -- where the lone
    wave's three block mates are dead waves shadowing it; so are the rows of a B = 4 call in the middle."""
    T, B, off = 6, 9, R.OFFSETS[1]
    net = R.net_of(arch)
    x, ce, cn, g = R.loop_inputs(arch, T, B)
    whole = loop(net, x, ce, cn, g, T, T - 1, T - 1, offset=off)
    for b in range(B):
        alone = loop(net, x[b:b + 1], ce[:, b:b + 1], cn[:, b:b + 1], g, T, T - 1, T - 1, offset=off + b)
        assert torch.equal(alone[0], whole[b]), b
    assert torch.equal(loop(net, x[3:7], ce[:, 3:7], cn[:, 3:7], g, T, T - 1, T - 1, offset=off + 3), whole[3:7])


def test_the_table_follows_T_on_a_live_handle():
    """T = 6, then 9, then 6 on one handle: each result carries the bits a fresh handle gives (the table is rebuilt when T changes)."""
    arch, B, off = (4, 2, 33), 9, R.OFFSETS[0]
    live = R.fresh_net(arch)
    seen = {}
    for T in (6, 9, 6):
        x, ce, cn, g = R.loop_inputs(arch, T, B)
        got = loop(live, x, ce, cn, g, T, 4, 3, offset=off)
        assert torch.equal(got, loop(R.fresh_net(arch), x, ce, cn, g, T, 4, 3, offset=off)), T
        assert T not in seen or torch.equal(got, seen[T])
        seen[T] = got
    # and the table matters: the T = 9 tables' first six rows at T = 6 (t / 6 in place of t / 9) move the state
    x, ce, cn, g = R.loop_inputs(arch, 9, B)
    assert not torch.equal(loop(live, x, ce[:6], cn[:6], g[:6], 6, 4, 3, offset=off), seen[9])


# ------------------------------------------------------------------------------------------ refusals
def test_the_loop_refuses_more_than_four_features():
    for arch in [a for a in R.ARCHS if a[0] > R.LOOP_MAX_F]:
        T, B = 6, 3
        x = torch.full((B, 1, arch[0]), 7.0)
        rc, state, tail = loop_rc(R.net_of(arch), x, *draw_tables(T, B), T, T - 1, 1)
        assert rc == ERR_UNSUPPORTED and b'nfeatures <= 4' in L().dlpm_last_error(), arch
        assert (state == 7.0).all() and torch.isnan(tail).all()


def test_the_loop_refuses_a_timestep_count_beyond_24_bits():
    """purpose | t << 8 would wrap, and T sizes the table: refused before anything is allocated or launched."""
    arch, B = (1, 0, 1), 3
    net = R.fresh_net(arch)
    x = torch.full((B, 1, 1), 7.0)
    tabs = draw_tables(8, B)
    for T in (1 << 24, (1 << 24) + 5):
        buf = torch.full((B + SPARE, 1, 1), float('nan'), device=DEV)
        buf[:B] = x.to(DEV)
        ce, cn, g = (v.to(DEV) for v in tabs)
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        with pytest.raises(ValueError, match='24 bits'):
            _lib.check(L().dlpm_mlp_sample_steps_f32(net.native_handle(), buf.data_ptr(), ce.data_ptr(), cn.data_ptr(), g.data_ptr(), T, B,
                                                     5, 1, R.SEED, 0, None, _lib.stream_ptr()))
        torch.cuda.synchronize()
        # the table of this T would take T * 64 * 4 bytes = 4 GiB
        assert free_before - torch.cuda.mem_get_info()[0] < (1 << 30)
        assert (buf[:B].cpu() == 7.0).all() and torch.isnan(buf[B:]).all()
    # the handle is as it was: the largest T that fits is still a question of memory alone, and a small one runs
    T = 8
    assert torch.equal(loop(net, x, *tabs, T, 5, 1), loop(R.fresh_net(arch), x, *tabs, T, 5, 1))


@pytest.mark.parametrize('t_start,nsteps', [(6, 1), (7, 1), (2, 3), (0, 1), (5, -1)])
def test_the_loop_refuses_a_step_range_outside_the_tables(t_start, nsteps):
    arch, T, B = (2, 4, 32), 6, 3
    x = torch.full((B, 1, 2), 7.0)
    rc, state, tail = loop_rc(R.net_of(arch), x, *draw_tables(T, B), T, t_start, nsteps)
    assert rc == -1 and b'bad step range' in L().dlpm_last_error()
    assert (state == 7.0).all() and torch.isnan(tail).all()


# ------------------------------------------------------------------------------------------ through the sampler
@pytest.mark.parametrize('F', [1, 3, 4])
def test_sample_reaches_the_loop_at_every_feature_count(F):
    """GenerativeLevyProcess.sample, T = 8, B = 9: the batch is its shards at their sample offsets, bit for bit, and the one-launch
    loop agrees with the per-step path under the bound of test_fused_mlp_loop_matches_step_by_step -- set for 99 steps, so at 8 it
    catches wiring errors only; the one-step tests above judge precision."""
    model = R.net_of(DRAW_ARCH[F])
    T, alpha, B = 8, 1.7, 9

    def run(n, offset, fused=True):
        m = dlpm_amd.GenerativeLevyProcess(alpha, DEV, T, rescale_timesteps=True, seed=9, sample_offset=offset, fused_mlp=fused)
        out = m.sample({'default': model}, [n, 1, F], T)
        m.close()
        return out.cpu()
    a = run(B, 0)
    assert a.shape == (B, 1, F) and torch.isfinite(a).all() and torch.equal(run(B, 0), a)
    assert torch.equal(torch.cat([run(5, 0), run(4, 5)]), a)
    assert torch.equal(run(1, B - 1), a[B - 1:])
    b = run(B, 0, fused=False)
    diff = (a - b).abs().max().item()
    print('sample F=%d: max |one launch - step by step| = %.3g (max |x| %.3g)' % (F, diff, b.abs().max().item()))
    assert diff < 2e-4 * max(1.0, b.abs().max().item())
