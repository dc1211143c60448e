"""The general toy-net forward on the MI355X (include/dlpm_amd_mlp.h, dlpm_amd/csrc/mlp_general.hip): every architecture of
tests/mlp_general_refs.py against the float64 mirror with torch's own fp32 forward as the yardstick, the reference's outputs (F25),
row independence bit for bit, the shipped net on both kernels, the samplers and the consumers of model(x, t)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden
import dlpm_amd
from dlpm_amd import _lib, cli
import mlp_general_refs as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'

TILE_ROWS = (16, 32)                  # the tile heights dlpm_mlp_forward can choose (mlp_general.hip: M = 16 MT, MT = 1 or 2);
FILL_TILES = 256                      # left to itself it takes 32 rows from this many tiles on (mlp_pack.h: GEN_FILL_TILES)
MAX_ROWS = 2 * max(TILE_ROWS) + 5     # one seeded batch per case; every row count is a prefix of it
# err_dev <= K * err_torch32, both relative L2 errors against the float64 mirror: err_dev over the rows of the call, err_torch32 of
# torch's fp32 forward on the CPU over the case's whole MAX_ROWS batch (one figure per case, computed once: over a single row of a
# net with one output it would be the rounding of one number).  The kernel's __expf SiLU, its k order and its LayerNorm sums are not
# torch's.  K is the worst ratio measured on the GPU over CASES x TILE_ROWS x row counts (profiles/mlp_general/README.md), doubled
# and rounded up to a power of two -- the rule tests/test_gpu_train.py states for its K.
K = 16.0
RTOL, ATOL = 1e-5, 2e-6               # whatever K is: the forward contract of test_mlp_forward_matches_reference, elementwise


def row_counts(M):
    return [1, 3, M - 1, M, M + 1, 2 * M + 5]


_NETS, _REFS = {}, {}


def net_of(case, M=None):
    """The seeded net of a case on M-row tiles whatever the batch (None: the launcher's own choice)."""
    key = (case, M)
    if key not in _NETS:
        net = R.seeded_net(case, tile_rows=M)
        assert M is None or _lib.lib().dlpm_mlp_tile_rows(net.native_handle()) == M, (case, M)
        _NETS[key] = net
    return _NETS[key]


def refs_of(case):
    """(x, t, y64, err_torch32) on the case's seeded MAX_ROWS batch, computed once."""
    if case not in _REFS:
        nf, gn, skip = R.CASES[case][0], R.CASES[case][4], R.CASES[case][5]
        g = torch.Generator().manual_seed(4000 + list(R.CASES).index(case))
        x, t = 2 * torch.randn(MAX_ROWS, 1, nf, generator=g), torch.rand(MAX_ROWS, generator=g)
        sd = net_of(case).state_dict()
        with torch.no_grad():
            y64 = R.forward(sd, x, t, gn, skip, torch.float64)
            y32 = R.forward(sd, x, t, gn, skip, torch.float32)
        _REFS[case] = (x, t, y64, R.rel_l2(y32, y64))
    return _REFS[case]


def forward_raw(net, x, t, spare_rows):
    """dlpm_mlp_forward into a NaN-filled buffer over-allocated by `spare_rows` rows: (output rows, the spare tail)."""
    rows, nf = x.shape[0], x.shape[2]
    out = torch.full((rows + spare_rows, 1, nf), float('nan'), dtype=torch.float32, device=DEV)
    xd, td = x.to(DEV).contiguous(), t.to(DEV).contiguous()
    _lib.check(_lib.lib().dlpm_mlp_forward(net.native_handle(), xd.data_ptr(), td.data_ptr(), out.data_ptr(), rows, _lib.stream_ptr()))
    out = out.cpu()
    return out[:rows], out[rows:]


def judge(tag, got, want64, err32):
    assert torch.isfinite(got).all(), tag
    e = R.rel_l2(got, want64)
    print('%s err_dev %.3e err_torch32 %.3e ratio %.2f' % (tag, e, err32, e / err32))
    assert e <= K * err32, (tag, e, err32)
    np.testing.assert_allclose(got.double().numpy(), want64.numpy(), rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize('M', TILE_ROWS)
@pytest.mark.parametrize('case', list(R.CASES))
def test_forward_against_the_float64_mirror(case, M):
    x, t, y64, err32 = refs_of(case)
    net = net_of(case, M)
    assert 0 < _lib.lib().dlpm_mlp_lds_bytes(net.native_handle()) <= 160 * 1024
    for rows in row_counts(M):
        got, tail = forward_raw(net, x[:rows], t[:rows], M)
        assert torch.isnan(tail).all(), (case, M, rows)          # nobody writes past row `rows`
        judge('%s M %d rows %d' % (case, M, rows), got, y64[:rows], err32)


@pytest.mark.parametrize('case', list(R.CASES))
def test_forward_matches_the_reference_output(case):
    f = golden('f25_mlp_general')
    net = net_of(case)
    y = net(torch.from_numpy(f[case + '__x']).to(DEV), torch.from_numpy(f[case + '__t']).to(DEV)).cpu().numpy()
    np.testing.assert_allclose(y, f[case + '__y'], rtol=RTOL, atol=ATOL)


def test_the_launchers_own_choice_across_its_threshold():
    """Left to itself the launcher takes 16-row tiles below FILL_TILES tiles of 32 rows and 32-row tiles from there on: the rows
    on both sides of the threshold carry the bits of either forced height."""
    case = 'u16_te7_nomid'
    B = 32 * (FILL_TILES - 1) + 1                # one row more needs FILL_TILES tiles of 32 rows
    g = torch.Generator().manual_seed(9)
    x, t = 2 * torch.randn(B, 1, 2, generator=g), torch.rand(B, generator=g)
    forced = forward_raw(net_of(case, 32), x, t, 32)[0]
    assert torch.isfinite(forced).all() and torch.equal(forward_raw(net_of(case, 16), x, t, 32)[0], forced)
    for rows in (B - 1, B):
        got, tail = forward_raw(net_of(case, None), x[:rows], t[:rows], 32)
        assert torch.isnan(tail).all() and torch.equal(got, forced[:rows]), rows
    assert {_lib.lib().dlpm_mlp_tile_rows(net_of(case, m).native_handle()) for m in TILE_ROWS} == set(TILE_ROWS)


# ------------------------------------------------------------------------------------------ row independence
@pytest.mark.parametrize('M', TILE_ROWS)
def test_a_row_depends_on_nothing_but_itself(M):
    """Each row computed alone equals, bit for bit, the same row inside the batch, inside the batch reversed, and inside the batch
    with every other row replaced by 1e30 and NaN; two calls give the same bits; so do the two tile heights."""
    case = 'u128'
    x, t, _, _ = refs_of(case)
    rows = 2 * M + 5
    x, t = x[:rows], t[:rows]
    net = net_of(case, M)
    whole, _ = forward_raw(net, x, t, M)
    again, _ = forward_raw(net, x, t, M)
    assert torch.isfinite(whole).all() and torch.equal(whole, again)
    rev, _ = forward_raw(net, x.flip(0), t.flip(0), M)
    assert torch.equal(rev.flip(0), whole)
    for other in (net_of(case, TILE_ROWS[0] if M == TILE_ROWS[1] else TILE_ROWS[1]), net_of(case, None)):
        assert torch.equal(forward_raw(other, x, t, max(TILE_ROWS))[0], whole)
    poison = torch.where(torch.arange(rows) % 2 == 0, torch.tensor(1e30), torch.tensor(float('nan')))
    for i in range(rows):
        alone, _ = forward_raw(net, x[i:i + 1], t[i:i + 1], M)
        assert torch.equal(alone[0], whole[i]), i
        xp, tp = poison.reshape(-1, 1, 1).expand_as(x).clone(), poison.clone()
        xp[i], tp[i] = x[i], t[i]
        got, _ = forward_raw(net, xp, tp, M)
        assert torch.equal(got[i], whole[i]), i


# ------------------------------------------------------------------------------------------ the shipped net on both kernels
def test_shipped_net_on_both_kernels():
    x, t, y64, err32 = refs_of('shipped_general')
    general = net_of('shipped_general')
    lane = R.seeded_net('shipped_general', kernel='auto')
    assert general.general and not lane.general
    assert _lib.lib().dlpm_mlp_tile_rows(lane.native_handle()) == 0
    a, b = general(x.to(DEV), t.to(DEV)).cpu(), lane(x.to(DEV), t.to(DEV)).cpu()
    judge('shipped net, general kernel', a, y64, err32)
    judge('shipped net, lane kernel', b, y64, err32)


# ------------------------------------------------------------------------------------------ sampling
def test_injected_noise_trajectory_against_the_reference():
    f = golden('f25_mlp_general')
    model = net_of('u128')
    T, alpha = int(f['traj__meta'][0]), float(f['traj__meta'][1])
    B = f['traj__xT'].shape[0]
    L, st = _lib.lib(), _lib.stream_ptr()
    meth = dlpm_amd.GenerativeLevyProcess(alpha, DEV, T, rescale_timesteps=True)
    h = meth._native_sampler(model, [B, 1, 2], 0, 0.0, None, None, 0)
    A, xT, z = (torch.from_numpy(f[k]).to(DEV) for k in ['traj__A', 'traj__xT', 'traj__z'])
    _lib.check(L.dlpm_sampler_begin_injected(h, A.contiguous().data_ptr(), xT.contiguous().data_ptr(), st))
    for k in range(T - 1):
        _lib.check(L.dlpm_sampler_step_injected(h, z[k].contiguous().data_ptr(), st))
    x = torch.empty(B, 1, 2, device=DEV)
    _lib.check(L.dlpm_sampler_copy_state(h, x.data_ptr(), st))
    fin = f['traj__final']
    assert np.abs(x.cpu().numpy() - fin).max() < 1e-4 * max(1.0, np.abs(fin).max())
    meth.close()


def test_sample_graph_eager_hand_loop_and_shards_agree_bit_for_bit():
    model = net_of('u128')
    T, alpha, B = 12, 1.7, 37

    def run(n, offset, graph):
        m = dlpm_amd.GenerativeLevyProcess(alpha, DEV, T, rescale_timesteps=True, seed=42, sample_offset=offset, use_graph=graph)
        out = m.sample({'default': model}, [n, 1, 2], T)
        m.close()
        return out.cpu()
    full = run(B, 0, True)
    assert torch.isfinite(full).all() and full.shape == (B, 1, 2)
    assert torch.equal(run(B, 0, False), full)
    assert torch.equal(torch.cat([run(20, 0, True), run(17, 20, True)]), full)
    a = dlpm_amd.GenerativeLevyProcess(alpha, DEV, T, rescale_timesteps=True, seed=42)
    gen = a.p_sample_loop_progressive(model, [B, 1, 2])
    x = next(gen)['sample']
    for i in range(T - 1, 0, -1):
        x = a.p_sample(model, x, torch.full((B,), i, device=DEV))['sample']
    assert torch.equal(x.cpu(), full)
    a.close()


def test_one_launch_loop_refuses_a_general_handle():
    L = _lib.lib()
    model = net_of('u128')
    B, T = 4, 10
    x = torch.zeros(B, 1, 2, device=DEV)
    tab = torch.ones(T, B, device=DEV)
    g = torch.ones(T, device=DEV)
    rc = L.dlpm_mlp_sample_steps_f32(model.native_handle(), x.data_ptr(), tab.data_ptr(), tab.data_ptr(), g.data_ptr(), T, B, T - 1, 1,
                                     0, 0, None, _lib.stream_ptr())
    assert rc == -3 and b'one-launch' in L.dlpm_last_error()


# ------------------------------------------------------------------------------------------ consumers
def test_training_losses_terms_are_the_mirror_formula():
    case, B = 'u128', 33
    net = net_of(case)
    g = torch.Generator().manual_seed(77)
    x0 = torch.randn(B, 1, 2, generator=g).to(DEV)
    a, b = (dlpm_amd.GenerativeLevyProcess(1.7, DEV, 100, rescale_timesteps=True, seed=21) for _ in range(2))
    out = a.training_losses({'default': net}, x0, lploss=2.0)
    assert torch.isfinite(out['losses']).all() and torch.isfinite(out['loss']) and out['losses'].shape == (B,)
    with torch.inference_mode():
        r = b._loss_terms(net, x0, 2, 1, 1, None, None, None, keep=True)
    assert torch.equal(r['losses'], out['losses'])
    sd = net.state_dict()
    target = r['eps_t'].cpu().double()

    def terms(dtype):
        eps = R.forward(sd, r['x_in'].cpu(), r['tvec'].cpu(), True, True, dtype).double()
        return ((eps - target) ** 2).reshape(B, -1).mean(1).sqrt()
    t64, t32 = terms(torch.float64), terms(torch.float32)
    e, e32 = R.rel_l2(out['losses'].cpu(), t64), R.rel_l2(t32, t64)
    print('training_losses terms: err_dev %.3e err_torch32 %.3e ratio %.2f' % (e, e32, e / e32))
    assert e <= K * e32
    a.close()
    b.close()


def test_trainer_refuses_a_general_net():
    net = net_of('u128')
    meth = dlpm_amd.GenerativeLevyProcess(1.7, DEV, 100, rescale_timesteps=True, seed=3)
    with pytest.raises(NotImplementedError, match='64-unit'):
        dlpm_amd.MLPTrainer(net, meth, lr=1e-3)
    with pytest.raises(NotImplementedError, match='64-unit'):
        dlpm_amd.TrainingManager({'default': net}, torch.zeros(8, 1, 2, device=DEV), meth, None, None, None, batch_size=4,
                                 p=R.config(2, 1, 32, 128))
    meth.close()


def test_command_line_generates_with_a_wide_net(tmp_path):
    out = tmp_path / 'wide.npy'
    cli.main(['--config', '2d_data', '--units', '128', '--blocks', '2', '--synthetic_weights', '1', '--generate', '64', '--out', str(out)])
    s = np.load(out)
    assert s.shape == (64, 1, 2) and s.dtype == np.float32 and np.isfinite(s).all()


def test_command_line_evaluates_a_wide_net_in_2d(capsys):
    """evaluate_metrics_2d through the command line on a 128-unit net without LayerNorm: the figures are finite."""
    p = R.config(2, 1, 32, 128, group_norm=False)
    net = dlpm_amd.MLPModel(p)
    assert net.general and not any('group_norm' in k for k in net.state_dict())
    res = cli.main(['--config', '2d_data', '--units', '128', '--blocks', '1', '--synthetic_weights', '1', '--generate', '512', '--eval_2d'])
    assert all(np.isfinite(float(res[k])) for k in ('wass', 'mmd', 'precision', 'recall', 'f_1_pr'))
    assert 'eval_2d wass' in capsys.readouterr().out


@pytest.mark.parametrize('arch', [(64, 0, 16, 128, True, True), (1, 1, 1, 1, False, True), (64, 1, 1024, 1000, True, False)],
                         ids=['many_features', 'one_unit', 'wide_time_embedding'])
def test_corners_of_the_ranges(arch):
    """Beyond the case list: more output partials than hidden columns (W * F > NP), the smallest net, and a time embedding as wide
    as the cap beside 1000 units (16-row tiles only) -- the elementwise forward contract against the float64 mirror."""
    nf, nb, te, nu, gn, skip = arch
    torch.manual_seed(3)
    net = R.perturb_norms_(dlpm_amd.MLPModel(R.config(nf, nb, te, nu, gn, skip)), 3)
    g = torch.Generator().manual_seed(6)
    x, t = 2 * torch.randn(37, 1, nf, generator=g), torch.rand(37, generator=g)
    with torch.no_grad():
        y64 = R.forward(net.state_dict(), x, t, gn, skip, torch.float64)
    got, tail = forward_raw(net, x, t, 32)
    assert torch.isnan(tail).all() and torch.isfinite(got).all()
    np.testing.assert_allclose(got.double().numpy(), y64.numpy(), rtol=RTOL, atol=ATOL)
