"""Gradients of the toy net at any width on the MI355X (include/dlpm_amd_mlp_grad.h, dlpm_amd/csrc/mlp_general_grad.hip, the autograd
bridge of dlpm_amd/mlp.py and dlpm_amd/method.py): the general backward against float64 autograd with torch's own fp32 autograd as
the yardstick, its determinism and independence of the tile height, that a row's dx is that row's alone, ragged tiles, the lane
net through the new entry points, the flat-vector map, the bridge, parameter freshness after torch.optim, the differentiable
training_losses, and the reference's own training loop on a 128-unit net."""
import copy

import pytest
import torch

import dlpm_amd
from dlpm_amd import _lib
import mlp_general_refs as G
import mlp_grad_refs as R
import train_refs as T

pytestmark = pytest.mark.gpu
DEV = 'cuda'

ROW_CHUNK = R.ROW_CHUNK            # rows per chunk of the weight pass (dlpm_amd/csrc/mlp_pack.h:102, GEN_GRAD_RC)
ROWS = R.ROWS
# err_dev <= K * err_torch32 per tensor: the kernel's __expf SiLU and its summation order are not torch's.  K is the worst ratio
# measured on the GPU over CASES x tile heights x ROWS, and over the training_losses gradient below
# (profiles/mlp_grad/backward_ratios.txt), doubled and rounded up to a power of two.
K = 32.0                           # measured 11.62 (u72, dx of a single row, where torch's fp32 error is 5e-8)


def stream():
    return _lib.stream_ptr()


def method_of(p, seed=0):
    return dlpm_amd.init_method_by_parameter(dict(p, device=DEV), rng='philox', seed=seed)


_NETS = {}


def net_of(case, tile_rows=None):
    key = (case, tile_rows)
    if key not in _NETS:
        _NETS[key] = G.seeded_net(case, tile_rows=tile_rows)
    return _NETS[key]


_REFS = {}


def refs_of(case, rows):
    """The seeded inputs and the fp64 and fp32 CPU autograd gradients, computed once per (case, rows)."""
    key = (case, rows)
    if key not in _REFS:
        net = net_of(case)
        x, t, dout = R.inputs(net.nfeatures, rows, 1000 + rows)
        _REFS[key] = (x, t, dout, R.autograd_grads(net, x, t, dout, torch.float64), R.autograd_grads(net, x, t, dout, torch.float32))
    return _REFS[key]


def dev_backward(net, x, t, dout, want_dx=True, entry='grad'):
    """(flat gradient, dx) of dlpm_mlp_grad_backward_f32 (entry='train': dlpm_mlp_backward_f32); outputs and workspace start as NaN,
    so an element nobody wrote shows."""
    L = _lib.lib()
    h = net.native_handle()
    rows = x.shape[0]
    if entry == 'grad':
        P, need, fn = L.dlpm_mlp_grad_param_floats(h), L.dlpm_mlp_grad_workspace_bytes(h, rows), L.dlpm_mlp_grad_backward_f32
    else:
        P, need, fn = L.dlpm_mlp_param_floats(h), L.dlpm_mlp_backward_workspace_bytes(h, rows), L.dlpm_mlp_backward_f32
    assert P > 0 and need > 0, L.dlpm_last_error()
    ws = torch.full(((need + 7) // 8,), float('nan'), dtype=torch.float64, device=DEV)
    grad = torch.full((P,), float('nan'), dtype=torch.float32, device=DEV)
    dx = torch.full(tuple(x.shape), float('nan'), dtype=torch.float32, device=DEV)
    xd, td, dd = x.to(DEV).contiguous(), t.to(DEV).contiguous(), dout.to(DEV).contiguous()
    _lib.check(fn(h, xd.data_ptr(), td.data_ptr(), dd.data_ptr(), rows, grad.data_ptr(), dx.data_ptr() if want_dx else None,
                  ws.data_ptr(), need, stream()))
    return grad, dx


def close_to(net, got, want, g64, g32, tag):
    """Two flat gradients that sum the same rows in different chunks: per tensor within K of the yardstick's own error."""
    a, b = R.split(net, got.cpu()), R.split(net, want.cpu())
    for n in g64:
        e, e32 = R.rel(a[n], b[n]), R.rel(g32[n], g64[n])
        assert e <= K * e32, (tag, n, e, e32)


# ------------------------------------------------------------------------------------------ the backward
@pytest.mark.parametrize('tile_rows', [16, 32])
@pytest.mark.parametrize('case', list(G.CASES))
def test_backward_against_float64_autograd(case, tile_rows):
    net = net_of(case, tile_rows)
    worst = 0.0
    for rows in ROWS:
        x, t, dout, (g64, dx64), (g32, dx32) = refs_of(case, rows)
        grad, dx = dev_backward(net, x, t, dout)
        worst = max(worst, R.judge('%s tile %d rows %d' % (case, tile_rows, rows), K, R.split(net, grad.cpu()), dx.cpu(), g64, dx64,
                                   g32, dx32))
        grad2, _ = dev_backward(net, x, t, dout, want_dx=False)       # without dx the flat gradient is the same bits
        assert torch.equal(grad, grad2)
    print('%s tile %d: worst ratio over the row counts %.2f' % (case, tile_rows, worst))


@pytest.mark.parametrize('case', list(G.CASES))
def test_backward_is_deterministic_and_independent_of_the_tile_height(case):
    x, t, dout = R.inputs(G.CASES[case][0], 69, 7)
    a, adx = dev_backward(net_of(case), x, t, dout)
    b, bdx = dev_backward(net_of(case), x, t, dout)
    assert torch.equal(a, b) and torch.equal(adx, bdx)
    for tile_rows in (16, 32):
        c, cdx = dev_backward(net_of(case, tile_rows), x, t, dout)
        assert torch.equal(a, c) and torch.equal(adx, cdx), tile_rows


@pytest.mark.parametrize('case', ['u72', 'u264_te130_plain', 'u128'])
def test_a_row_depends_on_nothing_but_itself(case):
    net = net_of(case)
    x, t, dout, (g64, _), (g32, _) = refs_of(case, 69)
    keep = torch.tensor([0, 5, 15, 16, 31, 32, 47, 64, 68])
    other = torch.ones(69, dtype=torch.bool)
    other[keep] = False
    _, dx = dev_backward(net, x, t, dout)
    for poison in (1e30, float('nan')):
        xp, dp = x.clone(), dout.clone()
        xp[other], dp[other] = poison, poison
        _, dxp = dev_backward(net, xp, t, dp)
        assert torch.equal(dxp[keep], dx[keep]), poison
    # alone in a batch of their own: the same dx bits, wherever the row sits in its tile
    galone, dxalone = dev_backward(net, x[keep], t[keep], dout[keep])
    assert torch.equal(dxalone, dx[keep])
    # rows with dout = 0 leave no trace in the parameter gradient (the chunking differs, hence a tolerance)
    dz = dout.clone()
    dz[other] = 0
    gzero, dxzero = dev_backward(net, x, t, dz)
    assert torch.equal(dxzero[keep], dx[keep]) and not dxzero[other].any()
    xk, tk, dk = x[keep], t[keep], dout[keep]
    close_to(net, gzero, galone, *[R.autograd_grads(net, xk, tk, dk, d)[0] for d in (torch.float64, torch.float32)], tag=case)


@pytest.mark.parametrize('case', ['u72', 'u80_noln', 'u1024'])
def test_ragged_last_tile_leaves_no_trace(case):
    """rows = 17: one full 16-row tile and one with 15 dead rows.  The gradient equals the sum of the gradients of rows 0..15 and of
    row 16 computed on their own, within the tolerance of the backward itself; dx of each row is the same bits in both."""
    net = net_of(case, 16)
    x, t, dout, (g64, _), (g32, _) = refs_of(case, 17)
    g17, dx17 = dev_backward(net, x, t, dout)
    g16, dx16 = dev_backward(net, x[:16], t[:16], dout[:16])
    g1, dx1 = dev_backward(net, x[16:], t[16:], dout[16:])
    assert torch.equal(dx17, torch.cat([dx16, dx1]))
    close_to(net, g17, (g16.double() + g1.double()).float(), g64, g32, case)


def test_shipped_net_general_backward_against_the_lane_backward():
    gen, lane = net_of('shipped_general'), G.seeded_net('shipped_general', kernel='auto')
    assert gen.general and not lane.general
    L = _lib.lib()
    for rows in (17, ROW_CHUNK + 1):
        x, t, dout, (g64, dx64), (g32, dx32) = refs_of('shipped_general', rows)
        gg, gdx = dev_backward(gen, x, t, dout)
        lg, ldx = dev_backward(lane, x, t, dout)
        a, b = R.split(gen, gg.cpu()), R.split(gen, lg.cpu())
        for n in g64:
            assert R.rel(a[n], b[n]) <= K * max(R.rel(a[n], g64[n]), R.rel(b[n], g64[n]), R.rel(g32[n], g64[n])), (rows, n)
        assert R.rel(gdx, ldx) <= K * max(R.rel(gdx, dx64), R.rel(ldx, dx64), R.rel(dx32, dx64))
        # the new entry points on a lane handle are the old ones, bit for bit
        tg, tdx = dev_backward(lane, x, t, dout, entry='train')
        assert torch.equal(lg, tg) and torch.equal(ldx, tdx)
    h = lane.native_handle()
    P = L.dlpm_mlp_grad_param_floats(h)
    assert P == L.dlpm_mlp_param_floats(h) == 55010
    a, b = torch.empty(P, device=DEV), torch.empty(P, device=DEV)
    _lib.check(L.dlpm_mlp_grad_export_params_f32(h, a.data_ptr(), P, stream()))
    _lib.check(L.dlpm_mlp_export_params_f32(h, b.data_ptr(), P, stream()))
    assert torch.equal(a, b) and torch.equal(a.cpu(), torch.nn.utils.parameters_to_vector(lane.parameters()).detach())
    v = a + 0.05 * torch.randn(P, generator=torch.Generator().manual_seed(4)).to(DEV)
    x = torch.randn(33, 1, 2, generator=torch.Generator().manual_seed(5)).to(DEV)
    tt = torch.rand(33, generator=torch.Generator().manual_seed(6)).to(DEV)
    twin = G.seeded_net('shipped_general', kernel='auto')
    _lib.check(L.dlpm_mlp_grad_import_params_f32(h, v.data_ptr(), P, stream()))
    _lib.check(L.dlpm_mlp_import_params_f32(twin.native_handle(), v.data_ptr(), P, stream()))
    assert torch.equal(lane(x, tt), twin(x, tt))


# ------------------------------------------------------------------------------------------ the flat vector on general handles
def load_flat(net, v):
    """`net` carrying the flat vector v, through load_state_dict (the handle is rebuilt through the host)."""
    with torch.no_grad():
        torch.nn.utils.vector_to_parameters(v.detach().cpu().clone(), net.parameters())
    net.invalidate()
    return net


@pytest.mark.parametrize('case', ['u72', 'u80_noln'])
def test_export_import_on_a_general_handle(case):
    L = _lib.lib()
    net = G.seeded_net(case, seed=3)
    h = net.native_handle()
    P = L.dlpm_mlp_grad_param_floats(h)
    got = torch.full((P,), float('nan'), device=DEV)
    _lib.check(L.dlpm_mlp_grad_export_params_f32(h, got.data_ptr(), P, stream()))
    assert torch.equal(got.cpu(), torch.nn.utils.parameters_to_vector(net.parameters()).detach())
    v = torch.randn(P, generator=torch.Generator().manual_seed(4)).to(DEV)
    _lib.check(L.dlpm_mlp_grad_import_params_f32(h, v.data_ptr(), P, stream()))
    back = torch.full((P,), float('nan'), device=DEV)
    _lib.check(L.dlpm_mlp_grad_export_params_f32(h, back.data_ptr(), P, stream()))
    assert torch.equal(back, v)
    # the forward and the backward of the imported handle are those of a fresh net loaded with v: both operand regions were
    # written and the padded elements stayed 0
    fresh = load_flat(G.seeded_net(case, seed=5), v)
    x, t, dout = R.inputs(net.nfeatures, 33, 9)
    assert torch.equal(net(x.to(DEV), t.to(DEV)), fresh(x.to(DEV), t.to(DEV)))
    ga, dxa = dev_backward(net, x, t, dout)
    gb, dxb = dev_backward(fresh, x, t, dout)
    assert torch.equal(ga, gb) and torch.equal(dxa, dxb)


# ------------------------------------------------------------------------------------------ the bridge
def bridge_net(which, **kw):
    if which == 'lane':
        torch.manual_seed(1)
        return G.perturb_norms_(dlpm_amd.MLPModel(dlpm_amd.load_config('2d_data'), **kw), 1)
    return G.seeded_net(which, **kw)


@pytest.mark.parametrize('which', ['u128', 'lane'])
def test_bridge_is_the_entry_point(which):
    net, plain = bridge_net(which, differentiable=True), bridge_net(which)
    assert plain.differentiable is False and net.general == (which != 'lane')
    x, t, dout = R.inputs(2, 69, 11)
    xd, td, dd = x.to(DEV).requires_grad_(True), t.to(DEV), dout.to(DEV)
    out = net(xd, td)
    assert out.grad_fn is not None and out.requires_grad
    ref = plain(x.to(DEV), td)
    assert not ref.requires_grad and ref.grad_fn is None and torch.equal(out.detach(), ref)
    (out * dd).sum().backward()
    flat, dx = dev_backward(plain, x, t, dout)
    want = R.split(net, flat.cpu())
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, want[n]), n
    assert torch.equal(xd.grad, dx)
    with torch.no_grad():
        quiet = net(xd, td)
    assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, ref)
    with torch.inference_mode():
        assert torch.equal(net(x.to(DEV), td), ref)
    # a second backward accumulates, as autograd does
    (net(xd.detach(), td) * dd).sum().backward()
    for n, p in net.named_parameters():
        assert torch.equal(p.grad, want[n] + want[n]), n


@pytest.mark.parametrize('which', ['u128', 'lane'])
def test_parameters_changed_in_place_reach_the_handle(which):
    net = bridge_net(which, differentiable=True)
    p = G.config(2, 1, 32, 128) if which == 'u128' else dlpm_amd.load_config('2d_data')
    x, t, dout = R.inputs(2, 33, 12)
    xd, td, dd = x.to(DEV), t.to(DEV), dout.to(DEV)
    meth = method_of(p, 9)
    before = meth.sample({'default': net}, [32, 1, 2], 10)        # captures a sampler on the handle
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    (net(xd, td) * dd).sum().backward()
    opt.step()
    # a sampler captured before the step is not reused: the next sample() is a fresh net's, with no forward in between
    meth.calls = 0
    after = meth.sample({'default': net}, [32, 1, 2], 10)
    fresh = bridge_net(which)
    fresh.load_state_dict(copy.deepcopy(net.state_dict()))
    other = method_of(p, 9)
    assert torch.equal(after, other.sample({'default': fresh}, [32, 1, 2], 10)) and not torch.equal(after, before)
    assert torch.equal(net(xd, td).detach(), fresh(xd, td))
    assert not torch.equal(fresh(xd, td), bridge_net(which)(xd, td))
    # the backward after the import multiplies by the new weights too
    net.zero_grad()
    (net(xd, td) * dd).sum().backward()
    flat, _ = dev_backward(fresh, x, t, dout, want_dx=False)
    assert torch.equal(torch.cat([q.grad.reshape(-1) for q in net.parameters()]), flat.cpu())
    for m in (meth, other):
        m.close()


# ------------------------------------------------------------------------------------------ training_losses with a graph
LOSS_CASES = {'dlpm_mean': ('dlpm', dict(lploss=2.0)),
              'dlpm_median': ('dlpm', dict(lploss=1.0, loss_monte_carlo='median', monte_carlo_outer=3, monte_carlo_inner=2)),
              'dlpm_sq_clamped': ('dlpm', dict(lploss=-1, clamp_a=5.0, clamp_eps=20.0)),
              'lim': ('lim', dict(clamp_eps=20.0))}


@pytest.mark.parametrize('case', list(LOSS_CASES))
def test_differentiable_training_losses_on_the_lane_net(case):
    """The loss is the forward-only call's bits; the gradient is MLPTrainer's, bit for bit (same seeds, same call number)."""
    name, kw = LOSS_CASES[case]
    p = T.toy_config(method=name)
    B = 33
    x = dlpm_amd.get_dataset(p, DEV, 0)[0][:B].contiguous()
    net, plain, third = (bridge_net('lane', differentiable=d) for d in (True, False, False))
    out = method_of(p, 5).training_losses({'default': net}, x, **kw)
    ref = method_of(p, 5).training_losses({'default': plain}, x, **kw)
    assert out['loss'].grad_fn is not None and ref['loss'].grad_fn is None
    assert torch.equal(out['loss'].detach(), ref['loss']) and torch.equal(out['losses'], ref['losses']) and torch.equal(out['t'], ref['t'])
    assert not out['losses'].requires_grad
    with torch.no_grad():
        quiet = method_of(p, 5).training_losses({'default': net}, x, **kw)
    assert quiet['loss'].grad_fn is None and torch.equal(quiet['loss'], ref['loss'])
    out['loss'].backward()
    tr = dlpm_amd.MLPTrainer(third, method_of(p, 5), lr=0.0)
    loss = tr.step(x, **kw)
    assert torch.equal(loss, ref['loss'])
    got = torch.cat([q.grad.reshape(-1) for q in net.parameters()])
    assert torch.equal(got, tr.grad.cpu()) and got.abs().max() > 0


def objective64(net, x_in, tvec, target, dtype):
    """d(mean over rows of sqrt(mean_d (net(x_in, tvec) - target)^2)) / d(parameters) by CPU autograd in `dtype`."""
    params, sd = R.leaf_state(net, dtype)
    out = R.forward(sd, x_in.cpu().to(dtype), tvec.cpu().to(dtype), net.group_norm, net.skip_connection)
    T.loss_terms(out, target.cpu().to(dtype), 2).mean().backward()
    return {n: q.grad for n, q in params.items()}


def test_differentiable_training_losses_on_a_wide_net():
    """u128: the gradient of the whole objective against its float64 mirror on the kept x_in, tvec and target."""
    B = 33
    net = G.seeded_net('u128', differentiable=True)
    x0 = torch.randn(B, 1, 2, generator=torch.Generator().manual_seed(77)).to(DEV)
    a, b, c = (dlpm_amd.GenerativeLevyProcess(1.7, DEV, 100, rescale_timesteps=True, seed=21) for _ in range(3))
    out = a.training_losses({'default': net}, x0, lploss=2.0)
    assert out['loss'].grad_fn is not None
    ref = c.training_losses({'default': net_of('u128')}, x0, lploss=2.0)
    assert torch.equal(out['loss'].detach(), ref['loss'])
    out['loss'].backward()
    with torch.inference_mode():
        r = b._loss_terms(net, x0, 2, 1, 1, None, None, None, keep=True)
    assert torch.equal(r['losses'], out['losses'])
    g64, g32 = (objective64(net, r['x_in'], r['tvec'], r['eps_t'], d) for d in (torch.float64, torch.float32))
    R.judge('u128 training_losses', K, {n: q.grad for n, q in net.named_parameters()}, None, g64, None, g32, None)
    for m in (a, b, c):
        m.close()


# ------------------------------------------------------------------------------------------ the reference's loop
def held_out_loss(p, net, test):
    ev = dlpm_amd.EvaluationManager(method_of(p, seed=123), None, None, verbose=False)
    return ev.evaluate_loss({'default': net}, test[:4096], 1024)


class Eager(torch.nn.Module):
    """The same container driven by torch-eager fp32 ops on the GPU: the yardstick of the training run."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x, t):
        return R.module_forward(self.net, x, t)


class Draws:
    """A stand-in model through which _loss_terms makes its draws: the objective's x_in, tvec and target for the eager mirror."""

    def __call__(self, x, t, **kw):
        return torch.zeros_like(x)


def run_reference_loop(p, seed, train, test, native, steps=100, B=512, curve=None):
    """bem/TrainingManager.py:116-125 as it stands, on a 128-unit net.  Returns the held-out loss before and after; `curve`, a list,
    receives the training loss of every tenth step (a host read each, which the loop itself never makes)."""
    torch.manual_seed(seed)
    net = dlpm_amd.MLPModel(p, differentiable=native).to(DEV)
    models = {'default': net}
    method = method_of(p, seed=seed)
    opt = torch.optim.AdamW(net.parameters(), lr=p['optim']['lr'])
    eager = Eager(net)
    start = held_out_loss(p, net, test)
    idx = torch.randint(0, train.shape[0], (steps, B), generator=torch.Generator().manual_seed(seed)).to(DEV)
    for i in range(steps):
        x = train[idx[i]]
        if native:
            loss = method.training_losses(models, x)['loss']
        else:
            with torch.no_grad():
                r = method._loss_terms(Draws(), x, 2, 1, 1, None, None, None, keep=True)
            loss = T.loss_terms(eager(r['x_in'], r['tvec']), r['eps_t'], 2).mean()
        if curve is not None and i % 10 == 0:
            curve.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        opt.step()
    if not native:
        net.invalidate()        # the handle is rebuilt from the module the eager run trained
    end = held_out_loss(p, net, test)
    method.close()
    return start, end


def test_the_reference_loop_trains_a_wide_net():
    """u128 on 2d_data, B = 512, 100 iterations of the reference's loop with torch.optim.AdamW and clip_grad_norm_.  The yardstick is
    the same container trained by torch-eager fp32 autograd on the same GPU through the same 100 iterations; the two runs draw
    different noise.  Measured over three seeds (profiles/mlp_grad/README.md): see there for both curves and the spread.  The native
    run's drop of the held-out loss must be at least half of the eager run's."""
    p = G.config(2, 1, 32, 128)
    train, test = dlpm_amd.get_dataset(p, DEV, 0)
    n0, n1 = run_reference_loop(p, 0, train, test, native=True)
    e0, e1 = run_reference_loop(p, 0, train, test, native=False)
    print('held-out loss, native: %.4f -> %.4f; torch eager: %.4f -> %.4f' % (n0, n1, e0, e1))
    assert n0 == e0                      # the same initialisation, the same held-out draw
    assert e0 - e1 > 0
    assert n0 - n1 >= 0.5 * (e0 - e1)
