"""Gradients of the toy net at any width, the part that needs no GPU: the C ABI of include/dlpm_amd_mlp_grad.h (symbols, C99,
the refusals before any device work, the parameter count of every architecture), the float64 / float32 mirror the GPU tests judge
by against torch.autograd through the MLPModel container's own modules, and the `differentiable` flag."""
import ctypes as C
import inspect

import pytest
import torch

import dlpm_amd
from dlpm_amd import _lib
import mlp_general_refs as G
import mlp_grad_refs as R

ERR_ARG, ERR_UNSUPPORTED, ERR_STATE, ERR_NOMEM = -1, -3, -4, -5


def _create(F, nu, nb, te, flags=0):
    L = _lib.lib()
    h = C.c_void_p()
    assert L.dlpm_mlp_create_ex(F, nu, nb, te, flags, C.byref(h)) == 0, L.dlpm_last_error()
    return h


def test_refusals_come_before_any_device_work():
    """Every refusal is decided on the host: the pointers below are never dereferenced."""
    L = _lib.lib()
    fake = 4096
    assert L.dlpm_mlp_grad_param_floats(None) < 0 and L.dlpm_mlp_grad_workspace_bytes(None, 4) < 0
    assert L.dlpm_mlp_grad_backward_f32(None, fake, fake, fake, 4, fake, None, fake, 1 << 40, None) == ERR_ARG
    assert L.dlpm_mlp_grad_export_params_f32(None, fake, 1, None) == ERR_ARG
    assert L.dlpm_mlp_grad_import_params_f32(None, fake, 1, None) == ERR_ARG
    h = _create(2, 128, 1, 32)
    try:
        P = L.dlpm_mlp_grad_param_floats(h)
        assert P > 0
        assert L.dlpm_mlp_grad_workspace_bytes(h, 0) < 0 and L.dlpm_mlp_grad_workspace_bytes(h, -3) < 0
        need = L.dlpm_mlp_grad_workspace_bytes(h, 4)
        assert need > 0
        for rows in (0, -1):
            assert L.dlpm_mlp_grad_backward_f32(h, fake, fake, fake, rows, fake, None, fake, 1 << 40, None) == ERR_ARG
            assert b'rows' in L.dlpm_last_error()
        for null in range(5):       # x, t, dout, grad, workspace; dx alone may be null
            a = [fake] * 5
            a[null] = None
            assert L.dlpm_mlp_grad_backward_f32(h, a[0], a[1], a[2], 4, a[3], None, a[4], need, None) == ERR_ARG
        assert L.dlpm_mlp_grad_backward_f32(h, fake, fake, fake, 4, fake, None, fake, need - 1, None) == ERR_NOMEM
        assert str(need).encode() in L.dlpm_last_error()
        # not finalized
        assert L.dlpm_mlp_grad_backward_f32(h, fake, fake, fake, 4, fake, None, fake, need, None) == ERR_STATE
        assert b'finalize' in L.dlpm_last_error()
        for fn in (L.dlpm_mlp_grad_export_params_f32, L.dlpm_mlp_grad_import_params_f32):
            assert fn(h, fake, P + 1, None) == ERR_ARG and b'parameters' in L.dlpm_last_error()
            assert fn(h, None, P, None) == ERR_ARG
            assert fn(h, fake, P, None) == ERR_STATE
    finally:
        L.dlpm_mlp_destroy(h)


def test_every_net_the_forward_takes_has_a_backward_budget():
    """The backward's LDS budget is the forward's (mlp_pack.h: mlp_gen_grad_lds_bytes), so the corner nfeatures 64, nunits 1024,
    time_emb_size 1024 is inside the supported range: the workspace query answers with a size, not with DLPM_ERR_UNSUPPORTED."""
    L = _lib.lib()
    h = _create(64, 1024, 0, 1024)
    try:
        assert L.dlpm_mlp_tile_rows(h) == 16
        assert L.dlpm_mlp_grad_workspace_bytes(h, 33) > 0
    finally:
        L.dlpm_mlp_destroy(h)


@pytest.mark.parametrize('case', list(G.CASES))
def test_param_floats_of_every_architecture(case):
    L = _lib.lib()
    nf, nb, te, nu, gn, skip, kernel = G.CASES[case]
    net = G.seeded_net(case, perturb=False)
    h = _create(nf, nu, nb, te, net.native_flags())
    try:
        assert L.dlpm_mlp_grad_param_floats(h) == sum(p.numel() for p in net.parameters())
        # the workspace: the per-row records and at most MAX_SLOTS fp64 copies of the gradient, whatever the row count
        P = L.dlpm_mlp_grad_param_floats(h)
        small, big = L.dlpm_mlp_grad_workspace_bytes(h, R.ROW_CHUNK), L.dlpm_mlp_grad_workspace_bytes(h, 1000 * R.ROW_CHUNK)
        per_row = (small - 8 * P) // R.ROW_CHUNK
        assert small > 0 and big <= per_row * 1000 * R.ROW_CHUNK + R.MAX_SLOTS * 8 * P + 8
    finally:
        L.dlpm_mlp_destroy(h)


def test_param_floats_of_the_shipped_lane_net():
    L = _lib.lib()
    h = _create(2, 64, 4, 32)
    try:
        assert L.dlpm_mlp_tile_rows(h) == 0
        assert L.dlpm_mlp_grad_param_floats(h) == 55010 == L.dlpm_mlp_param_floats(h)
        assert L.dlpm_mlp_grad_workspace_bytes(h, 65) == L.dlpm_mlp_backward_workspace_bytes(h, 65)
    finally:
        L.dlpm_mlp_destroy(h)


@pytest.mark.parametrize('case', ['u72', 'u80_noln', 'u264_te130_plain'])
def test_mirror_autograd_is_the_module_graph(case):
    """The mirror the GPU tests differentiate returns mlp_general_refs.forward's bits, and its fp32 autograd equals torch.autograd
    through the container's own modules."""
    net = G.seeded_net(case)
    gn, skip = G.CASES[case][4], G.CASES[case][5]
    x, t, dout = R.inputs(net.nfeatures, 17, 5)
    _, sd = R.leaf_state(net, torch.float32)
    assert torch.equal(R.forward(sd, x, t, gn, skip).detach(), G.forward(net.state_dict(), x, t, gn, skip, torch.float32))
    assert torch.equal(R.module_forward(net, x, t).detach(), G.forward(net.state_dict(), x, t, gn, skip, torch.float32))
    g32, dx32 = R.autograd_grads(net, x, t, dout, torch.float32)
    net.zero_grad()
    xx = x.clone().requires_grad_(True)
    (R.module_forward(net, xx, t) * dout).sum().backward()
    assert list(g32) == [n for n, _ in net.named_parameters()]
    for n, p in net.named_parameters():
        assert torch.equal(g32[n], p.grad), n
    assert torch.equal(dx32, xx.grad)
    g64, dx64 = R.autograd_grads(net, x, t, dout, torch.float64)
    assert all(g.dtype == torch.float64 for g in g64.values()) and all(R.rel(g32[n], g64[n]) < 1e-4 for n in g64)
    net.zero_grad()


def test_differentiable_flag():
    p = G.config(2, 1, 32, 128)
    net = dlpm_amd.MLPModel(p)
    assert net.differentiable is False
    assert dlpm_amd.MLPModel(p, differentiable=True).differentiable is True
    assert inspect.signature(dlpm_amd.MLPModel.__init__).parameters['differentiable'].default is False
    for bad in (1, 'yes', None):
        with pytest.raises(TypeError, match='differentiable'):
            dlpm_amd.MLPModel(p, differentiable=bad)
    net.differentiable = True       # a plain attribute
    assert net.differentiable is True


def test_the_fused_trainer_still_refuses_a_wide_net_and_names_the_autograd_route():
    net = G.seeded_net('u128', differentiable=True)
    with pytest.raises(NotImplementedError, match='64-unit') as e:
        dlpm_amd.training._refuse_model(net)
    assert 'differentiable=True' in str(e.value)
    L = _lib.lib()
    h = _create(2, 128, 1, 32)
    try:
        assert L.dlpm_mlp_param_floats(h) == ERR_UNSUPPORTED
        assert b'64-unit' in L.dlpm_last_error() and b'dlpm_amd_mlp_grad.h' in L.dlpm_last_error()
    finally:
        L.dlpm_mlp_destroy(h)
