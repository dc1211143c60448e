"""The mirrors tests/test_gpu_mlp_lane.py judges the lane kernels by (tests/mlp_lane_refs.py), pinned without a GPU: the float64
step on the fp32 forward is the fp32 step up to the update's own roundings, the fp32 step's eps is the oracle's forward, and the
yardstick passes the bound the kernel is held to at every case and input of the GPU tests -- so a failure there means the kernel.
(The blob offsets of mlp.hip are not reachable from Python; their rounding to 4 is exercised by the odd-F, odd-TE cases on the GPU.)"""
import numpy as np
import pytest
import torch

import mlp_general_refs as G
import mlp_lane_refs as R
import philox_ref
from oracle import nets

# (T, B, the steps judged): the one-step test and the whole trajectory of tests/test_gpu_mlp_lane.py
STEP_CASES = [(6, 9, (5, 3, 1)), (12, 5, tuple(range(11, 0, -1)))]


def test_the_case_list():
    assert R.ARCHS[0] == (2, 4, 32) and len(set(R.ARCHS)) == len(R.ARCHS)
    assert [a for a in R.ARCHS if a[0] > R.LOOP_MAX_F] == [(5, 1, 64), (64, 0, 32)] and len(R.LOOP_ARCHS) == 5
    for arch in R.ARCHS:
        net = R.net_of(arch)
        assert not net.general and (net.nfeatures, net.nblocks, net.time_emb_size) == arch
        sd = net.state_dict()
        assert all((sd[k] - (1.0 if k.endswith('weight') else 0.0)).abs().max() > 0.1 for k in sd if 'group_norm' in k)
        a, b = R.fresh_net(arch).state_dict(), sd
        assert all(torch.equal(a[k], b[k]) for k in b)


def test_scaled_t_is_the_fp32_product():
    for t, T in ((1, 6), (5, 6), (3, 9), (11, 12), (99, 100), (7, 1000)):
        v = R.scaled_t(t, T)
        assert isinstance(v, np.float32) and v == np.float32(np.float32(t) * np.float32(np.float32(1) / np.float32(T)))
    # not the same number as t / T rounded once, at some of the steps the tests visit: the distinction is observable
    assert any(R.scaled_t(t, T) != np.float32(t / T) for T in (6, 9, 12) for t in range(1, T))


@pytest.mark.parametrize('arch', R.LOOP_ARCHS, ids=R.arch_id)
def test_float64_step_on_the_fp32_forward_is_the_fp32_step(arch):
    """Same eps bit for bit; x' differs by the fp32 roundings of the update alone (the last term of step_bound, with the 2^-24 of
    rounding z itself)."""
    T, B = 6, 9
    sd = R.sd_of(arch)
    x, ce, cn, g = R.loop_inputs(arch, T, B)
    for t in (5, 1):
        z = R.step_normals(R.OFFSETS[1], B, arch[0], t)
        x64, eps_a, zz = R.step64(sd, x, t, T, ce, cn, g, z, forward_dtype=torch.float32)
        x32, eps_b = R.step32(sd, x, t, T, ce, cn, g, z)
        assert torch.equal(eps_a, eps_b.double())
        gt, cet, cnt = g[t].double(), ce[t].double().reshape(-1, 1, 1), cn[t].double().reshape(-1, 1, 1)
        arith = 2.0 ** -22 * ((x.double() / gt).abs() + (cet * eps_a / gt).abs() + (cnt * zz).abs())
        assert ((x32.double() - x64).abs() <= arith).all()
        assert not torch.equal(x32.double(), x64)                                # and they are two computations


def test_fp32_step_eps_is_the_oracle_forward():
    arch = R.ARCHS[0]
    T, B = 6, 9
    x, ce, cn, g = R.loop_inputs(arch, T, B)
    for t in (5, 3, 1):
        _, eps = R.step32(R.sd_of(arch), x, t, T, ce, cn, g, np.zeros((B, arch[0])))
        tv = torch.full((B,), float(R.scaled_t(t, T)))
        with torch.no_grad():
            assert torch.equal(eps, nets.mlp_forward(R.sd_of(arch), x, tv))


@pytest.mark.parametrize('arch', R.LOOP_ARCHS, ids=R.arch_id)
def test_the_yardstick_passes_its_own_bound(arch):
    """step32 - step64 under step_bound at every loop case, every step and both offsets the GPU tests use, and at t = 1 with
    c_noise[1] = 0; the bound itself stays inside the limits its three terms state."""
    sd = R.sd_of(arch)
    worst = 0.0
    for T, B, steps in STEP_CASES:
        x, ce, cn, g = R.loop_inputs(arch, T, B)
        cn0 = cn.clone()
        cn0[1] = 0
        for t in steps:
            for off in R.OFFSETS:
                for c in ((cn, cn0) if t == 1 else (cn,)):
                    z = R.step_normals(off, B, arch[0], t)
                    x64, eps64, zz = R.step64(sd, x, t, T, ce, c, g, z)
                    assert (zz == 0).all() == (c is cn0)
                    x32, _ = R.step32(sd, x, t, T, ce, c, g, z)
                    bound = R.step_bound(x, t, ce, c, g, eps64, zz)
                    err = (x32.double() - x64).abs()
                    assert (err <= bound).all(), (T, t, off, float((err / bound).max()))
                    worst = max(worst, float((err / bound).max()))
                    # the bound is no wider than its statement: coefficients <= 1.5 / 0.8, |z| and |x| as drawn
                    top = 1.875 * (R.RTOL * eps64.abs() + R.ATOL) + 1.5 * philox_ref.Z_BOUND \
                        + 2.0 ** -22 * (1.25 * x.abs().double() + 1.875 * eps64.abs() + 1.5 * zz.abs())
                    assert (bound > 0).all() and (bound <= top * (1 + 1e-12)).all()
    print('%s: the yardstick uses at most %.3f of the one-step bound' % (R.arch_id(arch), worst))


@pytest.mark.parametrize('arch', R.ARCHS, ids=R.arch_id)
def test_forward_yardstick_keeps_the_forward_contract(arch):
    x, t, y64, y32, err32 = R.forward_batch(arch)
    assert y64.dtype == torch.float64 and y64.shape == (max(R.ROWS), 1, arch[0]) and 0 < err32 < 5e-6
    np.testing.assert_allclose(y32.double().numpy(), y64.numpy(), rtol=R.RTOL, atol=R.ATOL)
    assert G.rel_l2(y32, y64) == err32


def test_step_normals_are_the_update_kernels_draw():
    """Components 0 .. F-1 of quad 0 at the step's counter: F = 1, 2, 3 are prefixes of F = 4; another step, offset or seed is
    another draw."""
    z4 = R.step_normals(R.OFFSETS[1], 9, 4, 3)
    for F in (1, 2, 3):
        assert np.array_equal(R.step_normals(R.OFFSETS[1], 9, F, 3), z4[:, :F])
    assert z4.shape == (9, 4) and np.array_equal(z4, philox_ref.normal4(R.SEED, R.gidx(R.OFFSETS[1], 9), 0, philox_ref.P_STEP_Z, 3))
    for other in (R.step_normals(R.OFFSETS[1], 9, 4, 2), R.step_normals(R.OFFSETS[0], 9, 4, 3), R.step_normals(R.OFFSETS[1], 9, 4, 3, seed=0xDEAD)):
        assert not np.isclose(other, z4).any()
    assert np.array_equal(R.step_normals(R.OFFSETS[0] + 4, 1, 4, 3), R.step_normals(R.OFFSETS[0], 9, 4, 3)[4:5])
