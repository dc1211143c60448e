"""What the tests of the toy net's lane kernels share (dlpm_amd/csrc/mlp.hip: k_mlp_forward, k_mlp_tp_table, k_mlp_sample);
tests/test_mlp_lane_cpu.py pins these mirrors on the CPU, tests/test_gpu_mlp_lane.py judges the kernels by them.

ARCHS / LOOP_ARCHS   the (F, nblocks, TE) cases at 64 units, and those the one-launch loop takes (F <= 4)
net_of / fresh_net   train_refs.toy_net at a case: seeded, LayerNorm weights and biases away from 1 and 0
forward_batch        the case's seeded forward inputs with their float64 and torch-fp32 outputs, computed once
loop_inputs          state, per-sample coefficient tables [T, B] and g [T] of a loop test; the tables differ per sample
step_normals         the z of step t from the host mirror of the Philox draws
step64 / step32      one step of the loop in float64, and the same step on torch's fp32 forward with fp32 arithmetic (the yardstick)
step_bound           the elementwise bound on |x' - step64| of one step
"""
import numpy as np
import torch

import mlp_general_refs as G
import philox_ref
import train_refs

# (F, nblocks, TE) at 64 units, LayerNorm and skip connections: what dlpm_mlp_create routes to the lane kernels
ARCHS = [
    (2, 4, 32),     # the shipped net
    (1, 0, 1),      # the smallest net: one feature, one time-embedding unit, no mid block
    (3, 1, 7),      # odd F and odd TE: every blob offset after them is rounded up to 4
    (4, 2, 33),     # F at the loop's cap, TE not a multiple of 4
    (4, 0, 64),     # TE equal to the lane width
    (5, 1, 64),     # forward only: one feature more than the loop keeps in registers
    (64, 0, 32),    # forward only: as many features as lanes
]
LOOP_MAX_F = 4
LOOP_ARCHS = [a for a in ARCHS if a[0] <= LOOP_MAX_F]
ROWS = [1, 3, 4, 5, 13, 260]           # k_mlp_forward owns 4 rows per wave: below, at and above one wave, ragged, 65 blocks
RTOL, ATOL = 1e-5, 2e-6                # the forward contract (test_mlp_forward_matches_reference)
SEED, OFFSETS = philox_ref.SEED, philox_ref.OFFSETS


def arch_id(arch):
    return 'F%d_b%d_te%d' % arch


_NETS, _FWD = {}, {}


def fresh_net(arch):
    """A new MLPModel (and so a new native handle) with the weights of net_of(arch)."""
    return train_refs.toy_net(*arch, seed=1 + ARCHS.index(arch))


def net_of(arch):
    if arch not in _NETS:
        _NETS[arch] = fresh_net(arch)
    return _NETS[arch]


def sd_of(arch):
    return {k: v.detach() for k, v in net_of(arch).state_dict().items()}


def forward_batch(arch):
    """(x [260, 1, F], t [260], y64, y32, err_torch32): err_torch32 is the relative L2 error of torch's fp32 forward over the whole
    batch (one figure per case: over one row of a one-feature net it would be the rounding of a single number)."""
    if arch not in _FWD:
        g = torch.Generator().manual_seed(5000 + ARCHS.index(arch))
        x, t = 2 * torch.randn(max(ROWS), 1, arch[0], generator=g), torch.rand(max(ROWS), generator=g)
        with torch.no_grad():
            y64 = G.forward(sd_of(arch), x, t, True, True, torch.float64)
            y32 = G.forward(sd_of(arch), x, t, True, True, torch.float32)
        _FWD[arch] = (x, t, y64, y32, G.rel_l2(y32, y64))
    return _FWD[arch]


def gidx(offset, B):
    return (np.int64(offset) + np.arange(B, dtype=np.int64)).astype(np.uint64)


def loop_inputs(arch, T, B, seed=0):
    """x [B, 1, F] = 3 randn, c_eps and c_noise [T, B] uniform in [0.5, 1.5], g [T] in [0.8, 1.25], all float32.  Every sample has
    its own column of coefficients and every step its own row, so a wrong index into either shows."""
    g = torch.Generator().manual_seed(6000 + 97 * ARCHS.index(arch) + 13 * T + B + 1000 * seed)
    x = 3 * torch.randn(B, 1, arch[0], generator=g)
    ce = 0.5 + torch.rand(T, B, generator=g)
    cn = 0.5 + torch.rand(T, B, generator=g)
    gg = 0.8 + 0.45 * torch.rand(T, generator=g)
    return x, ce, cn, gg


def step_normals(offset, B, F, t, seed=SEED):
    """z [B, F] float64 of step t: components 0 .. F-1 of philox_normal4(seed, offset + b, quad 0, purpose 4, t)."""
    return philox_ref.normals(seed, gidx(offset, B), F, philox_ref.P_STEP_Z, t)


def scaled_t(t, T):
    """The time the net sees at step t: fl32(fl32(t) * fl32(1 / T)), as GenerativeLevyProcess rescales it; a float32 scalar."""
    return np.float32(t) * (np.float32(1) / np.float32(T))


def _eps(sd, x, t, T, dtype):
    tv = torch.full((x.shape[0],), float(scaled_t(t, T)), dtype=torch.float32)          # computed in fp32, then widened
    assert np.float32(tv[0].item()) == scaled_t(t, T)
    with torch.no_grad():
        return G.forward(sd, x, tv, True, True, dtype)


def _masked(z, cn_t):
    """z where the step draws (c_noise != 0), 0 where it does not."""
    z = torch.as_tensor(np.asarray(z, dtype=np.float64)).reshape(cn_t.shape[0], 1, -1)
    return torch.where(cn_t.reshape(-1, 1, 1) != 0, z, torch.zeros_like(z))


def step64(sd, x, t, T, ce, cn, g, z, forward_dtype=torch.float64):
    """One step of the loop from the float32 state x [B, 1, F] with the tables' rows t (ce, cn [T, B], g [T]) and z [B, F]:
    x' = (x - ce eps) / g + cn z in float64, eps = net(x, t / T) in `forward_dtype`.  Returns (x', eps, z as used), float64."""
    eps = _eps(sd, x, t, T, forward_dtype).double()
    cet, cnt, gt = ce[t].double().reshape(-1, 1, 1), cn[t].double().reshape(-1, 1, 1), g[t].double()
    zz = _masked(z, cn[t])
    return (x.double() - cet * eps) / gt + cnt * zz, eps, zz


def step32(sd, x, t, T, ce, cn, g, z):
    """The yardstick: the same step with torch's fp32 forward on the CPU, z rounded to float32 and the update in float32, one
    rounding per operation.  Returns (x', eps), float32."""
    eps = _eps(sd, x, t, T, torch.float32)
    assert eps.dtype == torch.float32
    cet, cnt = ce[t].reshape(-1, 1, 1), cn[t].reshape(-1, 1, 1)
    zz = _masked(z, cn[t]).float()
    out = (x - cet * eps) / g[t] + cnt * zz
    assert out.dtype == torch.float32
    return out, eps


def step_bound(x, t, ce, cn, g, eps64, z):
    """Elementwise bound on |x' - step64| for a step whose forward keeps the forward contract:
      |ce / g| (RTOL |eps64| + ATOL)                         the forward's error, as the update scales it
    + |cn| Z_BOUND                                           the normal's (philox_ref)
    + 2^-22 (|x / g| + |ce eps64 / g| + |cn z|)              four fp32 operations, 2^-24 relative each, on every term
    `z` is the z the step used (0 where it draws nothing)."""
    cet, cnt, gt = ce[t].double().reshape(-1, 1, 1), cn[t].double().reshape(-1, 1, 1), g[t].double()
    z = torch.as_tensor(z).double().reshape(eps64.shape)
    fwd = (cet / gt).abs() * (RTOL * eps64.abs() + ATOL)
    arith = 2.0 ** -22 * ((x.double() / gt).abs() + (cet * eps64 / gt).abs() + (cnt * z).abs())
    return fwd + cnt.abs() * philox_ref.Z_BOUND + arith
