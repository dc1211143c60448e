"""TEST INFRASTRUCTURE ONLY: the Proposition-8 elements (dlpm/methods/dlpm.py:308-370) restated in NumPy fp32, one correctly
rounded operation per line in the reference's order -- what dlpm_two_rv_elements_f32 computes (include/dlpm_amd_step.h).  Shared by
tests/test_step_api_cpu.py and tests/test_gpu_step_api.py, with the F24 cases."""
import numpy as np

F24_CASES = ['s5_a1p7', 's5_a2p0', 's4_a1p7', 's4_a2p0']
F24_OUTPUTS = ('x_t', 'eps_t', 'm_tilde', 'Sigma_tilde', 'lambda', 'Sigma_prime_t_1', 'Sigma_prime_t', 'Gamma_prime')


def f24_case(f, tag):
    return {k[len(tag) + 1:]: f[k] for k in f.files if k.startswith(tag + '_')}


def two_rv_numpy(x0, t, a0, a1, z, g, bg, s, bs):
    """x0, z: [B, ...]; t: [B] ints; a0, a1: [B] (isotropic) or x0's shape (one per element).  Returns a dict keyed like F24, the
    per-sample quantities shaped as a0."""
    f32 = np.float32
    B = x0.shape[0]
    col = (B,) + (1,) * (x0.ndim - 1)
    n_shape = a0.shape
    if a0.ndim == 1:
        a0, a1 = a0.reshape(col), a1.reshape(col)
    g_, bg_, s_, bs_, bp_ = (v[t].reshape(col) for v in (g, bg, s, bs, np.roll(bs, 1)))       # np.roll(bs, 1)[t] = bs[t - 1], t >= 1
    with np.errstate(divide='ignore', invalid='ignore'):
        a0 = np.where((t == 1).reshape(col), f32(0), a0).astype(f32)
        sp1 = (bp_ * bp_) * a0
        g2 = g_ * g_
        sp = (s_ * s_) * a1 + g2 * sp1
        gam = f32(1) - (g2 * sp1) / sp
        sig_tilde = gam * sp1
        lam = bs_ / ((f32(2) * g_) * sp1)
        sq = np.sqrt(sp.astype(np.float64)).astype(f32)               # the correctly rounded fp32 root
        x_t = bg_ * x0 + sq * z
        eps_t = (x_t - x0 * bg_) / bs_
        m_tilde = (x_t - (bs_ * gam) * eps_t) / g_
    out = dict(x_t=x_t, eps_t=eps_t, m_tilde=m_tilde)
    for k, v in (('Sigma_tilde', sig_tilde), ('lambda', lam), ('Sigma_prime_t_1', sp1), ('Sigma_prime_t', sp), ('Gamma_prime', gam)):
        out[k] = np.ascontiguousarray(np.broadcast_to(v, a0.shape)).reshape(n_shape)
    assert all(v.dtype == f32 for v in out.values())
    return out
