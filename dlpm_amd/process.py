"""DLPM: the discrete-time heavy-tailed forward/backward process (sampling half).

Host-side mirror of dlpm/methods/dlpm.py:56-297 for the pieces the reverse loop needs: the noise
schedule vectors, `rescale_diffusion`, and the stateful clamp parameters of the two noise generators
(`gen_a`, `gen_eps`: bem/datasets/Data.py:17-89).  The arithmetic of the loop itself (A draws,
Sigma recursion, x_{t-1} update) lives in libdlpm_amd and keeps [T,B] scalars instead of the
reference's [T,B,C,H,W] tensors (non-isotropic noise, `isotropic=False`, is the one case that really
needs a value per element: [T,B,D] tables).

The helpers of the training half the reference exposes (`sample_x_t_from_xstart`, `predict_eps`, `predict_xstart`,
`get_one_rv_loss_elements`, dlpm.py:191-217,384-401) are thin calls into libdlpm_amd at a per-sample timestep; they take
tensors on the GPU.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


class NoiseParams:
    """The kwargs store of bem.datasets.Data.Generator (setParams mutates defaults: Data.py:60-65)."""

    def __init__(self, operation, **kwargs):
        if operation not in ('skewed_levy', 'sas'):
            raise Exception('Unknown distribution to sample from. Available distributions: {}'.format(
                ['skewed_levy', 'sas']))
        self.operation = operation
        self.kwargs = kwargs

    def setParams(self, *args, **kwargs):
        if args == () and kwargs == {}:
            raise Exception('Given void parameters')
        self.kwargs.update(kwargs)

    def get(self, name):
        return self.kwargs.get(name)


class DLPM:
    def __init__(self, alpha, device, diffusion_steps, time_spacing='linear', isotropic=True, clamp_a=None,
                 clamp_eps=None, scale='scale_preserving', native_schedule=False):
        if alpha > 2.0 or alpha <= 0.0:
            raise Exception('Wrong value of alpha ({}) for skewed levy r.v generation'.format(alpha))
        assert scale in ('scale_preserving', 'scale_exploding'), 'Unknown scale'
        self.alpha, self.device, self.time_spacing, self.isotropic, self.scale = alpha, device, time_spacing, isotropic, scale
        self.native_schedule = native_schedule
        self.gen_a = NoiseParams('skewed_levy', alpha=alpha, device=device, isotropic=isotropic, clamp_a=clamp_a)
        self.gen_eps = NoiseParams('sas', alpha=alpha, device=device, isotropic=isotropic, clamp_eps=clamp_eps)
        self._set_schedule(diffusion_steps, scale)

    def get_timesteps(self, steps):
        if self.time_spacing == 'linear':
            return torch.arange(0, steps, dtype=torch.float32)
        if self.time_spacing == 'quadratic':
            return steps * (torch.arange(0, steps, dtype=torch.float32) / steps) ** 2
        raise NotImplementedError(self.time_spacing)

    def gen_noise_schedule(self, diffusion_steps, scale='scale_preserving'):
        """[T] fp32 vectors gammas, bargammas, sigmas, barsigmas (dlpm.py:114-156).

        Several entries are differences of nearly equal fp32 numbers, so bit-level agreement with
        the reference needs the reference's own elementwise kernels: by default the T-vector is
        formed on the host with the same torch fp32 op sequence (host-side table setup, as in the
        reference, which also builds it on the CPU and copies it over, dlpm.py:76-77).
        `native_schedule=True` uses libdlpm_amd's dlpm_schedule_f32 instead (<= 1 ulp on gammas).
        """
        T = diffusion_steps
        if self.native_schedule:
            out = [np.empty(T, np.float32) for _ in range(4)]
            fn = _lib.lib().dlpm_schedule_f32 if scale == 'scale_preserving' else _lib.lib().dlpm_schedule_exploding_f32
            _lib.check(fn(T, float(self.alpha), *[o.ctypes.data for o in out]))
            return tuple(torch.from_numpy(o) for o in out)
        if scale == 'scale_exploding':                                              # dlpm.py:134-149
            ts = self.get_timesteps(T)
            sigma_min, sigma_max, rho = 0.002, 80, 7
            g, bg = torch.ones_like(ts), torch.ones_like(ts)
            bsig = (sigma_min ** (1 / rho) + (ts / (T - 1)) * (sigma_max ** (1 / rho) - sigma_min ** (1 / rho))) ** rho
            bsa = bsig ** self.alpha
            sa = torch.ones_like(bsig) * bsa[0]
            for i in range(1, len(bsig)):                 # the reference's running sums, summation order included
                sa[i] = bsa[i] - torch.sum(sa[:i])
            return g, bg, sa ** (1 / self.alpha), bsig
        assert scale == 'scale_preserving', 'Unknown scale'
        s = 0.008
        ts = self.get_timesteps(T)
        f = torch.cos((ts / T + s) / (1 + s) * torch.pi / 2) ** 2
        abar = f / f[0]
        beta = 1 - abar / torch.cat([abar[0:1], abar[0:-1]])
        g = (1 - beta) ** (1 / self.alpha)
        bg = torch.cumprod(g, dim=0)
        sig = (1 - g ** self.alpha) ** (1 / self.alpha)
        bsig = (1 - bg ** self.alpha) ** (1 / self.alpha)
        return g, bg, sig, bsig

    def _set_schedule(self, T, scale='scale_preserving'):
        self.host_schedule = tuple(v.contiguous() for v in self.gen_noise_schedule(T, scale))
        self.gammas, self.bargammas, self.sigmas, self.barsigmas = (v.to(self.device) for v in self.host_schedule)
        self.diffusion_steps = T

    def rescale_diffusion(self, diffusion_steps, time_spacing=None):
        assert isinstance(diffusion_steps, int), 'Diffusion steps must be an integer'
        if time_spacing is not None:
            self.time_spacing = time_spacing
        # as in the reference (dlpm.py:182-183) the regenerated schedule is ALWAYS scale_preserving, whatever
        # self.scale says: a scale_exploding process sampled with reverse_steps != its own switches schedule
        self._set_schedule(diffusion_steps)

    # -------------------------------------------------------------------------------- per-sample-t helpers (GPU)
    def _t_dev(self, x, t):
        """get_t_to_batch_size (dlpm.py:165-168) as int32 [B] on x's device."""
        if not x.is_cuda:
            raise _lib.DlpmError('the DLPM helpers run on the MI355X only (the tensor is on %s); there is no CPU fallback' % x.device)
        if isinstance(t, int):
            return torch.full([x.shape[0]], t, dtype=torch.int32, device=x.device)
        t = torch.as_tensor(t).to(x.device, torch.int32).contiguous()
        assert t.shape == (x.shape[0],), 't must be an int or [B]'
        return t

    def _at_t(self, mode, u, v, t):
        assert u.shape == v.shape
        t = self._t_dev(u, t)
        u, v = u.contiguous().float(), v.to(u.device).contiguous().float()
        out = torch.empty_like(u)
        B = u.shape[0]
        _lib.check(_lib.lib().dlpm_at_t_f32(mode, u.data_ptr(), v.data_ptr(), t.data_ptr(), _lib.ptr(self.bargammas),
                                            _lib.ptr(self.barsigmas), out.data_ptr(), B, u.numel() // B, self.diffusion_steps,
                                            _lib.stream_ptr()))
        return out

    def predict_xstart(self, x_t, t, eps):
        """(x_t - eps bs[t]) / bg[t]  (dlpm.py:191-196)."""
        return self._at_t(_lib.AT_T_PREDICT_XSTART, x_t, eps, t)

    def predict_eps(self, x_t, t, xstart):
        """(x_t - xstart bg[t]) / bs[t]  (dlpm.py:198-202)."""
        return self._at_t(_lib.AT_T_PREDICT_EPS, x_t, xstart, t)

    def sample_x_t_from_xstart(self, xstart, t, eps=None, seed=0, sample_offset=0):
        """(x_t, eps) with x_t = bg[t] xstart + bs[t] eps (dlpm.py:211-217).  eps=None draws gen_eps's noise -- clamp(sqrt(a) z) with
        an unclamped skewed-Levy a per sample (per element when non-isotropic) -- from the device Philox stream (seed, sample_offset)."""
        if eps is None:
            self._t_dev(xstart, 0)
            B = xstart.shape[0]
            eps = torch.empty(xstart.shape, dtype=torch.float32, device=xstart.device)
            ce = self.gen_eps.kwargs.get('clamp_eps')
            fn = _lib.lib().dlpm_init_state_philox_f32 if self.isotropic else _lib.lib().dlpm_init_state_elem_philox_f32
            _lib.check(fn(eps.data_ptr(), B, eps.numel() // B, float(self.alpha), -1.0 if ce is None else float(ce), 1.0, seed,
                          sample_offset, _lib.stream_ptr()))
        return self._at_t(_lib.AT_T_Q_SAMPLE, xstart, eps, t), eps

    def get_one_rv_loss_elements(self, t, x_0, a_t=None, z_t=None, seed=0, sample_offset=0):
        """(x_t, eps_t) of Proposition 9 (dlpm.py:395-401): x_t = bg[t] x_0 + sqrt(a_t bs[t]^2) z_t, eps_t = predict_eps(x_t, t, x_0).
        a_t: [B] or the reference's expanded [B, ...] (non-isotropic: one value per element); a_t / z_t left None are drawn by
        the kernel from the Philox stream (seed, sample_offset), a_t with gen_a's current clamp_a."""
        t = self._t_dev(x_0, t)
        x0 = x_0.contiguous().float()
        B = x0.shape[0]
        D = x0.numel() // B
        x_t, eps_t, x_in = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0)
        if a_t is not None:
            a_t = torch.as_tensor(a_t).to(x0.device, torch.float32).reshape(B, -1)
            a_t = (a_t[:, 0] if self.isotropic else a_t).contiguous()
            assert self.isotropic or a_t.shape[1] == D
        if z_t is not None:
            z_t = z_t.to(x0.device, torch.float32).contiguous()
            assert z_t.shape == x0.shape
        ca = self.gen_a.kwargs.get('clamp_a')
        a = _lib.LossArgs()
        a.x0_dev, a.t_dev, a.a_dev, a.z_dev = x0.data_ptr(), t.data_ptr(), _lib.ptr(a_t), _lib.ptr(z_t)
        a.bg_dev, a.bs_dev = _lib.ptr(self.bargammas), _lib.ptr(self.barsigmas)
        a.x_in_dev, a.eps_dev, a.x_t_dev = x_in.data_ptr(), eps_t.data_ptr(), x_t.data_ptr()
        a.B, a.D, a.T, a.outer, a.inner = B, D, self.diffusion_steps, 1, 1
        a.flags = 0 if self.isotropic else _lib.LOSS_ELEMENTWISE
        a.alpha, a.clamp_a, a.seed, a.sample_offset = float(self.alpha), -1.0 if ca is None else float(ca), seed, sample_offset
        _lib.check(_lib.lib().dlpm_loss_elements_f32(C.byref(a), _lib.stream_ptr()))
        return x_t, eps_t
