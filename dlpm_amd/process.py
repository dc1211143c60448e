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

The step-level half (dlpm.py:158-174,204-209,226-370): `sample_A` / `compute_Sigmas` and the `A` / `Sigmas` tables of
one trajectory, the moments of one reverse step (`anterior_mean_variance_dlpm` / `_dlim`: dlpm_anterior_f32), the Proposition-8
elements (`get_two_rv_loss_elements`: dlpm_two_rv_elements_f32) and the reference's one-line helpers as torch expressions on the
device.  GPU tensors only, like the rest.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


def clamp_arg(clamp):
    """A clamp as libdlpm_amd takes it: the bound, or -1.0 for None (no clamping)."""
    return -1.0 if clamp is None else float(clamp)


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
        self.constants = None
        # the tables of one trajectory (sample_A / compute_Sigmas): [T,n] on the device, n = B (isotropic) or B * D, and the sample
        # shape they were drawn for; `A` / `Sigmas` expose them in the reference's [T, *shape] form
        self._A = self._Sigmas = self._c_eps = self._c_noise = None
        self._table_shape = None
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
        self.constants = None

    def get_schedule(self, shape):
        """(g, bg, s, bs) as [T, *shape[1:]] (dlpm.py:158-163): stride-0 expanded views of the [T] vectors, so `g[t]` broadcasts
        against a [B, ...] batch as the reference's repeated tensors do and nothing is copied."""
        tail = tuple(shape)[1:]
        return tuple(v.view(-1, *([1] * len(tail))).expand(-1, *tail)
                     for v in (self.gammas, self.bargammas, self.sigmas, self.barsigmas))

    def get_t_to_batch_size(self, x_t, t):
        """dlpm.py:165-168."""
        if isinstance(t, int):
            return torch.full([x_t.shape[0]], t).to(self.device)
        return t

    def update_constants(self, shape):
        """dlpm.py:171-174: get_schedule(shape), kept until the shape or the schedule changes."""
        if (self.constants is None) or (self.constants[0].shape != (self.diffusion_steps,) + tuple(shape)[1:]):
            self.constants = self.get_schedule(shape)
        return self.constants

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
            eps = self._draw_state(xstart.shape, self.gen_eps.kwargs.get('clamp_eps'), 1.0, seed, sample_offset, device=xstart.device)
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
        a = _lib.LossArgs()
        a.x0_dev, a.t_dev, a.a_dev, a.z_dev = x0.data_ptr(), t.data_ptr(), _lib.ptr(a_t), _lib.ptr(z_t)
        a.bg_dev, a.bs_dev = _lib.ptr(self.bargammas), _lib.ptr(self.barsigmas)
        a.x_in_dev, a.eps_dev, a.x_t_dev = x_in.data_ptr(), eps_t.data_ptr(), x_t.data_ptr()
        a.B, a.D, a.T, a.outer, a.inner = B, D, self.diffusion_steps, 1, 1
        a.flags = 0 if self.isotropic else _lib.LOSS_ELEMENTWISE
        a.alpha, a.clamp_a, a.seed, a.sample_offset = float(self.alpha), clamp_arg(self.gen_a.kwargs.get('clamp_a')), seed, sample_offset
        _lib.check(_lib.lib().dlpm_loss_elements_f32(C.byref(a), _lib.stream_ptr()))
        return x_t, eps_t

    # -------------------------------------------------------------------------------- tables of one trajectory (GPU)
    def _need_gpu(self, *tensors):
        for x in tensors:
            if torch.is_tensor(x) and not x.is_cuda:
                raise _lib.DlpmError('the DLPM helpers run on the MI355X only (the tensor is on %s); there is no CPU fallback' % x.device)
        if not tensors and torch.device(self.device).type != 'cuda':
            raise _lib.DlpmError('the DLPM helpers run on the MI355X only (the process was built on %s); there is no CPU fallback'
                                 % (self.device,))

    def _cols(self, shape):
        """(B, D, n): n table entries per timestep for samples of this shape."""
        B, D = int(shape[0]), int(np.prod(shape[1:]))
        return B, D, (B if self.isotropic else B * D)

    def _draw_A(self, T, shape, clamp_a, seed, sample_offset):
        """A table of T rows for this shape: [T,n] skewed-Levy draws, one per (row, sample) -- per (row, element) when
        non-isotropic -- clamped at clamp_a (None: not at all), from the device Philox stream (seed, sample_offset)."""
        B, D, n = self._cols(shape)
        A = torch.empty((T, n), dtype=torch.float32, device=self.device)
        L, dims = _lib.lib(), ((B,) if self.isotropic else (B, D))
        fn = L.dlpm_skewed_levy_philox_f32 if self.isotropic else L.dlpm_skewed_levy_elem_philox_f32
        with torch.cuda.device(A.device):
            _lib.check(fn(A.data_ptr(), T, *dims, float(self.alpha), clamp_arg(clamp_a), seed, sample_offset, _lib.stream_ptr()))
        return A

    def _draw_state(self, shape, clamp_eps, scale, seed, sample_offset, device=None):
        """Noise state for this shape: scale * clamp(sqrt(a) z, clamp_eps) with an unclamped skewed-Levy a per sample (per element
        when non-isotropic), gen_eps's draw, from the device Philox stream (seed, sample_offset)."""
        B, D, n = self._cols(shape)
        x = torch.empty(tuple(shape), dtype=torch.float32, device=self.device if device is None else device)
        L = _lib.lib()
        fn = L.dlpm_init_state_philox_f32 if self.isotropic else L.dlpm_init_state_elem_philox_f32
        with torch.cuda.device(x.device):
            _lib.check(fn(x.data_ptr(), B, D, float(self.alpha), clamp_arg(clamp_eps), float(scale), seed, sample_offset,
                          _lib.stream_ptr()))
        return x

    def _as_table(self, v, shape):
        """A caller's [T,B], [T,n] or (expanded) [T, *shape] table as the contiguous fp32 [T,n] the kernels read."""
        B, D, n = self._cols(shape)
        v = torch.as_tensor(v).to(self.device, torch.float32)
        v = v.reshape(v.shape[0], B, -1)
        if self.isotropic:
            v = v[:, :, 0]
        else:
            assert v.shape[2] == D, 'a non-isotropic table holds one value per element: [T, *shape]'
        return v.reshape(v.shape[0], n).contiguous()

    def _expanded(self, v, shape):
        """[..., n] -> the reference's [..., *shape]: a stride-0 view when isotropic, a plain view otherwise."""
        lead = tuple(v.shape[:-1])
        shape = tuple(shape)
        if self.isotropic:
            return v.view(*lead, shape[0], *([1] * (len(shape) - 1))).expand(*lead, *shape)
        return v.view(*lead, *shape)

    @property
    def A(self):
        """[T, *shape] as in the reference (dlpm.py:227); stored [T,B] and expanded with stride 0 when isotropic."""
        return None if self._A is None else self._expanded(self._A, self._table_shape)

    @A.setter
    def A(self, v):
        if v is None:
            self._A = self._Sigmas = self._c_eps = self._c_noise = None
            return
        assert v.dim() >= 2, 'A is [T, *shape]'
        self._table_shape = tuple(v.shape[1:])
        self._A = self._as_table(v, self._table_shape)
        self._Sigmas = self._c_eps = self._c_noise = None

    @property
    def Sigmas(self):
        """[T, *shape] as in the reference (dlpm.py:239), a view of the [T,n] table compute_Sigmas filled."""
        return None if self._Sigmas is None else self._expanded(self._Sigmas, self._table_shape)

    def sample_A(self, shape, diffusion_steps, seed=0, sample_offset=0, A=None):
        """dlpm.py:226-227: A_{1:T} of one trajectory, one skewed-Levy draw per (t, sample) -- per (t, element) when
        non-isotropic -- with gen_a's current clamp_a, from the device Philox stream (seed, sample_offset); `A=` takes the table
        as given ([T,B], or the reference's [T, *shape])."""
        self._need_gpu()
        shape = tuple(int(v) for v in shape)
        T = int(diffusion_steps)
        if A is not None:
            A = self._as_table(A, shape)
            assert A.shape[0] == T, 'A holds {} timesteps, diffusion_steps is {}'.format(A.shape[0], T)
        else:
            A = self._draw_A(T, shape, self.gen_a.kwargs.get('clamp_a'), seed, sample_offset)
        self._A, self._table_shape = A, shape
        self._Sigmas = self._c_eps = self._c_noise = None

    def compute_Sigmas(self):
        """dlpm.py:230-239: Sigma_0 = s_0^2 A_0, Sigma_t = s_t^2 A_t + g_t^2 Sigma_{t-1} (k_coeff_tables, which also leaves the two
        coefficient tables of dlpm_update_f32 for p_sample)."""
        assert self._A is not None, 'compute_Sigmas needs A: call sample_A first'
        A = self._A
        T, n = A.shape
        assert T == self.diffusion_steps, 'A holds {} timesteps, the schedule {}'.format(T, self.diffusion_steps)
        self._c_eps, self._c_noise, self._Sigmas = torch.empty_like(A), torch.empty_like(A), torch.empty_like(A)
        _lib.check(_lib.lib().dlpm_coeff_tables_f32(A.data_ptr(), _lib.ptr(self.gammas), _lib.ptr(self.sigmas), _lib.ptr(self.barsigmas),
                                                    T, n, self._c_eps.data_ptr(), self._c_noise.data_ptr(), self._Sigmas.data_ptr(),
                                                    _lib.stream_ptr()))

    # -------------------------------------------------------------------------------- one-line helpers on caller tensors (GPU)
    # torch expressions on the device in the reference's operation order; `t` an int or a [B] tensor as there

    def sample_x_t_from_xstart_given_Sigma(self, xstart, t, Sigma_t, z_t=None):
        """bg[t] xstart + Sigma_t^(1/2) z_t (dlpm.py:242-248)."""
        self._need_gpu(xstart, Sigma_t, z_t)
        g, bg, s, bs = self.update_constants(xstart.shape)
        t = self.get_t_to_batch_size(xstart, t)
        if z_t is None:
            z_t = torch.randn_like(xstart)
        return bg[t] * xstart + Sigma_t ** (1 / 2) * z_t

    def compute_Gamma_t(self, t, Sigma_t_1, Sigma_t):
        """1 - (g[t]^2 Sigma_{t-1}) / Sigma_t (dlpm.py:250-254)."""
        self._need_gpu(Sigma_t_1, Sigma_t)
        g, bg, s, bs = self.update_constants(Sigma_t_1.shape)
        t = self.get_t_to_batch_size(Sigma_t_1, t)
        return 1 - (g[t] ** 2 * Sigma_t_1) / Sigma_t

    def compute_Sigma_tilde_t_1(self, Gamma_t, Sigma_t_1):
        """dlpm.py:256-257."""
        return Gamma_t * Sigma_t_1

    def compute_m_tilde_t_1(self, x_t, t, Gamma_t, eps_t):
        """(x_t - bs[t] Gamma_t eps_t) / g[t] (dlpm.py:259-263)."""
        self._need_gpu(x_t, Gamma_t, eps_t)
        g, bg, s, bs = self.update_constants(x_t.shape)
        t = self.get_t_to_batch_size(x_t, t)
        return (x_t - bs[t] * Gamma_t * eps_t) / g[t]

    def _tables_at(self, t):
        """(Sigmas[t-1], Sigmas[t]) at the timestep of an int, a 0-d tensor or a [B] tensor whose first entry is used -- the
        per-sample reading of the reference's `self.Sigmas[t]` (a [B] tensor t gives [B,B,...] there)."""
        assert self._Sigmas is not None, 'the anterior moments need Sigmas: call sample_A and compute_Sigmas first'
        if torch.is_tensor(t):
            t = t.reshape(-1)[0].to(self._Sigmas.device, torch.int64)
        S = self.Sigmas
        return S[t - 1], S[t]

    def predict_eps_from_m_tilde(self, x_t, t, m_tilde_t_1):
        """(x_t - m_tilde g[t]) / (bs[t] Gamma_t) with Gamma_t from the process's own Sigmas (dlpm.py:204-209)."""
        self._need_gpu(x_t, m_tilde_t_1)
        g, bg, s, bs = self.update_constants(m_tilde_t_1.shape)
        S0, S1 = self._tables_at(t)
        t = self.get_t_to_batch_size(m_tilde_t_1, t)
        Gamma_t = self.compute_Gamma_t(t, S0, S1)
        return (x_t - m_tilde_t_1 * g[t]) / (bs[t] * Gamma_t)

    def compute_one_rv_Sigma_prime_t(self, t, a_t):
        """a_t bs[t]^2 (dlpm.py:388-393)."""
        self._need_gpu(a_t)
        g, bg, s, bs = self.update_constants(a_t.shape)
        t = self.get_t_to_batch_size(a_t, t)
        return a_t * bs[t] ** 2

    def compute_two_rv_prime_constants(self, t, a_t_0, a_t_1):
        """(Sigma'_{t-1}, Sigma'_t, Gamma'_t) of Proposition 8 (dlpm.py:324-332)."""
        self._need_gpu(a_t_0, a_t_1)
        g, bg, s, bs = self.update_constants(a_t_0.shape)
        Sigma_prime_t_1 = bs[t - 1] ** 2 * a_t_0
        Sigma_prime_t = s[t] ** 2 * a_t_1 + g[t] ** 2 * Sigma_prime_t_1
        return Sigma_prime_t_1, Sigma_prime_t, self.compute_Gamma_t(t, Sigma_prime_t_1, Sigma_prime_t)

    def compute_two_rv_tilde_constants(self, t, Sigma_prime_t_1, Gamma_prime_t, x_0, x_t):
        """(eps_t, m_tilde_{t-1}, Sigma_tilde_{t-1}) (dlpm.py:337-346)."""
        self._need_gpu(Sigma_prime_t_1, Gamma_prime_t, x_0, x_t)
        g, bg, s, bs = self.update_constants(x_t.shape)
        Sigma_tilde_t_1 = Gamma_prime_t * Sigma_prime_t_1
        eps_t = self.predict_eps(x_t, t, x_0)
        m_tilde_t_1 = (x_t - bs[t] * Gamma_prime_t * eps_t) / g[t]
        return eps_t, m_tilde_t_1, Sigma_tilde_t_1

    def compute_two_rv_lambda(self, t, Sigma_prime_t_1):
        """bs[t] / (2 g[t] Sigma'_{t-1}) (dlpm.py:349-353); +inf where Sigma'_{t-1} = 0 (t == 1)."""
        self._need_gpu(Sigma_prime_t_1)
        g, bg, s, bs = self.update_constants(Sigma_prime_t_1.shape)
        t = self.get_t_to_batch_size(Sigma_prime_t_1, t)
        return bs[t] / (2 * g[t] * Sigma_prime_t_1)

    # -------------------------------------------------------------------------------- the moments of one reverse step (GPU)
    def _t_scalar(self, x, t):
        """The step's timestep as a device int32 [1] tensor, without a host read: an int, a 0-d tensor, or a [B] tensor whose first
        entry is used (the loops pass torch.tensor([i] * B))."""
        if torch.is_tensor(t):
            return t.reshape(-1)[:1].to(x.device, torch.int32).contiguous()
        return torch.full([1], int(t), dtype=torch.int32, device=x.device)

    def _anterior(self, mode, x_t, t, eps, eta=0.0, Sigmas=None, want_var=True):
        self._need_gpu(x_t, eps)
        assert x_t.shape == eps.shape
        x, e = x_t.contiguous().float(), eps.contiguous().float()
        B, D, n = self._cols(x.shape)
        a = _lib.AnteriorArgs()
        if mode == _lib.ANT_DLPM:
            if Sigmas is None:
                assert self._Sigmas is not None, 'the anterior moments need Sigmas: call sample_A and compute_Sigmas first'
                Sigmas = self._Sigmas
            else:
                Sigmas = self._as_table(Sigmas, x.shape)
            assert tuple(Sigmas.shape) == (self.diffusion_steps, n), 'Sigmas is {}, expected {}'.format(
                tuple(Sigmas.shape), (self.diffusion_steps, n))
            a.Sigmas_dev = Sigmas.data_ptr()
        elif eta != 0.0:
            assert self._A is not None and tuple(self._A.shape) == (self.diffusion_steps, n), \
                'DLIM with eta > 0 needs A for this shape: call sample_A first'
            a.A_dev = self._A.data_ptr()
        td = self._t_scalar(x, t)
        mean = torch.empty_like(x)
        var = torch.empty(n, dtype=torch.float32, device=x.device) if want_var else None
        a.x_dev, a.eps_dev, a.t_dev, a.g_dev, a.bs_dev = x.data_ptr(), e.data_ptr(), td.data_ptr(), _lib.ptr(self.gammas), _lib.ptr(self.barsigmas)
        a.mean_dev, a.var_dev = mean.data_ptr(), _lib.ptr(var)
        a.B, a.D, a.T, a.mode = B, D, self.diffusion_steps, mode
        a.flags = 0 if self.isotropic else _lib.UPD_ELEMENTWISE
        a.alpha, a.eta = float(self.alpha), float(eta)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().dlpm_anterior_f32(C.byref(a), _lib.stream_ptr()))
        return mean, (self._expanded(var, x.shape) if want_var else None)

    def anterior_mean_variance_dlpm(self, x_t, t, eps, Sigmas=None):
        """(mean, variance) of the stochastic reverse step (dlpm.py:272-278), both [B, ...]: Gamma_t = 1 - g_t^2 Sigma_{t-1} / Sigma_t,
        mean = (x_t - bs_t Gamma_t eps) / g_t, variance = Gamma_t Sigma_{t-1} (a stride-0 view of [B] when isotropic).  `t`: an int,
        a 0-d tensor or a [B] tensor whose first entry is used; it is read on the device.  `Sigmas=` (this build's addition): a
        table other than the process's own.  The reference returns [B,B,...] for an int or [B] t (Sigmas[t] indexed by a
        batch-sized t); the per-sample diagonal is the contract here."""
        return self._anterior(_lib.ANT_DLPM, x_t, t, eps, Sigmas=Sigmas)

    def anterior_mean_variance_dlim(self, x_t, t, eps, eta=0.0):
        """(mean, variance) of the DLIM step (dlpm.py:281-297).  eta = 0: (x_t - bs_t eps) / g_t + bs_{t-1} eps and the
        reference's literal 0; eta > 0: s' = eta bs_{t-1}, the mean gains (bs_{t-1}^alpha - s'^alpha)^(1/alpha) eps in place of
        bs_{t-1} eps, variance = 1[t != 1] s'^2 A_t as [B, ...] (the diagonal of the reference's [B,B,...])."""
        mean, var = self._anterior(_lib.ANT_DLIM, x_t, t, eps, eta=eta, want_var=eta != 0.0)
        return mean, (0 if eta == 0.0 else var)

    # -------------------------------------------------------------------------------- Proposition 8 / 9 draws and elements (GPU)
    def get_one_rv_faster_sampling(self, shape, seed=0, sample_offset=0):
        """gen_a.generate(size=shape) (dlpm.py:384-385): one clamped skewed-Levy a per sample (per element when non-isotropic)
        expanded to `shape`, from the device Philox stream (seed, sample_offset)."""
        self._need_gpu()
        shape = tuple(int(v) for v in shape)
        a = self._draw_A(1, shape, self.gen_a.kwargs.get('clamp_a'), seed, sample_offset)
        return self._expanded(a[0], shape)

    def _two_rv(self, t, x_0, a_t_0, a_t_1, z_t, seed, sample_offset, want):
        """dlpm_two_rv_elements_f32 with the outputs named in `want`; returns them as a dict of [B, ...] tensors ([n] ones expanded)."""
        t = self._t_dev(x_0, t)
        x0 = x_0.contiguous().float()
        B, D, n = self._cols(x0.shape)
        assert (a_t_0 is None) == (a_t_1 is None), 'a_t_0 and a_t_1 are given together or not at all'
        if a_t_0 is not None:
            a_t_0, a_t_1 = (self._as_table(v.unsqueeze(0), x0.shape)[0] for v in (torch.as_tensor(a_t_0), torch.as_tensor(a_t_1)))
        if z_t is not None:
            z_t = z_t.to(x0.device, torch.float32).contiguous()
            assert z_t.shape == x0.shape
        rows = ('x_t', 'eps_t', 'm_tilde')
        out = {k: (torch.empty_like(x0) if k in rows else torch.empty(n, dtype=torch.float32, device=x0.device)) for k in want}
        a = _lib.TwoRvArgs()
        a.x0_dev, a.t_dev = x0.data_ptr(), t.data_ptr()
        a.g_dev, a.bg_dev, a.s_dev, a.bs_dev = (_lib.ptr(v) for v in (self.gammas, self.bargammas, self.sigmas, self.barsigmas))
        a.a0_dev, a.a1_dev, a.z_dev = _lib.ptr(a_t_0), _lib.ptr(a_t_1), _lib.ptr(z_t)
        for k in want:
            setattr(a, k + '_dev', out[k].data_ptr())
        a.B, a.D, a.T = B, D, self.diffusion_steps
        a.flags = 0 if self.isotropic else _lib.LOSS_ELEMENTWISE
        a.alpha, a.clamp_a, a.seed, a.sample_offset = float(self.alpha), clamp_arg(self.gen_a.kwargs.get('clamp_a')), seed, sample_offset
        with torch.cuda.device(x0.device):
            _lib.check(_lib.lib().dlpm_two_rv_elements_f32(C.byref(a), _lib.stream_ptr()))
        return {k: (v if k in rows else self._expanded(v, x0.shape)) for k, v in out.items()}

    def get_two_rv_faster_sampling(self, Xbatch, t, seed=0, sample_offset=0):
        """(a_t_0, a_t_1) of Proposition 8 (dlpm.py:308-318), each expanded to Xbatch's shape, a_t_0 zeroed where t == 1; the two
        draws get_two_rv_loss_elements makes under the same (seed, sample_offset)."""
        r = self._two_rv(t, Xbatch, None, None, None, seed, sample_offset, ('a0_out', 'a1_out'))
        return r['a0_out'], r['a1_out']

    def get_two_rv_loss_elements(self, t, x_0, a_t_0=None, a_t_1=None, z_t=None, seed=0, sample_offset=0, return_constants=False):
        """(x_t, eps_t, m_tilde_{t-1}, Sigma_tilde_{t-1}, lambda_t) of Proposition 8 at a per-sample t (dlpm.py:356-370), one
        kernel.  a_t_0 / a_t_1 ([B] or the reference's expanded [B, ...]; together) and z_t left None are drawn by the kernel from
        the Philox stream (seed, sample_offset), the a's with gen_a's current clamp_a; a_t_0 is zeroed where t == 1, so there
        Sigma_tilde = 0 and lambda = +inf as in the reference.  `return_constants` appends (Sigma'_{t-1}, Sigma'_t, Gamma'_t)."""
        want = ('x_t', 'eps_t', 'm_tilde', 'Sigma_tilde', 'lambda')
        if return_constants:
            want += ('Sigma_prime_t_1', 'Sigma_prime_t', 'Gamma_prime')
        r = self._two_rv(t, x_0, a_t_0, a_t_1, z_t, seed, sample_offset, want)
        return tuple(r[k] for k in want)
