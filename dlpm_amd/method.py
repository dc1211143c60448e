"""GenerativeLevyProcess: the sampling entry point, drop-in for the reference's method object.

Mirrors the constructor and `sample(...)` signature of
dlpm/methods/GenerativeLevyProcess.py:48-90,512-569 (what `GenerationManager.generate` and
`eval.py --generate` call).  The loop itself runs in libdlpm_amd:

  * `models['default']` is a dlpm_amd.UNetModel / MLPModel  -> dlpm_sampler_* (one reverse step
    captured as a hipGraph and replayed T-1 times); a class-conditional UNetModel with
    `model_kwargs={'y': labels}` takes the same path (the labels sit in a device buffer the graph reads);
  * any other callable `model(x, t)` on the GPU                -> the same noise / table / update
    kernels, with the model called from Python between them.

`training_losses(...)` is the forward half of the reference's objective as a held-out evaluation metric (no
backward pass): forward noising at a per-sample timestep, the net, the loss terms and the mean / median-of-means
estimator, three kernels of libdlpm_amd around one forward.  With LIM=True it is LIM's own objective (training_losses_lim): a
symmetric alpha-stable draw, a continuous time, x_t from the VPSDE coefficients, the net, and the mean smooth-L1 against -e / alpha
-- one kernel of its own (k_lim_loss_elements) and the terms / estimator kernels of the DLPM loss.

One step at a time: `p_mean_variance`, `p_sample`, `ddim_sample` and the progressive loops
(`p_sample_loop_progressive`, `ddim_sample_loop_progressive`) with the reference's signatures.  A progressive loop takes the
trajectory's Philox key and tables at its first item; the step methods use them from then on, so a loop written by hand around
`p_sample` draws what `p_sample_loop` draws.

Two RNG modes:
  rng='philox'     device Philox4x32-10 keyed by (seed, GLOBAL sample index, step, element): the
                   samples do not depend on how a batch is sharded over GPUs (default);
  rng='reference'  the reference's CPU streams (numpy MT19937 -> scipy-style CMS, torch MT19937 ->
                   randn) regenerated on the host by libdlpm_amd and uploaded, for parity with the
                   reference CPU path on identical seeds.
"""
import contextlib
import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib
from .process import DLPM, clamp_arg


class ModelMeanType:
    """What the net predicts (dlpm/methods/dlpm.py:10-18)."""
    PREVIOUS_X = 'PREVIOUS_X'   # the anterior mean m_tilde_{t-1}
    START_X = 'START_X'         # x_0
    EPSILON = 'EPSILON'         # eps (every shipped config)
    Z = 'Z'                     # z_t


class ModelVarType:
    FIXED = 'FIXED'


class LossType:
    """dlpm/methods/dlpm.py:34-42; only EPS_LOSS is implemented there and here."""
    LP_LOSS = 'LP_LOSS'
    MEAN_LOSS = 'MEAN_LOSS'
    EPS_LOSS = 'EPS_LOSS'
    LAMBDA_LOSS = 'LAMBDA_LOSS'
    VAR_KL = 'VAR_KL'
    VAR_LP_SUM = 'VAR_LP_SUM'


class ReferenceStreams:
    """Stream N (numpy global RandomState, consumed by scipy's levy_stable.rvs) and stream P (torch's
    default CPU generator), as libdlpm_amd MT19937 states."""

    def __init__(self, np_seed=0, torch_seed=0):
        self.N, self.P = _lib.MT19937(), _lib.MT19937()
        L = _lib.lib()
        _lib.check(L.dlpm_mt19937_seed(C.byref(self.N), np_seed & 0xFFFFFFFF))
        _lib.check(L.dlpm_mt19937_seed(C.byref(self.P), torch_seed & 0xFFFFFFFF))
        # torch's own CPU generator under the same seed: the draws of training_losses (`randint`, `randn_like`), which
        # equal the default generator's after torch.manual_seed(torch_seed) bit for bit
        self.G = torch.Generator().manual_seed(torch_seed & 0xFFFFFFFF)

    @classmethod
    def from_global_numpy(cls, torch_seed):
        """Continue numpy's process-global stream exactly where it stands (write back with
        `store_global_numpy`)."""
        s = cls(0, torch_seed)
        kind, key, pos, _, _ = np.random.get_state()
        assert kind == 'MT19937'
        for i in range(624):
            s.N.key[i] = int(key[i])
        s.N.pos = int(pos)
        return s

    def store_global_numpy(self):
        key = np.array([self.N.key[i] for i in range(624)], dtype=np.uint32)
        np.random.set_state(('MT19937', key, int(self.N.pos), 0, 0.0))

    def skewed_levy(self, alpha, n, clamp_a=None):
        out = np.empty(n, np.float32)
        _lib.check(_lib.lib().dlpm_skewed_levy_host_f32(C.byref(self.N), float(alpha), n,
                                                       clamp_arg(clamp_a), out.ctypes.data))
        return torch.from_numpy(out)

    def randn(self, shape):
        n = int(np.prod(shape))
        out = np.empty(n, np.float32)
        _lib.check(_lib.lib().dlpm_randn_host_f32(C.byref(self.P), n, out.ctypes.data))
        return torch.from_numpy(out).reshape(list(shape))


class _TrainingLoss(torch.autograd.Function):
    """training_losses with a graph, for a differentiable MLPModel: the forward is the launches the forward-only call makes (the
    same bits), kept; the backward is dlpm_loss_grad_f32 times the incoming gradient and one backward of the net -- the pieces
    MLPTrainer.step composes.  Returns (loss, terms, t); only the loss is differentiable, with respect to the net's parameters."""

    @staticmethod
    def forward(ctx, method, model, spec, x_start, *params):
        B = int(x_start.shape[0])
        if spec['lim']:
            r = method._lim_loss_terms(model, x_start, spec['clamp_eps'], spec['noise'], keep=True)
            out, target, x_in, tvec = r['output'], r['score'], r['x_t'], r['t']
            lp, outer, inner, median = 1, 1, 1, None
        else:
            lp, outer, inner = spec['lploss'], spec['outer'], spec['inner']
            r = method._loss_terms(model, x_start, lp, outer, inner, None, spec['clamp_a'], spec['noise'], keep=True)
            out, target, x_in, tvec = r['model_eps'], r['eps_t'], r['x_in'], r['tvec']
            median = torch.empty(B, dtype=torch.int32, device=x_start.device) if spec['median'] else None
        loss = method._loss_reduce(r['losses'], B, outer, inner, 'median' if median is not None else 'mean', False, median_index=median)
        ctx.model, ctx.key, ctx.dims, ctx.median = model, model._imported, (B, outer, inner, lp), median
        ctx.save_for_backward(out, target, r['losses'], x_in, tvec)
        ctx.mark_non_differentiable(r['losses'], r['t'])
        return loss.clone(), r['losses'], r['t']

    @staticmethod
    def backward(ctx, gloss, _glosses, _gt):
        out, target, terms, x_in, tvec = ctx.saved_tensors
        model, (B, outer, inner, lp) = ctx.model, ctx.dims
        if model._imported != ctx.key:
            raise RuntimeError('a parameter of the MLPModel was modified between training_losses and this backward; the native '
                               'handle holds the newer values')
        with torch.cuda.device(out.device):
            dmodel = torch.empty_like(out)
            _lib.check(_lib.lib().dlpm_loss_grad_f32(out.data_ptr(), target.data_ptr(), terms.data_ptr(), _lib.ptr(ctx.median),
                                                     dmodel.data_ptr(), B, outer, inner, int(x_in[0].numel()), lp, _lib.stream_ptr()))
            dmodel.mul_(gloss.to(dmodel.dtype))
            flat, _ = model.native_backward(x_in, tvec, dmodel)
        return (None, None, None, None) + tuple(g if ctx.needs_input_grad[4 + i] else None for i, g in enumerate(model.split_flat(flat)))


def _wants_graph(model):
    from .mlp import MLPModel
    return (isinstance(model, MLPModel) and model.differentiable and torch.is_grad_enabled()
            and any(p.requires_grad for p in model.parameters()))


class GenerativeLevyProcess:
    def __init__(self, alpha, device, reverse_steps, model_mean_type=ModelMeanType.EPSILON,
                 model_var_type=ModelVarType.FIXED, time_spacing='linear', rescale_timesteps=False, isotropic=True,
                 LIM=False, scale='scale_preserving', input_scaling=False,
                 rng='philox', seed=0, sample_offset=0, use_graph=True, reference_streams=None, fused_mlp=True):
        # The reference constructor asserts EPSILON here (GenerativeLevyProcess.py:74-77) although p_mean_variance carries
        # the START_X / Z / PREVIOUS_X branches (:186-207), reachable there only by setting `model_mean_type` afterwards.
        # This build runs them (dlpm_predict_f32); the variance stays FIXED as in the reference.
        assert model_mean_type in _lib.MEAN_TYPES, 'unknown model_mean_type {}'.format(model_mean_type)
        assert model_var_type == ModelVarType.FIXED, 'Only fixed variance is supported for the moment'
        if LIM:
            assert (model_mean_type == ModelMeanType.EPSILON) and rescale_timesteps, \
                'LIM only supports epsilon prediction, fixed variance and rescaled timesteps'
            if not isotropic:
                raise NotImplementedError('the LIM sampler is isotropic only (its non-isotropic branch is commented '
                                          'out in the reference, LIM/functions/sampler.py:144-148)')
            from .lim import VPSDE
            self.sde = VPSDE(alpha, 'cosine')
        assert rng in ('philox', 'reference')
        self.alpha, self.device, self.reverse_steps = alpha, device, reverse_steps
        self.model_mean_type, self.model_var_type = model_mean_type, model_var_type
        self.time_spacing, self.rescale_timesteps, self.isotropic = time_spacing, rescale_timesteps, isotropic
        self.LIM, self.input_scaling = LIM, input_scaling
        self.rng, self.seed, self.sample_offset, self.use_graph = rng, seed, sample_offset, use_graph
        self.reference_streams = reference_streams
        self.fused_mlp = fused_mlp
        self.dlpm = DLPM(alpha, device, diffusion_steps=reverse_steps, time_spacing=time_spacing, isotropic=isotropic,
                         scale=scale)
        self._samplers = {}
        self.calls = 0          # number of sample() calls so far: folded into the Philox key
        self._dataset = None    # see dataset_stream()
        self._traj = None       # (seed, first global sample index) of the trajectory a progressive loop began: p_sample's Philox key
        self._native_owner = None   # the progressive generator that currently drives the native sampler (see _progressive)

    # -------------------------------------------------------------------------------- helpers
    def _scale_timesteps(self, t):
        if self.rescale_timesteps:
            return t.float() * (1.0 / self.reverse_steps)
        return t

    def get_timesteps(self, N, **kwargs):
        return self.dlpm.get_timesteps(N)

    def _philox_key(self):
        """(seed, first global sample index) of the next sample() call."""
        calls, first = (self._dataset['calls'], self._dataset['next']) if self._dataset else (self.calls, 0)
        return (self.seed + 0x9E3779B97F4A7C15 * calls) & 0xFFFFFFFFFFFFFFFF, self.sample_offset + first

    def _advance_key(self, n):
        """n samples were drawn under _philox_key(): the dataset stream moves on by n, or the call counter by one."""
        if self._dataset is not None:
            self._dataset['next'] += n
        else:
            self.calls += 1

    def _takes_native(self, model, model_kwargs, denoised_fn=None):
        """Whether the native (graph) sampler takes this call: one of the package's nets, scaled timesteps, no Python hook on
        the x_0 prediction, and model_kwargs it carries."""
        from .unet import UNetModel
        from .mlp import MLPModel
        return isinstance(model, (UNetModel, MLPModel)) and self.rescale_timesteps and denoised_fn is None and \
            _native_kwargs(model, model_kwargs)

    @contextlib.contextmanager
    def dataset_stream(self, first_index=0):
        """Inside this context every sample() call continues ONE Philox stream indexed by the running sample
        count, so the i-th generated sample does not depend on how the G samples are cut into chunks
        (EvaluationManager's eval.batch_size loop) or split over ranks.  Outside it each call draws a fresh
        stream, as successive reference calls do.  No effect with rng='reference' (the MT19937 streams
        simply continue, which is the reference's behaviour)."""
        assert self._dataset is None, 'dataset_stream() does not nest'
        self._dataset = dict(calls=self.calls, next=first_index)
        try:
            yield self
        finally:
            self._dataset = None
            self.calls += 1

    def _input_scale(self):
        """[T] host table 1/(1 + barsigma_t), or None: the factor the net input is multiplied by when input_scaling
        is on and the process was built scale_exploding (GenerativeLevyProcess.py:176-180)."""
        if self.input_scaling and self.dlpm.scale == 'scale_exploding':
            return (1 / (1 + self.dlpm.host_schedule[3])).contiguous()
        return None

    def _streams(self):
        if self.reference_streams is None:
            self.reference_streams = ReferenceStreams(self.seed, self.seed)
        return self.reference_streams

    def _native_sampler(self, model, shape, flags, eta, clamp_a, clamp_eps, seed, offset=None):
        offset = self.sample_offset if offset is None else offset
        self._native_owner = None       # whoever was stepping the native sampler has lost its state
        lim = bool(flags & _lib.SMP_LIM)
        from .unet import UNetModel
        B = shape[0]
        if isinstance(model, UNetModel):
            assert len(shape) == 4 and shape[2] == shape[3], shape
            dims = (shape[1], shape[2], shape[3])
            handles = dict(unet=model.native_handle(shape[2]), mlp=None)
        else:
            assert len(shape) == 3 and shape[1] == 1, shape
            dims = (1, 1, shape[2])
            handles = dict(unet=None, mlp=model.native_handle())
        if not self.isotropic:
            flags |= _lib.UPD_ELEMENTWISE
        # the handle GENERATION, not its address: after load_state_dict / invalidate() a new handle is likely to get the
        # old one's address back from the allocator, and a cached sampler's hipGraph still points at the freed weights
        key = (id(model), model.handle_generation, tuple(shape),
               self.reverse_steps, self.alpha, flags, eta, clamp_a, clamp_eps, self.use_graph, self.fused_mlp,
               self.dlpm.host_schedule[3].data_ptr(), self._input_scale() is not None, self.model_mean_type)
        ent = self._samplers.get(key)
        if ent is not None:
            _lib.check(_lib.lib().dlpm_sampler_reseed(ent['h'], seed, offset))
            return ent['h']
        # one live native sampler per method object: they own activation workspaces sized for B
        for k in list(self._samplers):
            _lib.lib().dlpm_sampler_destroy(self._samplers.pop(k)['h'])
        cfg = _lib.SamplerConfig()
        cfg.unet, cfg.mlp = handles['unet'], handles['mlp']
        cfg.B, (cfg.C, cfg.H, cfg.W), cfg.T = B, dims, self.reverse_steps + (1 if lim else 0)
        cfg.alpha = float(self.alpha)
        cfg.clamp_a, cfg.clamp_eps = clamp_arg(clamp_a), clamp_arg(clamp_eps)
        cfg.flags = flags | (0 if self.fused_mlp else _lib.SMP_NO_FUSED_MLP)
        cfg.dlim_eta, cfg.seed = float(eta), seed
        cfg.mean_type = _lib.MEAN_TYPES[self.model_mean_type]
        gs = 0
        if self.use_graph and self.rng == 'philox':
            # steps per captured graph: 1 for the UNets (~150 launches, ms-long steps), 33 for the
            # launch-bound MLP (4 launches per step) unless the caller asked for a specific count
            gs = self.use_graph if isinstance(self.use_graph, int) and not isinstance(self.use_graph, bool) else (
                1 if handles['unet'] else 33)
        cfg.sample_offset, cfg.use_graph = offset, gs
        sched = self.dlpm.host_schedule
        cfg.g, cfg.bg, cfg.s, cfg.bs = (v.data_ptr() for v in sched)
        isc = None if lim else self._input_scale()
        if isc is not None:
            cfg.in_scale = isc.data_ptr()
        if lim:
            from .lim import lim_tables
            tabs = lim_tables(self.sde, self.reverse_steps, bool(flags & _lib.UPD_DLIM))     # kept alive until create returns
            cfg.lim_ts, cfg.lim_tmp, cfg.lim_cx, cfg.lim_cs, cfg.lim_cn = (v.data_ptr() for v in tabs)
        h = C.c_void_p()
        _lib.check(_lib.lib().dlpm_sampler_create(C.byref(cfg), C.byref(h)))
        self._samplers[key] = dict(h=h, model=weakref.ref(model))
        model._dependents.add(self)
        return h

    def _drop_samplers_of(self, model):
        """Called by a model before it destroys its native handle: samplers built on it go first."""
        for k in list(self._samplers):
            m = self._samplers[k]['model']()
            if m is None or m is model:
                _lib.lib().dlpm_sampler_destroy(self._samplers.pop(k)['h'])

    def close(self):
        for k in list(self._samplers):
            _lib.lib().dlpm_sampler_destroy(self._samplers.pop(k)['h'])

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -------------------------------------------------------------------------------- loops
    def _host_noise_prologue(self, shape, clamp_a, clamp_eps, noise):
        """A[T,B] and x_T from the reference's CPU streams, in its draw order."""
        st = self._streams()
        T, B = self.reverse_steps, shape[0]
        n = B if self.isotropic else int(np.prod(shape))       # non-isotropic: one draw per element (Distributions.py:48)
        A = torch.stack([st.skewed_levy(self.alpha, n, clamp_a) for _ in range(T)])       # dlpm.py:226-227
        if noise is not None:
            xT = noise.detach().to('cpu', torch.float32)
        else:                                                                             # GLP.py:313
            a0 = st.skewed_levy(self.alpha, n, None)           # gen_sas draws its own UNclamped a
            a0 = a0.view(-1, *([1] * (len(shape) - 1))) if self.isotropic else a0.view(shape)
            e = torch.sqrt(a0) * st.randn(shape)
            if clamp_eps is not None:
                e = torch.clamp(e, -clamp_eps, clamp_eps)
            xT = self.dlpm.host_schedule[3][-1] * e
        return A.contiguous(), xT.contiguous()

    def _host_noise_prologue_lim(self, shape, clamp_eps):
        """x_0 = gen_eps.generate(shape) then one unclamped a per (step, sample), in the reference's draw order on
        stream N: a_0 first (GenerativeLevyProcess.py:464), then step by step (LIM/functions/sampler.py:143)."""
        st = self._streams()
        steps, B = self.reverse_steps, shape[0]
        a0 = st.skewed_levy(self.alpha, B, None) if self.alpha != 2.0 else torch.full((B,), 2.0)
        e = torch.sqrt(a0.view(-1, *([1] * (len(shape) - 1)))) * st.randn(shape)
        if clamp_eps is not None:
            e = torch.clamp(e, -clamp_eps, clamp_eps)
        return a0, e.contiguous()

    def _run_native(self, model, shape, flags, eta, clamp_a, clamp_eps, noise, history, progress, labels=None):
        L, st = _lib.lib(), _lib.stream_ptr()
        lim = bool(flags & _lib.SMP_LIM)
        T = self.reverse_steps + (1 if lim else 0)      # LIM runs `reverse_steps` updates, DLPM reverse_steps - 1
        seed, offset = self._philox_key()
        if getattr(model, 'num_classes', None) is not None:
            if lim:
                raise NotImplementedError('the LIM sampler does not take class labels')
            labels = model._check_labels(shape[0], labels)      # the reference's checks, before any device work
        h = self._native_sampler(model, shape, flags, eta, clamp_a, clamp_eps, seed, offset)
        dev = torch.device(self.device)
        if labels is not None:
            # into the sampler's own buffer: its captured graph reads them from there, so new labels need no recapture
            y_d = labels.to(dev, torch.int64).contiguous()
            _lib.check(L.dlpm_sampler_set_labels(h, y_d.data_ptr(), st))
        x = torch.empty(shape, dtype=torch.float32, device=dev)
        # the update kernel stores every intermediate state into this buffer (row T - t), inside the graph
        hist = torch.empty([T] + list(shape), dtype=torch.float32, device=dev) if history else None
        _lib.check(L.dlpm_sampler_set_history(h, hist.data_ptr() if history else None, st))

        pbar = _progress_bar(progress, T)
        if lim and self.rng == 'reference':
            # stream N interleaves with the model calls in the reference but is independent of stream P, so all the
            # per-step a's can be drawn up front
            _, x0 = self._host_noise_prologue_lim(shape, clamp_eps)
            ode = bool(flags & _lib.UPD_DLIM)
            A = torch.ones((T - 1, shape[0])) if (ode or self.alpha == 2.0) else torch.stack(
                [self._streams().skewed_levy(self.alpha, shape[0], None) for _ in range(T - 1)])
            A_d, x0_d = A.contiguous().to(dev), x0.to(dev)
            _lib.check(L.dlpm_sampler_begin_injected(h, A_d.data_ptr(), x0_d.data_ptr(), st))
            for _ in range(T - 1):
                z_d = None if ode else self._streams().randn(shape).to(dev)
                _lib.check(L.dlpm_sampler_step_injected(h, z_d.data_ptr() if z_d is not None else None, st))
                if pbar:
                    pbar.update(1)
        elif self.rng == 'reference' or noise is not None:
            A, xT = self._host_noise_prologue(shape, clamp_a, clamp_eps, noise)
            A_d, xT_d = A.to(dev), xT.to(dev)
            _lib.check(L.dlpm_sampler_begin_injected(h, A_d.data_ptr(), xT_d.data_ptr(), st))
            need_z = not (flags & _lib.UPD_DLIM) or eta != 0.0
            for _ in range(T - 1):
                z_d = self._streams().randn(shape).to(dev) if (need_z and self.rng == 'reference') else None
                if z_d is None and need_z:
                    z_d = torch.randn(shape, device=dev)
                _lib.check(L.dlpm_sampler_step_injected(h, z_d.data_ptr() if z_d is not None else None, st))
                if pbar:
                    pbar.update(1)
        else:
            _lib.check(L.dlpm_sampler_begin(h, st))
            if pbar:
                for _ in range(T - 1):
                    _lib.check(L.dlpm_sampler_steps(h, 1, st))
                    pbar.update(1)
            else:
                _lib.check(L.dlpm_sampler_steps(h, T - 1, st))
        if pbar:
            pbar.close()
        _lib.check(L.dlpm_sampler_copy_state(h, x.data_ptr(), st))
        if history:
            _lib.check(L.dlpm_sampler_set_history(h, None, st))
        return (x, hist) if history else x

    def _run_callable(self, model, shape, flags, eta, clamp_a, clamp_eps, noise, history, progress,
                      denoised_fn=None, model_kwargs=None):
        """Generic `model(x, t, **model_kwargs)` (any torch callable on the GPU): same kernels, Python between them.
        Also the loop for a `denoised_fn` (a Python function applied to the x_0 prediction, p_mean_variance :162-167)."""
        model_kwargs = model_kwargs or {}
        L, st = _lib.lib(), _lib.stream_ptr()
        d = self.dlpm
        T, B = self.reverse_steps, shape[0]
        D = int(np.prod(shape[1:]))
        dev = torch.device(self.device)
        seed, offset = self._philox_key()
        g, bg, s, bs = (v.to(dev) for v in d.host_schedule)
        host = self.rng == 'reference' or noise is not None
        if host:
            A, xT = self._host_noise_prologue(shape, clamp_a, clamp_eps, noise)
            A, x = A.to(dev), xT.to(dev).reshape(shape).contiguous()
        else:
            # the loop's own tables: dlpm.A / dlpm.Sigmas stay what the caller's step methods hold
            A = d._draw_A(T, shape, clamp_a, seed, offset)
            x = d._draw_state(shape, clamp_eps, d.host_schedule[3][-1], seed, offset)
        c_eps, c_noise = torch.empty_like(A), torch.empty_like(A)
        _lib.check(L.dlpm_coeff_tables_f32(A.data_ptr(), g.data_ptr(), s.data_ptr(), bs.data_ptr(), T, A.shape[1],
                                          c_eps.data_ptr(), c_noise.data_ptr(), None, st))
        tab = dict(g=g, bg=bg, bs=bs, c_eps=c_eps, c_noise=c_noise, A=A)
        t_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        tvec = torch.empty(B, dtype=torch.float32, device=dev)
        isc = self._input_scale()
        isc = None if isc is None else isc.to(dev)
        hist = [x.clone()] if history else []
        need_z = not (flags & _lib.UPD_DLIM) or eta != 0.0
        clip = bool(flags & _lib.UPD_CLIP)
        flags = (flags & ~_lib.UPD_CLIP) | (0 if self.isotropic else _lib.UPD_ELEMENTWISE)
        args = self._update_args(tab, t_dev, B, D, flags, eta, seed, offset)
        pbar = _progress_bar(progress, T)
        for i in range(T - 1, 0, -1):
            t_dev.fill_(i)
            _lib.check(L.dlpm_fill_scaled_t_f32(tvec.data_ptr(), t_dev.data_ptr(), T, B, st))
            xin = x if isc is None else x * isc[i]
            out = model(xin, tvec if self.rescale_timesteps else torch.full((B,), i, device=dev), **model_kwargs)
            eps, clip_flag = self._eps_of_output(out, x, t_dev, tab, clip, denoised_fn, fold_clip=True)
            z = None
            if host and need_z:
                z = (self._streams().randn(shape) if self.rng == 'reference' else torch.randn(shape)).to(dev)
            args.x_dev, args.eps_dev, args.z_dev = x.data_ptr(), eps.data_ptr(), _lib.ptr(z)
            args.flags = flags | clip_flag
            _lib.check(L.dlpm_update_f32(C.byref(args), st))
            if history:
                hist.append(x.clone())
            if pbar:
                pbar.update(1)
        if pbar:
            pbar.close()
        return (x, torch.stack(hist)) if history else x

    def _run_callable_lim(self, model, shape, flags, clamp_eps, history, progress):
        """LIM loop around a generic `model(x, t)` callable: same kernels, Python between them."""
        from .lim import lim_tables
        L, st = _lib.lib(), _lib.stream_ptr()
        steps, B = self.reverse_steps, shape[0]
        T = steps + 1
        D = int(np.prod(shape[1:]))
        dev = torch.device(self.device)
        ode = bool(flags & _lib.UPD_DLIM)
        seed, offset = self._philox_key()
        ts, tmp, cx, cs, cn = (v.to(dev) for v in lim_tables(self.sde, steps, ode))
        host = self.rng == 'reference'
        gauss = self.alpha == 2.0
        A = None
        if host:
            _, x0 = self._host_noise_prologue_lim(shape, clamp_eps)
            x = x0.to(dev)
            if not (ode or gauss):
                A = torch.stack([self._streams().skewed_levy(self.alpha, B, None) for _ in range(steps)]).contiguous().to(dev)
        else:
            x = self.dlpm._draw_state(shape, clamp_eps, 1.0, seed, offset)
            if not (ode or gauss):
                A = self.dlpm._draw_A(steps, shape, None, seed, offset)      # (unclamped; LIM is isotropic: [steps,B])
        t_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        a = _lib.LimUpdateArgs()
        a.t_dev, a.tmp_dev, a.cx_dev, a.cs_dev, a.cn_dev = t_dev.data_ptr(), tmp.data_ptr(), cx.data_ptr(), cs.data_ptr(), cn.data_ptr()
        a.A_dev = A.data_ptr() if A is not None else None
        a.B, a.D, a.T, a.flags, a.clamp_eps = B, D, T, (_lib.UPD_DLIM if ode else 0), clamp_arg(clamp_eps)
        a.seed, a.sample_offset = seed, offset
        hist = [x.clone()] if history else []
        pbar = _progress_bar(progress, steps)
        for i in range(steps):
            t_dev.fill_(T - 1 - i)
            eps = model(x, torch.ones(B, device=dev) * ts[i]).contiguous().float()      # sampler.py:233
            z = self._streams().randn(shape).to(dev) if (host and not ode) else None
            a.x_dev, a.eps_dev, a.z_dev = x.data_ptr(), eps.data_ptr(), z.data_ptr() if z is not None else None
            _lib.check(L.dlpm_lim_update_f32(C.byref(a), st))
            if history:
                hist.append(x.clone())
            if pbar:
                pbar.update(1)
        if pbar:
            pbar.close()
        return (x, torch.stack(hist)) if history else x

    def _loop(self, model, shape, flags, eta, noise, denoised_fn, model_kwargs, history, progress):
        if hasattr(model, 'eval'):
            model.eval()
        clamp_a = self.dlpm.gen_a.kwargs.get('clamp_a')
        clamp_eps = self.dlpm.gen_eps.kwargs.get('clamp_eps')
        with torch.inference_mode():
            if self._takes_native(model, model_kwargs, denoised_fn):
                out = self._run_native(model, list(shape), flags, eta, clamp_a, clamp_eps, noise, history, progress,
                                       labels=(model_kwargs or {}).get('y'))
            else:
                out = self._run_callable(model, list(shape), flags, eta, clamp_a, clamp_eps, noise, history, progress,
                                         denoised_fn=denoised_fn, model_kwargs=model_kwargs)
        self._advance_key(shape[0])
        return out

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=False, denoised_fn=None, model_kwargs=None, progress=False,
                      get_sample_history=False):
        """GenerativeLevyProcess.p_sample_loop (:241-289): the stochastic loop with the arguments `sample()` does not pass on --
        `noise` (x_T), `denoised_fn`, `model_kwargs`.  Clamps are the generators' current ones (set by the last sample())."""
        assert self.device is not None
        assert isinstance(shape, (tuple, list))
        return self._loop(model, shape, _lib.UPD_CLIP if clip_denoised else 0, 0.0, noise, denoised_fn, model_kwargs,
                          get_sample_history, progress)

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=False, denoised_fn=None, model_kwargs=None, progress=False,
                         eta=0.0, get_sample_history=False):
        """GenerativeLevyProcess.ddim_sample_loop (:364-403): the DLIM loop."""
        assert self.device is not None
        assert isinstance(shape, (tuple, list))
        return self._loop(model, shape, _lib.UPD_DLIM | (_lib.UPD_CLIP if clip_denoised else 0), eta, noise, denoised_fn,
                          model_kwargs, get_sample_history, progress)

    # -------------------------------------------------------------------------------- one step at a time
    def _eps_of_output(self, out, x, t_dev, tab, clip, denoised_fn, fold_clip):
        """What p_mean_variance does to the model's output (GenerativeLevyProcess.py:182-207), for the loop of _run_callable and
        the step methods alike: EPSILON without clipping bypasses everything (a denoised_fn is then never called, as in the
        reference); `fold_clip` leaves "EPSILON + clip, no denoised_fn" to the update kernel's own flag; every other case goes
        model output -> x_0 -> [denoised_fn] -> [clamp] -> eps through dlpm_predict_f32.  `tab`: the trajectory's tables (see
        _tables).  Returns (eps, UPD_CLIP where the update kernel still has to clip, else 0)."""
        eps = out.contiguous().float()
        mean_type = _lib.MEAN_TYPES[self.model_mean_type]
        predict = (mean_type != 0) or (clip and (denoised_fn is not None or not fold_clip))
        if not predict:
            return eps, (_lib.UPD_CLIP if clip else 0)
        if eps.data_ptr() == x.data_ptr():          # a model that returns its input: the conversion below writes in place
            eps = eps.clone()
        L, st = _lib.lib(), _lib.stream_ptr()
        pa = _lib.PredictArgs()
        pa.t_dev, pa.g_dev, pa.bg_dev, pa.bs_dev = t_dev.data_ptr(), _lib.ptr(tab['g']), _lib.ptr(tab['bg']), _lib.ptr(tab['bs'])
        pa.c_eps_dev, pa.A_dev = tab['c_eps'].data_ptr(), tab['A'].data_ptr()
        pa.B, pa.D, pa.T, pa.mean_type = x.shape[0], x[0].numel(), self.reverse_steps, mean_type
        el = _lib.PRED_ELEMENTWISE if not self.isotropic else 0
        tail = (_lib.PRED_CLIP if clip else 0) | _lib.PRED_TO_EPS | el
        pa.x_dev, pa.in_dev, pa.out_dev = x.data_ptr(), eps.data_ptr(), eps.data_ptr()
        if denoised_fn is None:
            pa.flags = _lib.PRED_TO_XSTART | tail
            _lib.check(L.dlpm_predict_f32(C.byref(pa), st))
        else:
            pa.flags = _lib.PRED_TO_XSTART | el
            _lib.check(L.dlpm_predict_f32(C.byref(pa), st))
            eps = denoised_fn(eps.view(x.shape)).contiguous().float()
            pa.in_dev, pa.out_dev, pa.flags = eps.data_ptr(), eps.data_ptr(), tail
            _lib.check(L.dlpm_predict_f32(C.byref(pa), st))
        return eps, 0

    def _update_args(self, tab, t_dev, B, D, flags, eta, seed, offset):
        """dlpm_update_args of one trajectory (tables `tab`, Philox key); the caller sets x_dev / eps_dev / z_dev per step."""
        a = _lib.UpdateArgs()
        a.t_dev, a.g_dev, a.bg_dev, a.bs_dev = t_dev.data_ptr(), _lib.ptr(tab['g']), _lib.ptr(tab['bg']), _lib.ptr(tab['bs'])
        a.c_eps_dev, a.c_noise_dev, a.A_dev = tab['c_eps'].data_ptr(), tab['c_noise'].data_ptr(), tab['A'].data_ptr()
        a.B, a.D, a.T, a.flags, a.dlim_eta, a.alpha = B, D, self.reverse_steps, flags, float(eta), float(self.alpha)
        a.seed, a.sample_offset = seed, offset
        return a

    def _tables(self):
        """The tables the step methods read: the process's schedule and the A / coefficient tables of its current trajectory."""
        d = self.dlpm
        return dict(g=d.gammas, bg=d.bargammas, bs=d.barsigmas, c_eps=d._c_eps, c_noise=d._c_noise, A=d._A)

    def _step_eps(self, model, x, t, clip, denoised_fn, model_kwargs, fold_clip):
        """The model call of a step method and the eps of its output (_eps_of_output) on the process's own tables.  Returns (x as
        contiguous fp32, eps, the int32 [1] device timestep, update flags)."""
        d = self.dlpm
        if not (torch.is_tensor(x) and x.is_cuda):
            raise _lib.DlpmError('the step methods run on the MI355X only (x is on {}); there is no CPU fallback'.format(
                x.device if torch.is_tensor(x) else type(x).__name__))
        B = x.shape[0]
        assert torch.is_tensor(t) and t.shape == (B,), 't must be a [B] tensor'
        _, D, n = d._cols(x.shape)
        T = self.reverse_steps
        if d._Sigmas is None or tuple(d._Sigmas.shape) != (T, n) or d._table_shape != tuple(x.shape):
            raise _lib.DlpmError('the step methods need the tables of a trajectory of shape {}: iterate p_sample_loop_progressive / '
                                 'ddim_sample_loop_progressive, or call dlpm.sample_A(shape, reverse_steps) and '
                                 'dlpm.compute_Sigmas()'.format(tuple(x.shape)))
        x = x.contiguous().float()
        t = t.to(x.device)
        t_dev = d._t_scalar(x, t)
        isc = self._input_scale_dev()
        xin = x if isc is None else x * isc[t.long()].view(-1, *([1] * (x.dim() - 1)))
        out = model(xin, self._scale_timesteps(t), **(model_kwargs or {}))
        assert out.shape == x.shape, 'the model returned {}, expected {}'.format(tuple(out.shape), tuple(x.shape))
        eps, clip_flag = self._eps_of_output(out, x, t_dev, self._tables(), clip, denoised_fn, fold_clip)
        return x, eps, t_dev, clip_flag | (0 if self.isotropic else _lib.UPD_ELEMENTWISE)

    def p_mean_variance(self, model, x, t, clip_denoised=False, denoised_fn=None, model_kwargs=None):
        """GenerativeLevyProcess.p_mean_variance (:154-219): {'eps', 'mean', 'variance'} of p(x_{t-1} | x_t).  The model is called
        with the scaled timesteps (and the input scaling of a scale_exploding process), its output becomes the eps of the step
        formulas per model_mean_type / clip_denoised / denoised_fn (dlpm_predict_f32), and the moments come from
        dlpm_anterior_f32 on the process's Sigmas -- the tables of the trajectory a progressive loop began, or of the caller's
        own dlpm.sample_A / compute_Sigmas.  `t`: a [B] tensor; the step formulas use its first entry, as the reference does
        (t[0], :210).  'variance' is a stride-0 view of [B] when the noise is isotropic.  No host read."""
        with torch.no_grad():
            x, eps, _, _ = self._step_eps(model, x, t, clip_denoised, denoised_fn, model_kwargs, fold_clip=False)
            mean, var = self.dlpm.anterior_mean_variance_dlpm(x, t, eps)
        return {'eps': eps, 'mean': mean, 'variance': var}

    def _step(self, model, x, t, clip, denoised_fn, model_kwargs, dlim, eta, noise):
        """One reverse step as the loops take it: the eps of _step_eps, then ONE dlpm_update_f32 on a copy of x."""
        with torch.no_grad():
            x, eps, t_dev, flags = self._step_eps(model, x, t, clip, denoised_fn, model_kwargs, fold_clip=True)
            need_z = (not dlim) or eta != 0.0
            z = None
            if noise is not None:
                z = noise.to(x.device, torch.float32).contiguous()
                assert z.shape == x.shape, 'noise must have the shape of x'
            elif need_z and self.rng == 'reference':
                z = self._streams().randn(x.shape).to(x.device)
            seed, offset = self._traj if self._traj is not None else self._philox_key()
            out = x.clone()
            a = self._update_args(self._tables(), t_dev, x.shape[0], x[0].numel(), flags | (_lib.UPD_DLIM if dlim else 0), eta,
                                  seed, offset)
            a.x_dev, a.eps_dev, a.z_dev = out.data_ptr(), eps.data_ptr(), _lib.ptr(z)
            _lib.check(_lib.lib().dlpm_update_f32(C.byref(a), _lib.stream_ptr()))
        return {'sample': out}

    def p_sample(self, model, x, t, clip_denoised=False, denoised_fn=None, model_kwargs=None, noise=None):
        """GenerativeLevyProcess.p_sample (:225-239): {'sample': x_{t-1}} = mean + 1[t != 1] sqrt(variance) z, one dlpm_update_f32
        on a copy of x (x itself is left as it is).  z: `noise=` as given (this build's addition); else, rng='philox', the
        sampler's own counters -- (key of the current trajectory, global sample, step t, element), the key being the one the last
        progressive loop took, or the next sample() call's when none has begun -- so a hand-written loop over p_sample draws what
        p_sample_loop draws; rng='reference': the next randn of the reference's torch stream."""
        return self._step(model, x, t, clip_denoised, denoised_fn, model_kwargs, False, 0.0, noise)

    def ddim_sample(self, model, x, t, clip_denoised=False, denoised_fn=None, model_kwargs=None, eta=0.0, noise=None):
        """GenerativeLevyProcess.ddim_sample (:332-363): the DLIM step, deterministic at eta = 0 (no z is drawn); z as p_sample."""
        return self._step(model, x, t, clip_denoised, denoised_fn, model_kwargs, True, eta, noise)

    def q_posterior_mean_variance(self, x_start, x_t, t, Sigmas):
        """(mean, variance) of q(x_{t-1} | x_t, x_0, a_{1:T}) from a caller-given Sigmas table ([T,B] or [T, *shape]).  The
        reference's method (:118-133) raises AttributeError: it calls dlpm.anterior_mean_dlpm / anterior_variance_dlpm, which do
        not exist there.  Its evident meaning is built here: eps = predict_eps(x_t, t, x_start), then the DLPM moments of
        anterior_mean_variance_dlpm on the given Sigmas instead of the process's own."""
        assert x_start.shape == x_t.shape
        eps = self.dlpm.predict_eps(x_t, t, x_start)
        mean, var = self.dlpm.anterior_mean_variance_dlpm(x_t, t, eps, Sigmas=Sigmas)
        assert mean.shape[0] == var.shape[0] == x_start.shape[0]
        return mean, var

    def _progressive(self, model, shape, flags, eta, noise, clip, denoised_fn, model_kwargs):
        """The generator behind both progressive loops.  Prologue (at the first next()): take the Philox key of this trajectory,
        keep it for the step methods, advance the call counter (or the dataset stream) at once -- a generator dropped half way
        has still used its key -- fill dlpm.A / dlpm.Sigmas, draw x_T.  Then one fresh tensor per step.

        A native net (UNetModel / MLPModel) with isotropic noise, device draws and no denoised_fn runs on the graph sampler: one
        replay and one device copy per yield.  Everything else is the loop over p_sample / ddim_sample."""
        assert self.device is not None
        assert isinstance(shape, (tuple, list))
        shape = [int(v) for v in shape]
        if hasattr(model, 'eval'):
            model.eval()
        d = self.dlpm
        T, dev = self.reverse_steps, torch.device(self.device)
        if dev.type != 'cuda':
            raise _lib.DlpmError('the progressive loops run on the MI355X only (device is {}); there is no CPU fallback'.format(dev))
        clamp_a, clamp_eps = d.gen_a.kwargs.get('clamp_a'), d.gen_eps.kwargs.get('clamp_eps')
        dlim = bool(flags & _lib.UPD_DLIM)
        native = self._takes_native(model, model_kwargs, denoised_fn) and self.isotropic and self.rng == 'philox' and noise is None
        seed, offset = self._philox_key()
        self._traj = (seed, offset)
        self._advance_key(shape[0])
        L, st = _lib.lib(), _lib.stream_ptr()
        if self.rng == 'reference' or noise is not None:
            with torch.no_grad():
                A, xT = self._host_noise_prologue(shape, clamp_a, clamp_eps, noise)
            d.sample_A(shape, T, A=A.to(dev))
            x = xT.to(dev).reshape(shape).contiguous().clone()
        else:
            d.sample_A(shape, T, seed=seed, sample_offset=offset)
            x = None
        d.compute_Sigmas()
        if native:
            labels = (model_kwargs or {}).get('y')
            if getattr(model, 'num_classes', None) is not None:
                labels = model._check_labels(shape[0], labels)
            h = self._native_sampler(model, shape, flags | (_lib.UPD_CLIP if clip else 0), eta, clamp_a, clamp_eps, seed, offset)
            me = self._native_owner = object()
            if labels is not None:
                y_d = labels.to(dev, torch.int64).contiguous()
                _lib.check(L.dlpm_sampler_set_labels(h, y_d.data_ptr(), st))
            _lib.check(L.dlpm_sampler_set_history(h, None, st))
            _lib.check(L.dlpm_sampler_begin(h, st))
            for i in range(T):
                if self._native_owner is not me:
                    raise _lib.DlpmError('another loop ran on this method object since this progressive generator began; its '
                                         'sampler state is gone')
                st = _lib.stream_ptr()
                if i:
                    _lib.check(L.dlpm_sampler_steps(h, 1, st))
                x = torch.empty(shape, dtype=torch.float32, device=dev)
                _lib.check(L.dlpm_sampler_copy_state(h, x.data_ptr(), st))
                yield {'sample': x}
            return
        if x is None:
            x = d._draw_state(shape, clamp_eps, d.host_schedule[3][-1], seed, offset)
        yield {'sample': x}
        for i in range(T - 1, 0, -1):
            t = torch.full((shape[0],), i, dtype=torch.int64, device=dev)
            out = self._step(model, x, t, clip, denoised_fn, model_kwargs, dlim, eta, None)
            yield out
            x = out['sample']

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=False, denoised_fn=None, model_kwargs=None):
        """GenerativeLevyProcess.p_sample_loop_progressive (:291-330): a generator over {'sample': x} dicts, x_T first, then one
        per reverse step (reverse_steps dicts in all); every yielded tensor is fresh.  The trajectory's key and tables are taken
        when the first item is asked for, and the step methods (p_sample, ddim_sample, p_mean_variance) use them from then on, so
        a caller may leave the generator at any step and go on by hand.  One native progressive loop per method object at a time."""
        return self._progressive(model, shape, 0, 0.0, noise, clip_denoised, denoised_fn, model_kwargs)

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=False, denoised_fn=None, model_kwargs=None,
                                     eta=0.0):
        """GenerativeLevyProcess.ddim_sample_loop_progressive (:412-452): the DLIM loop as a generator; see
        p_sample_loop_progressive."""
        return self._progressive(model, shape, _lib.UPD_DLIM, eta, noise, clip_denoised, denoised_fn, model_kwargs)

    def _lim_run(self, model, shape, ode, history, progress, clamp_eps):
        """The LIM sampler on a native net (graph sampler) or a generic callable; `ode` selects the deterministic update."""
        from .unet import UNetModel
        from .mlp import MLPModel
        flags = _lib.SMP_LIM | (_lib.UPD_DLIM if ode else 0)
        if isinstance(model, (UNetModel, MLPModel)) and self.rescale_timesteps:
            return self._run_native(model, shape, flags, 0.0, None, clamp_eps, None, history, progress)
        return self._run_callable_lim(model, shape, flags, clamp_eps, history, progress)

    def lim_sample(self, model, shape, ddim=False, get_sample_history=False, clip_denoised=False):
        """GenerativeLevyProcess.lim_sample (:454-506): the LIM sampler by its own name, what sample() runs for a method built
        with LIM=True; `ddim` selects the ODE, `clip_denoised` is accepted and ignored as in the reference.  x_0 is gen_eps's
        noise under its current clamp_eps."""
        assert self.LIM, 'lim_sample belongs to a method built with LIM=True'
        if getattr(model, 'num_classes', None) is not None:
            raise NotImplementedError('the LIM sampler does not take model_kwargs / class labels')
        if hasattr(model, 'eval'):
            model.eval()
        with torch.inference_mode():
            out = self._lim_run(model, list(shape), ddim, get_sample_history, False, self.dlpm.gen_eps.kwargs.get('clamp_eps'))
        self._advance_key(shape[0])
        return out

    # -------------------------------------------------------------------------------- BEM: SAMPLING
    def sample(self, models, shape, reverse_steps, time_spacing=None, initial_data=None, clip_denoised=False,
               deterministic=False, dlim_eta=1.0, print_progression=False, get_sample_history=False, clamp_a=None,
               clamp_eps=None, model_kwargs=None):
        """GenerativeLevyProcess.sample: dlpm/methods/GenerativeLevyProcess.py:512-569.  `model_kwargs` (this build's addition, passed on
        to the model as the reference's loops do, :601): {'y': labels} for a class-conditional UNetModel."""
        self.dlpm.gen_a.setParams(clamp_a=clamp_a)          # stateful, as in the reference (:526-527)
        self.dlpm.gen_eps.setParams(clamp_eps=clamp_eps)
        model = models['default']
        assert time_spacing is None, 'Specific time spacing is not yet supported for diffusion reverse sampling'
        if self.reverse_steps != reverse_steps:
            assert self.rescale_timesteps, 'Rescaling only works when rescale_timesteps is True'
            self.dlpm.rescale_diffusion(reverse_steps, time_spacing=time_spacing)
            self.reverse_steps = reverse_steps            # (the reference never restores it: SURVEY.md 3.4)
        if hasattr(model, 'eval'):
            model.eval()
        shape_arg = list(shape)
        shape = list(initial_data.shape) if (deterministic and initial_data is not None) else list(shape)
        noise = initial_data if deterministic else None
        flags = (_lib.UPD_DLIM if deterministic else 0) | (_lib.UPD_CLIP if clip_denoised else 0)
        eta = dlim_eta if deterministic else 0.0
        native = self._takes_native(model, model_kwargs)
        labels = (model_kwargs or {}).get('y')
        with torch.inference_mode():
            if self.LIM and (model_kwargs or getattr(model, 'num_classes', None) is not None):
                raise NotImplementedError('the LIM sampler does not take model_kwargs / class labels')
            if self.LIM:
                # lim_sample (GenerativeLevyProcess.py:454-507): `deterministic` selects the ODE; clip_denoised and
                # initial_data are accepted and ignored, as in the reference
                shape = shape_arg
                out = self._lim_run(model, shape, deterministic, get_sample_history, print_progression, clamp_eps)
            elif native:
                out = self._run_native(model, shape, flags, eta, clamp_a, clamp_eps, noise, get_sample_history, print_progression,
                                       labels=labels)
            else:
                out = self._run_callable(model, shape, flags, eta, clamp_a, clamp_eps, noise, get_sample_history, print_progression,
                                         model_kwargs=model_kwargs)
        self._advance_key(shape[0])
        return out

    # -------------------------------------------------------------------------------- BEM: held-out loss
    def q_sample(self, x_start, t, eps=None):
        """GenerativeLevyProcess.q_sample (:105-116): (x_t, eps) from q(x_t | x_0)."""
        return self.dlpm.sample_x_t_from_xstart(x_start, t, eps)

    def _input_scale_dev(self):
        """_input_scale() on the device, uploaded once per schedule (the loss kernels index it per sample)."""
        isc = self._input_scale()
        if isc is None:
            return None
        key = self.dlpm.host_schedule[3].data_ptr()
        if getattr(self, '_isc_dev', None) is None or self._isc_dev[0] != key:
            self._isc_dev = (key, isc.to(self.device))
        return self._isc_dev[1]

    def _loss_host_draws(self, shape, outer, inner, clamp_a):
        """rng='reference': (t, a, z) on the host in the reference's order (GenerativeLevyProcess.py:634,650,652) -- `randint(1, T,
        [B])` and `randn` on a private torch.Generator seeded like the torch stream (ReferenceStreams.G: torch's own generator, so t
        and z equal the reference's bit for bit), `outer * B` (non-isotropic: `outer * B * D`) skewed-Levy draws on the restated
        numpy stream."""
        st = self._streams()
        B, D = shape[0], int(np.prod(shape[1:]))
        t = torch.randint(1, self.reverse_steps, size=[B], generator=st.G)
        a = st.skewed_levy(self.alpha, outer * B * (1 if self.isotropic else D), clamp_a)
        z = torch.randn([outer * inner * B] + list(shape[1:]), generator=st.G)
        return {'t': t, 'a': a, 'z': z}

    def _loss_terms(self, model, x_start, lploss, outer, inner, model_kwargs, clamp_a, noise, out=None, out_stride=None,
                    out_offset=0, t_out=None, keep=False):
        """The launches before the estimator: k_loss_elements, the net on the extended batch, k_loss_terms.  Terms go to
        `out[r * out_stride + out_offset + b]` (default: a fresh [outer * inner * B] buffer, the reference's layout).  Returns a dict
        with 'losses', 't' (int32 [B]) and, with `keep`, 'x_t', 'eps_t', 'x_in', 'model_eps', 'tvec' (the times the net was given).  No synchronisation, no host read."""
        from .unet import UNetModel
        from .mlp import MLPModel
        L, st = _lib.lib(), _lib.stream_ptr()
        dev = x_start.device
        shape = list(x_start.shape)
        B, D, R = shape[0], int(np.prod(shape[1:])), outer * inner
        T = self.reverse_steps
        x0 = x_start.contiguous().float()
        if noise is None and self.rng == 'reference':
            noise = self._loss_host_draws(shape, outer, inner, clamp_a)
        noise = dict(noise or {})
        assert set(noise) <= {'t', 'a', 'z'}, 'noise takes the keys t, a, z; got {}'.format(sorted(noise))
        t_in = a_in = z_in = None
        if noise.get('t') is not None:
            t_in = torch.as_tensor(noise['t']).to(dev, torch.int32).contiguous()
            assert t_in.shape == (B,), 't must be [B]'
        if noise.get('a') is not None:
            a_in = torch.as_tensor(noise['a']).to(dev, torch.float32).reshape(outer * B, -1)
            if self.isotropic:
                a_in = a_in[:, 0]               # as drawn [outer * B], or the reference's expanded [outer * B, C, H, W]
            else:
                assert a_in.shape[1] == D, 'non-isotropic a must be [outer * B, D]'
            a_in = a_in.contiguous()
        if noise.get('z') is not None:
            z_in = torch.as_tensor(noise['z']).to(dev, torch.float32).contiguous()
            assert z_in.numel() == R * B * D, 'z must be [outer * inner * B, ...]'
        ext = [R * B] + shape[1:]
        x_in = torch.empty(ext, dtype=torch.float32, device=dev)
        eps_t = torch.empty(ext, dtype=torch.float32, device=dev)
        x_t = torch.empty(ext, dtype=torch.float32, device=dev) if keep else None
        tvec = torch.empty(R * B, dtype=torch.float32, device=dev)
        if t_out is None:
            t_out = torch.empty(B, dtype=torch.int32, device=dev)
        isc = self._input_scale_dev()
        seed, offset = self._philox_key()
        a = _lib.LossArgs()
        a.x0_dev, a.t_dev, a.a_dev, a.z_dev = x0.data_ptr(), _lib.ptr(t_in), _lib.ptr(a_in), _lib.ptr(z_in)
        a.bg_dev, a.bs_dev, a.in_scale_dev = _lib.ptr(self.dlpm.bargammas), _lib.ptr(self.dlpm.barsigmas), _lib.ptr(isc)
        a.x_in_dev, a.eps_dev, a.x_t_dev = x_in.data_ptr(), eps_t.data_ptr(), _lib.ptr(x_t)
        a.tvec_out_dev, a.t_out_dev, a.a_out_dev = tvec.data_ptr(), t_out.data_ptr(), None
        a.B, a.D, a.T, a.outer, a.inner = B, D, T, outer, inner
        a.flags = (_lib.LOSS_RESCALE_T if self.rescale_timesteps else 0) | (0 if self.isotropic else _lib.LOSS_ELEMENTWISE)
        a.alpha, a.clamp_a = float(self.alpha), clamp_arg(clamp_a)
        a.seed, a.sample_offset = seed, offset
        _lib.check(L.dlpm_loss_elements_f32(C.byref(a), st))

        kw = dict(model_kwargs or {})
        y = kw.get('y')
        if y is not None and R > 1 and torch.is_tensor(y) and y.shape[:1] == (B,):
            kw['y'] = y = y.to(dev).repeat(R, *([1] * (y.dim() - 1)))       # replica r of sample b carries label y[b]
        if isinstance(model, UNetModel) and set(kw) <= {'y'}:
            model_eps = model._forward_checked(x_in, tvec, y)
        elif isinstance(model, MLPModel) and not kw:
            model_eps = model(x_in, tvec)
        else:
            t_arg = tvec if self.rescale_timesteps else t_out.to(torch.int64).repeat(R)
            model_eps = model(x_in, t_arg, **kw).contiguous().float()
        assert model_eps.shape == x_in.shape, 'the model returned {}, expected {}'.format(tuple(model_eps.shape), tuple(x_in.shape))

        if out is None:
            out, out_stride = torch.empty(R * B, dtype=torch.float32, device=dev), B
        _lib.check(L.dlpm_loss_terms_f32(model_eps.data_ptr(), eps_t.data_ptr(), out.data_ptr(), B, R, D, int(lploss), out_stride,
                                         out_offset, st))
        self._advance_key(B)
        res = {'losses': out, 't': t_out}
        if keep:
            res.update(x_t=x_t, eps_t=eps_t, x_in=x_in, model_eps=model_eps, tvec=tvec)
        return res

    def _loss_reduce(self, terms, N, outer, inner, loss_monte_carlo, check_finite, median_index=None, flag=None):
        """k_loss_reduce on terms[outer * inner * N] -> 0-dim fp32 loss on the device; `check_finite` reads the 4-byte flag
        (`flag`: an int32 [1] device tensor of the caller's to receive it instead of a fresh one)."""
        res = torch.empty(1, dtype=torch.float32, device=terms.device)
        if flag is None:
            flag = torch.empty(1, dtype=torch.int32, device=terms.device)
        _lib.check(_lib.lib().dlpm_loss_reduce_f32(terms.data_ptr(), N, outer, inner, int(loss_monte_carlo == 'median'),
                                                   res.data_ptr(), flag.data_ptr(), _lib.ptr(median_index), _lib.stream_ptr()))
        if check_finite:
            assert int(flag) == 0, 'Nan in losses'                         # GenerativeLevyProcess.py:667
        return res[0]

    def _loss_check_args(self, model, x_start, loss_type, lploss, loss_monte_carlo, outer, inner, model_kwargs):
        """Every argument check of training_losses_dlpm, before any device work.  Returns (lploss as int, model_kwargs)."""
        from .unet import UNetModel
        from .mlp import MLPModel
        assert self.model_mean_type == ModelMeanType.EPSILON, 'only epsilon model output is supported for the moment'
        assert loss_type == LossType.EPS_LOSS, 'only epsilon loss is supported for the moment'
        if lploss not in (2, 1, -1):
            # the reference's general-p branch (torch.linalg.norm over three dims) raises on image tensors and is not reproduced
            raise ValueError('lploss must be 2, 1 or -1 (L2, smooth-L1, squared L2), got {}'.format(lploss))
        assert loss_monte_carlo in ('mean', 'median'), "loss_monte_carlo must be 'mean' or 'median'"
        outer, inner = int(outer), int(inner)
        assert outer >= 1 and inner >= 1, 'monte_carlo_outer and monte_carlo_inner must be >= 1'
        if loss_monte_carlo == 'median' and outer > 64:
            raise ValueError('median of means takes monte_carlo_outer <= 64, got {}'.format(outer))
        model_kwargs = dict(model_kwargs or {})
        if set(model_kwargs) == {'model_kwargs'}:          # the nested form a reference caller has to write (:608)
            model_kwargs = dict(model_kwargs['model_kwargs'] or {})
        assert torch.is_tensor(x_start) and x_start.dim() >= 2 and x_start.shape[0] >= 1, 'x_start must be a [B, ...] tensor'
        if isinstance(model, UNetModel):
            y = model_kwargs.get('y')
            if set(model_kwargs) <= {'y'}:
                model._check_labels(x_start.shape[0], y)    # the reference's checks, once, on the [B] labels
        elif isinstance(model, MLPModel):
            assert x_start.dim() == 3 and tuple(x_start.shape[1:]) == (1, model.nfeatures), x_start.shape
        if not x_start.is_cuda:
            raise _lib.DlpmError('training_losses runs on the MI355X only (x_start is on {}); there is no CPU fallback'.format(
                x_start.device))
        return int(lploss), model_kwargs

    def training_losses_dlpm(self, model, x_start, loss_type='EPS_LOSS', lploss=2.0, loss_monte_carlo='mean', monte_carlo_outer=1,
                             monte_carlo_inner=1, model_kwargs=None, clamp_a=None, clamp_eps=None, noise=None, check_finite=True,
                             return_terms=False):
        """Forward-only, under torch.inference_mode(): the result carries no autograd graph -- this is the Proposition-9 loss
        (GenerativeLevyProcess.training_losses_dlpm, :612-677) as an evaluation metric, not a training step.

        Three kernels of libdlpm_amd around one forward of the net on the `outer * inner * B` extended batch; nothing is
        synchronised and no host value is read unless `check_finite` (one 4-byte flag, the reference's `Nan in losses`
        assertion).  `loss_type` defaults to 'EPS_LOSS' (the reference's own default 'EPSILON' fails its own assertion).
        `noise={'t': [B], 'a': [outer*B] (non-isotropic [outer*B, D]), 'z': [outer*inner*B, ...]}` injects any of the draws;
        what is not injected comes from the device Philox stream (rng='philox': key as sample(), so dataset_stream() and
        sample_offset mean the same here) or, with rng='reference', all three from the reference's CPU streams
        (_loss_host_draws).  The index quirk of the reference is kept: replica r reads a[(r mod outer) * B + b], while the
        median estimator reads the terms as [outer, inner, B].  Returns the 0-dim fp32 loss on the device (with
        `return_terms`: (loss, terms[outer*inner*B], t[B]))."""
        lploss, model_kwargs = self._loss_check_args(model, x_start, loss_type, lploss, loss_monte_carlo, monte_carlo_outer,
                                                     monte_carlo_inner, model_kwargs)
        outer, inner = int(monte_carlo_outer), int(monte_carlo_inner)
        self.dlpm.gen_a.setParams(clamp_a=clamp_a)          # stateful, as in the reference (:629-630)
        self.dlpm.gen_eps.setParams(clamp_eps=clamp_eps)
        if hasattr(model, 'eval'):
            model.eval()
        if _wants_graph(model) and not model_kwargs:
            # a differentiable MLPModel under grad mode: the same launches with a graph behind the loss.  No host read here
            # (`check_finite` is not consulted): a non-finite loss shows in the caller's own loss.item()
            spec = dict(lim=False, lploss=lploss, outer=outer, inner=inner, clamp_a=clamp_a, noise=noise, median=loss_monte_carlo == 'median')
            loss, terms, t = _TrainingLoss.apply(self, model, spec, x_start, *model.parameters())
            return (loss, terms, t) if return_terms else loss
        with torch.inference_mode():
            r = self._loss_terms(model, x_start, lploss, outer, inner, model_kwargs, clamp_a, noise)
            loss = self._loss_reduce(r['losses'], x_start.shape[0], outer, inner, loss_monte_carlo, check_finite)
        return (loss, r['losses'], r['t']) if return_terms else loss

    # -------------------------------------------------------------------------------- BEM: held-out loss, LIM
    def _lim_loss_host_draws(self, shape, clamp_eps):
        """rng='reference': the draws of training_losses_lim on the host in the reference's order (GenerativeLevyProcess.py:691-705,
        Distributions.py:57-73).  alpha != 2: B unclamped skewed-Levy draws on the restated numpy stream, `randn(shape)` then
        `rand(B)` on ReferenceStreams.G, e = clamp(sqrt(a) z) in fp32 (the root correctly rounded, the product and the clamp torch's);
        alpha = 2: `randn`, then `rand`.  Returns
        {'t', 'e', 'a' (None at alpha = 2), 'z'} on the CPU."""
        st = self._streams()
        B = shape[0]
        if self.alpha == 2.0:
            a, z = None, torch.randn(list(shape), generator=st.G)
            e = z
        else:
            a = st.skewed_levy(self.alpha, B, None)
            z = torch.randn(list(shape), generator=st.G)
            # sqrt(a) as the correctly rounded fp32 root (the fp64 one rounded once: 53 >= 2 * 24 + 2 bits).  torch.sqrt on a CPU is
            # within 1 ulp of it but not the same value on every host (0.7 % of 2^20 inputs differ from the IEEE root on the host that
            # recorded F22, 19 % on an MI355X host), and the reference's recorded e is the product with the IEEE root in every F22 case
            root = torch.from_numpy(np.sqrt(a.numpy().astype(np.float64)).astype(np.float32))
            e = root.view(-1, *([1] * (len(shape) - 1))) * z
            if clamp_eps is not None:
                e = torch.clamp(e, -clamp_eps, clamp_eps)
        t = torch.rand(B, generator=st.G) * (self.sde.T - 1e-5) + 1e-5
        return {'t': t, 'e': e, 'a': a, 'z': z}

    def _lim_check_args(self, model, x_start, y=None, noise=None):
        """Every argument check of training_losses_lim that needs no device.  Returns the injected draws as a dict of contiguous
        fp32 tensors (on whatever device the caller left them)."""
        from .mlp import MLPModel
        assert self.LIM, 'training_losses_lim belongs to a method built with LIM=True'
        if y is not None or getattr(model, 'num_classes', None) is not None:
            raise NotImplementedError('training_losses_lim takes unconditional nets only: the reference hard-wires y = None '
                                      '(dlpm/methods/GenerativeLevyProcess.py:706)')
        assert torch.is_tensor(x_start) and x_start.dim() >= 2 and x_start.shape[0] >= 1, 'x_start must be a [B, ...] tensor'
        if isinstance(model, MLPModel):
            assert x_start.dim() == 3 and tuple(x_start.shape[1:]) == (1, model.nfeatures), x_start.shape
        noise = dict(noise or {})
        keys = {'t', 'e', 'x_coeff', 'sigma'}
        assert set(noise) <= keys, 'noise takes the keys {}; got {}'.format(sorted(keys), sorted(noise))
        noise = {k: torch.as_tensor(v).to(torch.float32).contiguous() for k, v in noise.items() if v is not None}
        if ('x_coeff' in noise) != ('sigma' in noise):
            raise ValueError('noise: x_coeff and sigma are given together or not at all')
        B = x_start.shape[0]
        for k in ('t', 'x_coeff', 'sigma'):
            assert k not in noise or tuple(noise[k].shape) == (B,), '{} must be [B] = [{}], got {}'.format(k, B, tuple(noise[k].shape))
        assert 'e' not in noise or noise['e'].shape == x_start.shape, 'e must have the shape of x_start {}, got {}'.format(
            tuple(x_start.shape), tuple(noise['e'].shape))
        return noise

    def _lim_loss_terms(self, model, x_start, clamp_eps, noise, out=None, out_offset=0, t_out=None, keep=False):
        """The launches before the estimator: k_lim_loss_elements, the net, k_loss_terms (smooth-L1).  `noise`: the dict
        _lim_check_args returned.  Terms go to `out[out_offset + b]` (default: a fresh [B] buffer), the times to `t_out` (default:
        a fresh [B] buffer).  Returns {'losses', 't'} and, with `keep`, 'x_t', 'score', 'e', 'a', 'x_coeff', 'sigma', 'output'.
        No synchronisation and no host read unless rng='reference' (whose draws are made on the host)."""
        from .unet import UNetModel
        from .mlp import MLPModel
        L, st = _lib.lib(), _lib.stream_ptr()
        dev = x_start.device
        shape = list(x_start.shape)
        B, D = shape[0], int(np.prod(shape[1:]))
        x0 = x_start.contiguous().float()
        if not noise and self.rng == 'reference':
            d = self._lim_loss_host_draws(shape, clamp_eps)
            noise = {'t': d['t'], 'e': d['e'].contiguous()}
        if 't' in noise and 'x_coeff' not in noise and not noise['t'].is_cuda:
            # a time known on the host: the reference's own evaluation, torch's fp32 ops on the CPU (loss.py:20-21)
            t_host = noise['t']
            noise = dict(noise, sigma=self.sde.marginal_std(t_host).contiguous(), x_coeff=self.sde.diffusion_coeff(t_host).contiguous())
        inj = {k: v.to(dev) for k, v in noise.items()}
        x_t = torch.empty(shape, dtype=torch.float32, device=dev)
        score = torch.empty(shape, dtype=torch.float32, device=dev)
        if t_out is None:
            t_out = torch.empty(B, dtype=torch.float32, device=dev)
        kept = {}
        if keep:
            kept = dict(e=torch.empty(shape, dtype=torch.float32, device=dev))
            kept.update({k: torch.empty(B, dtype=torch.float32, device=dev) for k in ('a', 'x_coeff', 'sigma')})
        seed, offset = self._philox_key()
        a = _lib.LimLossArgs()
        a.x0_dev, a.t_dev, a.e_dev = x0.data_ptr(), _lib.ptr(inj.get('t')), _lib.ptr(inj.get('e'))
        a.x_coeff_dev, a.sigma_dev = _lib.ptr(inj.get('x_coeff')), _lib.ptr(inj.get('sigma'))
        a.x_t_dev, a.score_dev, a.tvec_out_dev = x_t.data_ptr(), score.data_ptr(), _lib.ptr(t_out)
        a.a_out_dev, a.e_out_dev = _lib.ptr(kept.get('a')), _lib.ptr(kept.get('e'))
        a.x_coeff_out_dev, a.sigma_out_dev = _lib.ptr(kept.get('x_coeff')), _lib.ptr(kept.get('sigma'))
        a.B, a.D, a.alpha, a.t_max = B, D, float(self.alpha), float(self.sde.T)
        a.clamp_eps = clamp_arg(clamp_eps)
        a.seed, a.sample_offset = seed, offset
        _lib.check(L.dlpm_lim_loss_elements_f32(C.byref(a), st))

        if isinstance(model, UNetModel):
            output = model._forward_checked(x_t, t_out, None)
        elif isinstance(model, MLPModel):
            output = model(x_t, t_out)
        else:
            output = model(x_t, t_out).contiguous().float()                                      # loss.py:32
        assert output.shape == x_t.shape, 'the model returned {}, expected {}'.format(tuple(output.shape), tuple(x_t.shape))

        if out is None:
            out = torch.empty(B, dtype=torch.float32, device=dev)
        # F.smooth_l1_loss(output, score, beta=1, reduction='mean') (loss.py:39) is the mean of the per-sample means: every row has D
        # elements
        _lib.check(L.dlpm_loss_terms_f32(output.data_ptr(), score.data_ptr(), out.data_ptr(), B, 1, D, 1, out.numel(), out_offset, st))
        self._advance_key(B)
        res = {'losses': out, 't': t_out}
        if keep:
            res.update(kept, x_t=x_t, score=score, output=output)
        return res

    def training_losses_lim(self, model, x_start, y=None, clamp_a=None, clamp_eps=None, noise=None, return_terms=False,
                            check_finite=True):
        """Forward-only, under torch.inference_mode(): LIM's objective (GenerativeLevyProcess.training_losses_lim, :680-709, and
        loss_fn, LIM/functions/loss.py:12-41) as an evaluation metric, not a training step.

        One kernel of its own (k_lim_loss_elements: e, t, x_t = x0 diffusion_coeff(t) + e marginal_std(t), score = -e / alpha),
        one forward of the net on (x_t, t), then the DLPM loss's terms kernel (smooth-L1, beta = 1) and its estimator (the mean,
        with the non-finite flag that stands for the reference's `Nan in losses` assertion, read only with `check_finite`).
        Returns the 0-dim fp32 loss on the device (with `return_terms`: (loss, terms[B], t[B] float32)).  `clamp_a` is accepted and
        stored as the reference does; gen_sas draws its a without it.  Unconditional nets only.

        Draws.  rng='philox': all on the device, keyed as sample() keys its own (dataset_stream() and sample_offset mean the
        same here).  rng='reference': the reference's host order (_lim_loss_host_draws).  `noise=` injects any of 't' [B], 'e'
        (shape of x_start, used as given), 'x_coeff' and 'sigma' [B] (together).

        Coefficients.  diffusion_coeff(t) and marginal_std(t) are differences of nearly equal numbers, and the reference's fp32
        evaluation destroys them: against fp64, marginal_std is off by 6-12 % as t -> 1e-5 (1.614e-4 against 1.541e-4 at t = 1e-5,
        alpha = 1.7), by more than 1e-3 relative on 0.04-0.07 % of uniform draws and by more than 1e-5 on 1.8-2.7 %;
        diffusion_coeff by up to 1.8e-5.  What a given fp32 evaluation returns there depends on its libm, so no device formula can
        agree with it.  Hence: when t is known on the host (rng='reference', or an injected 't' that is a CPU tensor or an
        array) and no coefficients are injected, they are computed there with lim.VPSDE's torch ops, the reference's own
        sequence, and passed to the kernel as arrays; when t is drawn on the device (or injected as a device tensor) the kernel
        evaluates them in fp64 from the fp32 t and rounds once."""
        if not (torch.is_tensor(x_start) and x_start.is_cuda):
            raise NotImplementedError('training_losses_lim runs on the GPU only; there is no CPU fallback')
        noise = self._lim_check_args(model, x_start, y, noise)
        self.dlpm.gen_a.setParams(clamp_a=clamp_a)          # stateful, as in the reference (:688-689)
        self.dlpm.gen_eps.setParams(clamp_eps=clamp_eps)
        if hasattr(model, 'eval'):
            model.eval()
        if _wants_graph(model):       # as in training_losses_dlpm
            spec = dict(lim=True, clamp_eps=clamp_eps, noise=noise)
            loss, terms, t = _TrainingLoss.apply(self, model, spec, x_start, *model.parameters())
            return (loss, terms, t) if return_terms else loss
        with torch.inference_mode():
            r = self._lim_loss_terms(model, x_start, clamp_eps, noise)
            loss = self._loss_reduce(r['losses'], x_start.shape[0], 1, 1, 'mean', check_finite)
        return (loss, r['losses'], r['t']) if return_terms else loss

    def training_losses(self, models, x_start, model_kwargs=None, **kwargs):
        """GenerativeLevyProcess.training_losses (:581-609).  For a differentiable MLPModel (MLPModel(p, differentiable=True)) under
        grad mode 'loss' carries a graph -- one autograd.Function around the whole loss, the same launches and bits, nothing read on
        the host -- so the reference's loop (loss.backward(), optimizer.step()) trains it.  Otherwise forward-only, under
        torch.inference_mode(), as a held-out metric: {'loss': 0-dim fp32 tensor on the device, 'losses': the per-extended-sample terms
        [outer * inner * B] (this build's addition), 't': the timesteps [B]}.  `model_kwargs={'y': labels}` reaches a
        class-conditional net with the labels following their sample into every replica; the nested form
        {'model_kwargs': {'y': labels}} (the only one the reference's own splat lets through) is accepted too.  Other keywords
        as training_losses_dlpm.  With LIM=True the call goes to training_losses_lim (`model_kwargs` is splatted into it as the
        reference does, :606, so {'y': ...} reaches its refusal); 'losses' are then the [B] per-sample terms and 't' the
        continuous times, float32."""
        model = models['default']
        if self.LIM:
            assert 'return_terms' not in kwargs
            loss, losses, t = self.training_losses_lim(model, x_start, **dict(model_kwargs or {}), return_terms=True, **kwargs)
            return {'loss': loss, 'losses': losses, 't': t}
        mk = dict(model_kwargs or {})
        if set(mk) == {'model_kwargs'}:
            mk = dict(mk['model_kwargs'] or {})
        assert 'model_kwargs' not in kwargs and 'return_terms' not in kwargs
        loss, losses, t = self.training_losses_dlpm(model, x_start, model_kwargs=mk, return_terms=True, **kwargs)
        return {'loss': loss, 'losses': losses, 't': t}


def _progress_bar(progress, total):
    """A tqdm bar of `total` steps, or None when no progress display is asked for."""
    if not progress:
        return None
    from tqdm import tqdm
    return tqdm(total=total)


def _native_kwargs(model, model_kwargs):
    """Whether the native sampler carries these model_kwargs: none for an unconditional net, exactly {'y': labels} for a
    class-conditional UNetModel.  Anything else runs the model from Python (model(x, t, **model_kwargs))."""
    if getattr(model, 'num_classes', None) is not None:
        return set(model_kwargs or {}) == {'y'}
    return not model_kwargs


def init_method_by_parameter(p, **kw):
    """dlpm/dlpm_experiment.py:103-131 for method == 'dlpm'."""
    m = p['method']
    assert m in ['dlpm', 'lim'], "chosen_gen_model should be in ['dlpm', 'lim'], got {}".format(m)
    q = p[m]
    return GenerativeLevyProcess(alpha=q['alpha'], device=p['device'], reverse_steps=q['reverse_steps'],
                                 model_mean_type=q.get('mean_predict', 'EPSILON'),
                                 model_var_type=q.get('var_predict', 'FIXED'),
                                 rescale_timesteps=q['rescale_timesteps'], isotropic=q['isotropic'], LIM=(m == 'lim'),
                                 scale=q.get('scale', 'scale_preserving'), input_scaling=q.get('input_scaling', False),
                                 **kw)
