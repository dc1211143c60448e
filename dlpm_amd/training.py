"""Training of the 2-D toy net on the device: the step that produces a checkpoint.

`MLPTrainer.step` is one optimisation step of the reference's loop (bem/TrainingManager.py:116-133) for an `MLPModel`: the loss
elements, the net, the loss terms and their estimator -- the launches `training_losses` makes -- then the loss gradient, the net's
backward, the gradient-norm clip, AdamW and the EMA shadows (include/dlpm_amd_train.h).  Nothing is synchronised and no device
value is read: the loss and the non-finite flag stay on the device.  `TrainingManager` is the reference's wrapper around it:
epochs over a [N, 1, dim] device tensor, one host read per epoch, checkpoints in the reference's format.

The parameters live in ONE flat fp32 vector, `torch.nn.utils.parameters_to_vector(model.parameters())` -- `named_parameters()`
order, every alias of the state_dict once, as the reference's EMA shadows and optimizer state are keyed -- and so do both moments
and every shadow.  After each step the vector is scattered back into the net's packed blob, so `model(x, t)` sees the current
weights; the torch module itself is only written by `sync()`.  UNet training is out of scope.
"""
import copy
import ctypes as C

import torch

from . import _lib
from . import checkpoint as _checkpoint
from .mlp import MLPModel

MAX_EMA = 8


def _refuse_model(model):
    if not isinstance(model, MLPModel):
        raise NotImplementedError('training runs for the 2-D toy net (MLPModel) only, got {}: training of the UNets is out of scope '
                                  '(DESIGN.md section 8)'.format(type(model).__name__))
    if model.general:
        raise NotImplementedError('training runs at the shipped 64-unit architecture (nunits 64, time_emb_size <= 64, LayerNorm, skip '
                                  "connections, kernel='auto'); this net (nunits {}, time_emb_size {}, group_norm {}, skip_connection {}, "
                                  'kernel {!r}) takes the general forward.  Its gradients come through torch.autograd -- '
                                  'MLPModel(p, differentiable=True), then the reference\'s own loop: training_losses(...)[\'loss\'].backward() '
                                  'and a torch.optim optimizer (DESIGN.md section 3.21); the fused trainer for wide nets is a follow-up '
                                  '(DESIGN.md section 9)'.format(model.nunits, model.time_emb_size, model.group_norm,
                                                                           model.skip_connection, model.kernel))


class MLPTrainer:
    """AdamW (torch.optim.AdamW's update, decoupled decay) with optional EMA shadows and gradient-norm clip on an MLPModel.

    `lr` is an attribute: a schedule is host arithmetic between steps.  After `step()`: `last_loss` (0-dim fp32) and `last_flag`
    (int32 [1], 1 when a loss term or the loss was not finite) on the device."""

    def __init__(self, model, method, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, ema_rates=None, grad_clip=None):
        _refuse_model(model)
        ema_rates = [float(mu) for mu in (ema_rates or [])]
        if len(ema_rates) > MAX_EMA:
            raise ValueError('at most {} EMA rates, got {}'.format(MAX_EMA, len(ema_rates)))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError('betas must lie in [0, 1), got {}'.format(tuple(betas)))
        if grad_clip is not None and not grad_clip > 0:
            raise ValueError('grad_clip must be positive or None, got {}'.format(grad_clip))
        self.model, self.method = model, method
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.ema_rates, self.grad_clip = ema_rates, grad_clip
        self.names = [n for n, _ in model.named_parameters()]
        self.shapes = [tuple(p.shape) for p in model.parameters()]
        self.numels = [p.numel() for p in model.parameters()]
        self.device = dev = torch.device(method.device)
        L = _lib.lib()
        h = model.native_handle()
        self.P = P = int(L.dlpm_mlp_param_floats(h))
        assert P == sum(self.numels), 'the library counts {} parameters, the module {}'.format(P, sum(self.numels))
        with torch.cuda.device(dev):
            self.theta = torch.empty(P, dtype=torch.float32, device=dev)
            _lib.check(L.dlpm_mlp_export_params_f32(h, self.theta.data_ptr(), P, _lib.stream_ptr()))
        self._generation = model.handle_generation
        self.exp_avg = torch.zeros(P, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(P, dtype=torch.float32, device=dev)
        self.shadows = [self.theta.clone() for _ in ema_rates]
        self.grad = torch.zeros(P, dtype=torch.float32, device=dev)
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.clip_coef = torch.ones(1, dtype=torch.float32, device=dev)
        self.last_loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.last_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.step_count = 0
        self._ws = None

    # ------------------------------------------------------------------------------------------ the native handle
    def _handle(self):
        """The net's handle holding the trainer's parameters: a handle rebuilt from the torch module meanwhile (load_state_dict,
        invalidate) is given the flat vector again."""
        h = self.model.native_handle()
        if self.model.handle_generation != self._generation:
            _lib.check(_lib.lib().dlpm_mlp_import_params_f32(h, self.theta.data_ptr(), self.P, _lib.stream_ptr()))
            self._generation = self.model.handle_generation
        return h

    def _workspace(self, h, rows):
        need = int(_lib.lib().dlpm_mlp_backward_workspace_bytes(h, rows))
        assert need > 0
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    # ------------------------------------------------------------------------------------------ one step
    def backward(self, x_in, tvec, dmodel):
        """self.grad <- d loss / d parameters for dL/d(output) `dmodel` at the net's inputs (x_in [rows, 1, F], tvec [rows])."""
        h = self._handle()
        rows = int(x_in.shape[0])
        ws = self._workspace(h, rows)
        _lib.check(_lib.lib().dlpm_mlp_backward_f32(h, x_in.data_ptr(), tvec.data_ptr(), dmodel.data_ptr(), rows, self.grad.data_ptr(),
                                                    None, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        return self.grad

    def apply_gradient(self):
        """The clip (when set), AdamW and the shadows on self.grad, then the new parameters into the net."""
        L, st = _lib.lib(), _lib.stream_ptr()
        if self.grad_clip is not None:
            _lib.check(L.dlpm_grad_clip_coef_f32(self.grad.data_ptr(), self.P, float(self.grad_clip), self.grad_norm.data_ptr(),
                                                 self.clip_coef.data_ptr(), st))
        a = _lib.AdamwArgs()
        a.theta_dev, a.grad_dev = self.theta.data_ptr(), self.grad.data_ptr()
        a.exp_avg_dev, a.exp_avg_sq_dev, a.n = self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.P
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay
        a.step = self.step_count + 1
        a.coef_dev = self.clip_coef.data_ptr() if self.grad_clip is not None else None
        a.n_ema = len(self.shadows)
        for i, (s, mu) in enumerate(zip(self.shadows, self.ema_rates)):
            a.ema_dev[i], a.ema_mu[i] = s.data_ptr(), mu
        _lib.check(L.dlpm_adamw_step_f32(C.byref(a), st))
        _lib.check(L.dlpm_mlp_import_params_f32(self._handle(), self.theta.data_ptr(), self.P, st))
        self.step_count += 1

    def step(self, x_start, loss_type='EPS_LOSS', lploss=2.0, loss_monte_carlo='mean', monte_carlo_outer=1, monte_carlo_inner=1,
             clamp_a=None, clamp_eps=None, noise=None, y=None):
        """One optimisation step on the batch x_start [B, 1, F] (a device tensor).  Arguments as training_losses_dlpm -- for a
        method built with LIM=True as training_losses_lim (y, clamp_a, clamp_eps, noise).  Returns the loss, a 0-dim tensor on the
        device; nothing is read."""
        model, method = self.model, self.method
        L = _lib.lib()
        if not (torch.is_tensor(x_start) and x_start.is_cuda):
            raise _lib.DlpmError('MLPTrainer.step runs on the MI355X only; there is no CPU fallback')
        for m in list(model._dependents):       # a sampler captured on this handle reads tables the new weights outdate
            m._drop_samplers_of(model)
        self._handle()
        B = int(x_start.shape[0])
        with torch.no_grad(), torch.cuda.device(self.device):
            if method.LIM:
                inj = method._lim_check_args(model, x_start, y, noise)
                method.dlpm.gen_a.setParams(clamp_a=clamp_a)
                method.dlpm.gen_eps.setParams(clamp_eps=clamp_eps)
                r = method._lim_loss_terms(model, x_start, clamp_eps, inj, keep=True)
                out, target, x_in, tvec = r['output'], r['score'], r['x_t'], r['t']
                lp, outer, inner, median = 1, 1, 1, None
            else:
                assert y is None, 'the toy net takes no labels'
                lp, _ = method._loss_check_args(model, x_start, loss_type, lploss, loss_monte_carlo, monte_carlo_outer, monte_carlo_inner,
                                                None)
                outer, inner = int(monte_carlo_outer), int(monte_carlo_inner)
                method.dlpm.gen_a.setParams(clamp_a=clamp_a)
                method.dlpm.gen_eps.setParams(clamp_eps=clamp_eps)
                r = method._loss_terms(model, x_start, lp, outer, inner, None, clamp_a, noise, keep=True)
                out, target, x_in, tvec = r['model_eps'], r['eps_t'], r['x_in'], r['tvec']
                median = torch.empty(B, dtype=torch.int32, device=self.device) if loss_monte_carlo == 'median' else None
            self.last_loss = method._loss_reduce(r['losses'], B, outer, inner, 'median' if median is not None else 'mean', False,
                                                 median_index=median, flag=self.last_flag)
            D = int(x_in[0].numel())
            dmodel = torch.empty_like(out)
            _lib.check(L.dlpm_loss_grad_f32(out.data_ptr(), target.data_ptr(), r['losses'].data_ptr(), _lib.ptr(median),
                                            dmodel.data_ptr(), B, outer, inner, D, lp, _lib.stream_ptr()))
            self.backward(x_in, tvec, dmodel)
            self.apply_gradient()
        return self.last_loss

    # ------------------------------------------------------------------------------------------ state
    def sync(self):
        """The parameters back into the torch module (one device read), through the module's own invalidate(): samplers captured
        earlier are dropped and the next forward rebuilds the handle from the module."""
        with torch.no_grad():
            flat = self.theta.cpu()
            for p, n, shape, off in zip(self.model.parameters(), self.numels, self.shapes, self._offsets()):
                p.copy_(flat[off:off + n].reshape(shape).to(p.device))
        self.model.invalidate()
        return self.model

    def _offsets(self):
        offs, o = [], 0
        for n in self.numels:
            offs.append(o)
            o += n
        return offs

    def _split(self, flat):
        return {name: flat[off:off + n].reshape(shape) for name, n, shape, off in zip(self.names, self.numels, self.shapes, self._offsets())}

    def _join(self, d, what):
        missing = [n for n in self.names if n not in d]
        assert not missing, '{} lacks {}'.format(what, missing[:4])
        parts = []
        for name, shape in zip(self.names, self.shapes):
            v = torch.as_tensor(d[name])
            assert tuple(v.shape) == shape, (what, name, tuple(v.shape), shape)
            parts.append(v.detach().to(self.device, torch.float32).reshape(-1))
        return torch.cat(parts)

    def ema_state(self, i):
        """The i-th shadow as EMAHelper.state_dict() gives it: the bare {parameter name: tensor} dict over named_parameters()."""
        return self._split(self.shadows[i].clone())

    def load_ema_state(self, i, shadow):
        self.shadows[i].copy_(self._join(_checkpoint._strip_module(dict(shadow)), 'the EMA shadow'))

    def load_parameters(self):
        """The flat vector again from the torch module (after model.load_state_dict)."""
        with torch.no_grad():
            self.theta.copy_(torch.nn.utils.parameters_to_vector([p.detach().float() for p in self.model.parameters()]).to(self.device))
        self._generation = None
        self._handle()

    def state_dict(self):
        """The optimizer state in the form torch.optim.AdamW.state_dict() has (optimizer_state_dict)."""
        return optimizer_state_dict(self.names, self.shapes, self.exp_avg.cpu(), self.exp_avg_sq.cpu(), self.step_count, self.lr,
                                    self.betas, self.eps, self.weight_decay)

    def load_state_dict(self, sd):
        groups = sd['param_groups']
        assert len(groups) == 1 and len(groups[0]['params']) == len(self.names), 'one parameter group over model.parameters() is expected'
        g = groups[0]
        if g.get('amsgrad') or g.get('maximize'):
            raise NotImplementedError('amsgrad / maximize are not implemented')
        self.lr, self.betas, self.eps, self.weight_decay = float(g['lr']), (float(g['betas'][0]), float(g['betas'][1])), float(g['eps']), \
            float(g['weight_decay'])
        state = sd['state']
        if not state:
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            self.step_count = 0
            return
        ids = g['params']
        steps = {int(state[i]['step']) for i in ids}
        assert len(steps) == 1, 'the parameters are at different steps: {}'.format(sorted(steps))
        self.step_count = steps.pop()
        self.exp_avg.copy_(self._join({n: state[i]['exp_avg'] for n, i in zip(self.names, ids)}, 'exp_avg'))
        self.exp_avg_sq.copy_(self._join({n: state[i]['exp_avg_sq'] for n, i in zip(self.names, ids)}, 'exp_avg_sq'))


def optimizer_state_dict(names, shapes, exp_avg, exp_avg_sq, step, lr, betas, eps, weight_decay):
    """torch.optim.AdamW.state_dict() from flat moment vectors: 'state' {index: step, exp_avg, exp_avg_sq} over model.parameters()
    order (empty before the first step, as torch's), one entry in 'param_groups' with the keys the installed torch writes."""
    template = torch.optim.AdamW([torch.zeros(1) for _ in names], lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay).state_dict()
    group = dict(template['param_groups'][0], params=list(range(len(names))))
    state, off = {}, 0
    for i, shape in enumerate(shapes):
        n = 1
        for d in shape:
            n *= d
        if step > 0:
            state[i] = {'step': torch.tensor(float(step)), 'exp_avg': exp_avg[off:off + n].reshape(shape).clone(),
                        'exp_avg_sq': exp_avg_sq[off:off + n].reshape(shape).clone()}
        off += n
    return {'state': state, 'param_groups': [group]}


def _adamw_settings(opt):
    """(lr, betas, eps, weight_decay) of a torch.optim.AdamW with one parameter group; anything else is refused."""
    if not isinstance(opt, torch.optim.AdamW):
        raise NotImplementedError('the device optimizer is AdamW: pass None or a torch.optim.AdamW whose hyper-parameters are read, '
                                  'got {}'.format(type(opt).__name__))
    assert len(opt.param_groups) == 1, 'one parameter group is expected'
    g = opt.param_groups[0]
    if g.get('amsgrad') or g.get('maximize'):
        raise NotImplementedError('amsgrad / maximize are not implemented')
    return dict(lr=g['lr'], betas=tuple(g['betas']), eps=g['eps'], weight_decay=g['weight_decay'])


class TrainingManager:
    """bem/TrainingManager.py for the toy net, the loop on the device.

    `models`: {'default': MLPModel}.  `data`: a [N, 1, dim] device tensor or a ToyLoader (its tensor and batch size are taken).
    `optimizers`: None -- AdamW at p['optim']['lr'], betas (0.9, 0.999) -- or a torch.optim.AdamW (or {'default': one}) whose
    hyper-parameters are read.  `learning_schedules`: None or 'steplr' (lr = lr0 * lr_gamma ** (steps // lr_step_size), torch's
    StepLR stepped once per batch as the reference steps it); the reference's other schedules come from a `get_scheduler` that
    is not part of this build.  Further keywords: `p` (the config: optim.lr, optim.lr_step_size, optim.lr_gamma,
    training.batch_size), `batch_size`, `lr_step_size`, `lr_gamma`, `seed`; what remains is passed to train() as the reference
    passes its own.

    Each epoch walks a permutation of the data drawn from a CPU torch.Generator seeded by (seed, epoch); the last short batch is
    trained as it is.  The Philox key of a step is that of the method's call number `total_steps`, so a run resumed from a
    checkpoint draws what the uninterrupted run draws.  The device is read once per epoch: the mean loss (-> `epoch_losses`)
    and the non-finite flag, which raises FloatingPointError('nan in loss detected') or calls `reset_models`."""

    def __init__(self, models, data, method, optimizers, learning_schedules, eval, logger=None, ema_rates=None, reset_models=None,
                 **kwargs):
        assert 'default' in models, "models must contain the 'default' model"
        if set(models) != {'default'}:
            raise NotImplementedError("one net is trained, models['default']; got {}".format(sorted(models)))
        _refuse_model(models['default'])
        kwargs = dict(kwargs)
        self.p = kwargs.pop('p', None)
        optim = dict((self.p or {}).get('optim') or {})
        opt = optimizers.get('default') if isinstance(optimizers, dict) else optimizers
        if opt is None:
            assert 'lr' in optim, "optimizers=None reads p['optim']['lr']: pass p="
            self._opt = dict(lr=optim['lr'], betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
        else:
            self._opt = _adamw_settings(opt)
        ls = learning_schedules.get('default') if isinstance(learning_schedules, dict) else learning_schedules
        if ls not in (None, 'steplr'):
            raise NotImplementedError("learning schedule {!r}: None and 'steplr' are implemented (the reference builds the others with a "
                                      'get_scheduler that is not part of this build)'.format(ls))
        self.schedule = ls
        self.lr_step_size = kwargs.pop('lr_step_size', optim.get('lr_step_size'))
        self.lr_gamma = kwargs.pop('lr_gamma', optim.get('lr_gamma'))
        if ls == 'steplr':
            assert self.lr_step_size and self.lr_gamma is not None, "'steplr' takes lr_step_size and lr_gamma"
        self.seed = int(kwargs.pop('seed', getattr(method, 'seed', 0)))
        batch_size = kwargs.pop('batch_size', None)
        if hasattr(data, 'data') and hasattr(data, 'batch_size'):       # a ToyLoader
            batch_size = batch_size or data.batch_size
            data = data.data
        if batch_size is None:
            batch_size = ((self.p or {}).get('training') or {}).get('batch_size')
        assert batch_size, 'no batch size: pass a ToyLoader, batch_size= or p with training.batch_size'
        assert torch.is_tensor(data) and data.dim() == 3 and data.shape[1] == 1 and data.dtype == torch.float32, \
            'data must be a float32 [N, 1, dim] tensor or a ToyLoader'
        self.epochs = 0
        self.total_steps = 0
        self.models, self.data, self.batch_size, self.method = models, data, int(batch_size), method
        self.optimizers, self.learning_schedules = optimizers, learning_schedules
        self.eval, self.logger, self.reset_models = eval, logger, reset_models
        self.ema_rates = list(ema_rates) if ema_rates else None
        self.kwargs = kwargs
        self.epoch_losses = []
        self.trainer = None

    def exists_ls(self, name='default'):
        return name == 'default' and self.schedule is not None

    def _trainer(self, grad_clip=None):
        if self.trainer is None:
            self.trainer = MLPTrainer(self.models['default'], self.method, ema_rates=self.ema_rates, **self._opt)
            self.base_lr = self.trainer.lr
        self.trainer.grad_clip = grad_clip
        return self.trainer

    def current_lr(self):
        if self.schedule == 'steplr':
            return self.base_lr * self.lr_gamma ** (self.total_steps // self.lr_step_size)
        return self.base_lr

    def train(self, total_epoch, **kwargs):
        kw = copy.deepcopy(self.kwargs)
        kw.update(kwargs)
        return self._train_epochs(total_epoch, **kw)

    def _train_epochs(self, total_epochs, eval_freq=None, checkpoint_freq=None, checkpoint_callback=None, no_ema_eval=False, grad_clip=None,
                      max_batch_per_epoch=None, **loss_kwargs):
        method = self.method
        dev = torch.device(method.device)
        data = self.data.to(dev)
        N, bs = int(data.shape[0]), self.batch_size
        tr = self._trainer(grad_clip)
        while self.epochs < total_epochs:
            g = torch.Generator()
            g.manual_seed((self.seed * 1000003 + self.epochs) & 0x7FFFFFFFFFFFFFFF)
            perm = torch.randperm(N, generator=g).to(dev)
            loss_sum = torch.zeros(1, dtype=torch.float64, device=dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            steps = 0
            for i, first in enumerate(range(0, N, bs)):
                if max_batch_per_epoch is not None and i >= max_batch_per_epoch:
                    break
                x = data[perm[first:first + bs]]
                tr.lr = self.current_lr()
                saved, method.calls = method.calls, self.total_steps
                try:
                    loss = tr.step(x, **loss_kwargs)
                finally:
                    method.calls = saved
                loss_sum += loss
                flag |= tr.last_flag
                steps += 1
                self.total_steps += 1
            assert steps > 0, 'an epoch without a batch'
            host = torch.cat([loss_sum, flag.double()]).cpu()        # the epoch's one device read
            self.epochs += 1
            if host[1] != 0:
                if self.reset_models is None:
                    raise FloatingPointError('nan in loss detected')
                print('nan in loss detected, reinitializing models...')
                self.models, self.optimizers, self.learning_schedules = self.reset_models()
                _refuse_model(self.models['default'])
                self.trainer = None
                tr = self._trainer(grad_clip)
                continue
            epoch_loss = float(host[0]) / steps
            self.epoch_losses.append(epoch_loss)
            if self.eval is not None and hasattr(self.eval, 'register_epoch_loss'):
                self.eval.register_epoch_loss(epoch_loss)
            if self.logger is not None:
                self.logger.log('current_epoch', self.epochs)
            if checkpoint_freq is not None and self.epochs % checkpoint_freq == 0:
                checkpoint_callback(self.epochs)
            if eval_freq is not None and self.epochs % eval_freq == 0:
                self.evaluate()
                if not no_ema_eval:
                    self.evaluate(evaluate_emas=True)
        return self.epoch_losses

    def sync(self):
        """The trained parameters into models['default'] (MLPTrainer.sync)."""
        if self.trainer is not None:
            self.trainer.sync()
        return self.models

    def ema_model(self, i):
        """A fresh MLPModel (built from `p`) carrying the i-th shadow."""
        assert self.trainer is not None and self.p is not None, 'an EMA model is built from the config: pass p='
        m = MLPModel(self.p)
        self.sync()
        sd = _checkpoint.model_state({'model_parameters': self.models['default'].state_dict(),
                                      'ema_models': [{k: v.cpu() for k, v in self.trainer.ema_state(i).items()}]}, ema=0, model=m)
        m.load_state_dict(sd)
        return m

    def evaluate(self, evaluate_emas=False, **kwargs):
        if self.eval is None:
            return
        if not evaluate_emas:
            self.sync()
            with torch.inference_mode():
                self.eval.evaluate_model(self.models, **kwargs)
        elif self.ema_rates:
            for i in range(len(self.ema_rates)):
                with torch.inference_mode():
                    self.eval.evaluate_model({'default': self.ema_model(i)}, **kwargs)

    def _schedule_state(self):
        if self.schedule is None:
            return None
        return {'schedule': self.schedule, 'step_size': self.lr_step_size, 'gamma': self.lr_gamma, 'base_lrs': [self.base_lr],
                'last_epoch': self.total_steps, '_last_lr': [self.current_lr()]}

    def save(self, filepath):
        tr = self._trainer(self.trainer.grad_clip if self.trainer is not None else None)
        self.sync()
        shadows = None
        if self.ema_rates:
            shadows = {'default': [{k: v.cpu() for k, v in tr.ema_state(i).items()} for i in range(len(self.ema_rates))]}
        sd = tr.state_dict()
        sd['param_groups'][0]['lr'] = self.base_lr if self.schedule is None else self.current_lr()
        return _checkpoint.save_checkpoint(filepath, self.models, epoch=self.epochs, steps=self.total_steps, ema_shadows=shadows,
                                           optimizers={'default': sd}, learning_schedules={'default': self._schedule_state()})

    def load(self, filepath):
        ck = _checkpoint.read_checkpoint(filepath)
        self.total_steps, self.epochs = ck['steps'], ck['epoch']
        self.models['default'].load_state_dict(_checkpoint.model_state(ck))
        tr = self._trainer(self.trainer.grad_clip if self.trainer is not None else None)
        tr.load_parameters()
        if ck.get('optimizer') is not None:
            tr.load_state_dict(ck['optimizer'])
        ls = ck.get('learning_schedule')
        if ls is not None and self.schedule is not None:
            self.base_lr = ls['base_lrs'][0]
        elif ck.get('optimizer') is not None:
            self.base_lr = tr.lr
        if self.ema_rates:
            assert ck.get('ema_models') is not None, 'no ema model in checkpoint'
            for i, shadow in zip(range(len(self.ema_rates)), ck['ema_models']):
                tr.load_ema_state(i, shadow)
