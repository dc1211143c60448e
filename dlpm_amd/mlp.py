"""MLPModel: the 2-D toy score network (dlpm/models/Model.py:17-211) as a parameter container whose
forward runs in libdlpm_amd.  Same `state_dict` keys (including the aliases the reference's
nn.Sequential re-registrations create) and the same construction order, hence the same default
initialisation under a given torch.manual_seed.

Any nunits / time_emb_size up to 1024, nfeatures up to 64, nblocks >= 0, group_norm and skip_connection on or
off, as the reference takes them.  The shipped architecture (64 units, time_emb_size <= 64, LayerNorm, skip)
runs on the lane kernels; every other one, or any with kernel='general', on the general MFMA forward
(include/dlpm_amd_mlp.h).  The fused trainer (dlpm_amd.training) runs the shipped architecture only; with
`differentiable=True` every architecture is differentiable through torch.autograd (include/dlpm_amd_mlp_grad.h), so
the reference's own loop -- loss.backward(), torch.optim, clip_grad_norm_, EMAHelper -- trains it on these kernels.
"""
import ctypes as C
import weakref

import torch
import torch.nn as nn

from . import _lib


MAX_UNITS, MAX_TIME_EMB, MAX_FEATURES = 1024, 1024, 64     # GEN_MAX_* of dlpm_amd/csrc/mlp_pack.h


class _Forward(torch.autograd.Function):
    """model(x, t) for a differentiable MLPModel: the forward is the launch MLPModel.forward always makes, the backward one
    dlpm_mlp_grad_backward_f32 whose flat gradient is handed to autograd as views in named_parameters() order."""

    @staticmethod
    def forward(ctx, model, x, t, *params):
        ctx.model, ctx.key = model, model._imported
        ctx.save_for_backward(x, t)
        return model._launch(x, t)

    @staticmethod
    def backward(ctx, dout):
        x, t = ctx.saved_tensors
        model = ctx.model
        if model._imported != ctx.key:
            raise RuntimeError('a parameter of the MLPModel was modified between its forward and this backward; the native handle '
                               'holds the newer values')
        flat, dx = model.native_backward(x, t, dout, want_dx=ctx.needs_input_grad[1])
        return (None, dx, None) + tuple(g if ctx.needs_input_grad[3 + i] else None for i, g in enumerate(model.split_flat(flat)))


def _cond_block(nunits, temb, group_norm=True):
    """Parameters of DiffusionBlockConditioned (time-conditioned): DiffusionBlocks.py:88-123."""
    blk = nn.Module()
    blk.group_norm1 = nn.LayerNorm([nunits]) if group_norm else nn.Identity()
    blk.group_norm2 = nn.LayerNorm([nunits]) if group_norm else nn.Identity()
    drop = nn.Dropout(p=0.0)
    act = nn.SiLU()
    blk.mlp_1 = nn.Sequential(drop, nn.Linear(nunits, nunits), blk.group_norm1)
    blk.t_proj = nn.Sequential(drop, nn.Linear(temb, nunits), act)
    blk.mlp_2 = nn.Sequential(drop, nn.Linear(nunits, nunits), blk.group_norm2)
    return blk


class MLPModel(nn.Module):
    def __init__(self, p, kernel='auto', tile_rows=None, differentiable=False):
        """kernel: 'auto' (the lane kernels for the shipped architecture, the general forward otherwise) or 'general' (the general
        forward whatever the architecture).  tile_rows: None (the general forward takes 32-row tiles where they fit the LDS and
        fill the chip, 16-row tiles otherwise), or 16 / 32 for that height whatever the batch (the results are the same bits).
        differentiable (also a plain attribute): False -- forward returns a tensor without a graph, the handle keeps the parameters
        it was created with.  True -- when grad mode is on and x or a parameter requires grad, forward goes through
        torch.autograd (the same launch, the same bits; backward: dlpm_mlp_grad_backward_f32), and every forward first compares
        the parameters' identities and versions with those the handle holds and, on a change (torch.optim steps in place),
        imports them on the device (so does every other use of the handle: sampling, evaluation)."""
        super().__init__()
        m = p['model']
        self.nfeatures = int(p['data']['nfeatures'])
        self.nunits, self.nblocks, self.time_emb_size = int(m['nunits']), int(m['nblocks']), int(m['time_emb_size'])
        self.group_norm, self.skip_connection = bool(m['group_norm']), bool(m['skip_connection'])
        if kernel not in ('auto', 'general'):
            raise ValueError("kernel must be 'auto' or 'general', got {!r}".format(kernel))
        if tile_rows not in (None, 16, 32):
            raise ValueError('tile_rows must be None, 16 or 32, got {!r}'.format(tile_rows))
        if not isinstance(differentiable, bool):
            raise TypeError('differentiable must be a bool, got {!r}'.format(differentiable))
        self.kernel, self.tile_rows, self.differentiable = kernel, tile_rows, differentiable
        unsupported = []
        if not (m['no_a'] and p[p['method']]['isotropic']):
            unsupported.append('a_t inputs / non-isotropic (the reference asserts the same, Model.py:44)')
        if m['time_emb_type'] != 'learnable':
            unsupported.append("time_emb_type != 'learnable' (the reference's other two types do not run: Model.py:59 reads an "
                               'undefined attribute, :188 appends to an undefined list)')
        if m.get('a_pos_emb') or m.get('learn_variance'):
            unsupported.append('a_pos_emb / learn_variance')
        if m.get('dropout_rate', 0.0):
            unsupported.append('dropout (the forward is an inference path)')
        if self.nunits < 1 or self.time_emb_size < 1 or self.nfeatures < 1 or self.nblocks < 0:
            raise ValueError('nunits, time_emb_size and nfeatures must be positive and nblocks >= 0')
        if self.nunits > MAX_UNITS:
            unsupported.append('nunits {} > {} (a 16-row tile of activations must fit the LDS)'.format(self.nunits, MAX_UNITS))
        if self.time_emb_size > MAX_TIME_EMB:
            unsupported.append('time_emb_size {} > {}'.format(self.time_emb_size, MAX_TIME_EMB))
        if self.nfeatures > MAX_FEATURES:
            unsupported.append('nfeatures {} > {} (the input and output layers run on the VALU)'.format(self.nfeatures, MAX_FEATURES))
        if unsupported:
            raise NotImplementedError('dlpm_amd.MLPModel does not implement: ' + '; '.join(unsupported))
        act = nn.SiLU()
        self.group_norm_in = nn.LayerNorm([self.nunits]) if self.group_norm else nn.Identity()
        self.time_emb = nn.Linear(1, self.time_emb_size)
        self.time_mlp = nn.Sequential(self.time_emb, act, nn.Linear(self.time_emb_size, self.time_emb_size), act)
        self.linear_in = nn.Linear(self.nfeatures, self.nunits)
        self.inblock = nn.Sequential(self.linear_in, self.group_norm_in, act)
        self.midblocks = nn.ModuleList([_cond_block(self.nunits, self.time_emb_size, self.group_norm) for _ in range(self.nblocks)])
        self.outblocks_mean = nn.ModuleList([_cond_block(self.nunits, self.time_emb_size, self.group_norm),
                                             nn.Linear(self.nunits, self.nfeatures)])
        self._handle = None
        self.handle_generation = 0          # bumped whenever the native handle is destroyed (sampler cache keys carry it)
        self._dependents = weakref.WeakSet()  # method objects holding native samplers built on this handle
        self._imported = None               # (id, version) of every parameter as the handle holds them (differentiable)
        self._grad_ws = None                # workspace of the backward, grown as needed

    @property
    def general(self):
        """True when the forward is the general MFMA kernel (the routing of dlpm_mlp_create_ex): such a net samples and evaluates
        but has no one-launch sampling loop and no fused trainer (its gradients come through differentiable=True)."""
        return not (self.nunits == 64 and self.time_emb_size <= 64 and self.group_norm and self.skip_connection
                    and self.kernel == 'auto')

    def native_flags(self):
        return ((0 if self.group_norm else _lib.MLP_NO_LAYERNORM) | (0 if self.skip_connection else _lib.MLP_NO_SKIP)
                | (_lib.MLP_FORCE_GENERAL if self.kernel == 'general' else 0) | {None: 0, 16: _lib.MLP_TILE_16, 32: _lib.MLP_TILE_32}[self.tile_rows])

    def invalidate(self):
        for m in list(self._dependents):
            m._drop_samplers_of(self)
        if self._handle is not None:
            _lib.lib().dlpm_mlp_destroy(self._handle)
            self.handle_generation += 1
        self._handle = None

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self.invalidate()
        return r

    def __del__(self):
        try:
            self.invalidate()
        except Exception:
            pass

    def native_handle(self):
        if self._handle is not None:
            if self.differentiable:
                self._import_if_stale()
            return self._handle
        L = _lib.lib()
        h = C.c_void_p()
        _lib.check(L.dlpm_mlp_create_ex(self.nfeatures, self.nunits, self.nblocks, self.time_emb_size, self.native_flags(), C.byref(h)))
        try:
            assert (L.dlpm_mlp_tile_rows(h) > 0) == self.general, 'the library routes this net differently from MLPModel.general'
            for k, v in self.state_dict().items():
                w = v.detach().to('cpu', torch.float32).contiguous()
                _lib.check(L.dlpm_mlp_set_param(h, k.encode(), w.data_ptr(), w.numel()))
            _lib.check(L.dlpm_mlp_finalize(h))
        except Exception:
            L.dlpm_mlp_destroy(h)
            raise
        self._handle = h
        self._imported = self._param_key()
        return h

    # ------------------------------------------------------------------------------------------ autograd (differentiable=True)
    def _param_key(self):
        return tuple((id(p), p._version) for p in self.parameters())

    def _import_if_stale(self):
        """The handle with the parameters as they are now: after an in-place update (torch.optim) they are flattened on the device
        and imported, without the host and without finalize; samplers captured on the handle are dropped first, as
        MLPTrainer.step does."""
        key = self._param_key()
        if key != self._imported:
            for m in list(self._dependents):
                m._drop_samplers_of(self)
            first = next(self.parameters())
            device = first.device if first.is_cuda else torch.device('cuda', torch.cuda.current_device())
            with torch.no_grad(), torch.cuda.device(device):
                flat = torch.cat([p.detach().reshape(-1) for p in self.parameters()]).to(device, torch.float32).contiguous()
                _lib.check(_lib.lib().dlpm_mlp_grad_import_params_f32(self._handle, flat.data_ptr(), flat.numel(), _lib.stream_ptr()))
            self._imported = key

    def split_flat(self, flat):
        """Views of a flat parameter-sized vector in named_parameters() order, each on its parameter's device."""
        out, off = [], 0
        for p in self.parameters():
            g = flat[off:off + p.numel()].reshape(p.shape)
            out.append(g if g.device == p.device else g.to(p.device))
            off += p.numel()
        assert off == flat.numel(), 'the flat vector has {} elements, the parameters {}'.format(flat.numel(), off)
        return out

    def native_backward(self, x, t, dout, want_dx=False):
        """(flat gradient [P], dx or None) for dout = dL/d(output) at the inputs of a forward: one dlpm_mlp_grad_backward_f32 on
        the handle as it stands (lane or general)."""
        L, h = _lib.lib(), self.native_handle()
        rows = int(x.shape[0])
        x, dout = x.contiguous().float(), dout.contiguous().float()
        t = t.to(x.device, torch.float32).contiguous()
        assert dout.shape == x.shape, (tuple(dout.shape), tuple(x.shape))
        with torch.cuda.device(x.device):
            need = int(L.dlpm_mlp_grad_workspace_bytes(h, rows))
            if need <= 0:
                raise _lib.DlpmError('[dlpm status %d] %s' % (need, L.dlpm_last_error().decode('utf-8', 'replace')))
            if self._grad_ws is None or self._grad_ws.numel() < need or self._grad_ws.device != x.device:
                self._grad_ws = torch.empty(need, dtype=torch.uint8, device=x.device)
            flat = torch.empty(int(L.dlpm_mlp_grad_param_floats(h)), dtype=torch.float32, device=x.device)
            dx = torch.empty_like(x) if want_dx else None
            _lib.check(L.dlpm_mlp_grad_backward_f32(h, x.data_ptr(), t.data_ptr(), dout.data_ptr(), rows, flat.data_ptr(), _lib.ptr(dx),
                                                    self._grad_ws.data_ptr(), self._grad_ws.numel(), _lib.stream_ptr()))
        return flat, dx

    def _launch(self, x, t):
        out = torch.empty_like(x)
        _lib.check(_lib.lib().dlpm_mlp_forward(self.native_handle(), x.data_ptr(), t.data_ptr(), out.data_ptr(), x.shape[0],
                                              _lib.stream_ptr()))
        return out

    def forward(self, x, timestep, a_t_prime=None, a_t_1=None):
        """eps[B,1,F] = model(x[B,1,F], t[B]) on the GPU."""
        if not x.is_cuda:
            raise _lib.DlpmError('dlpm_amd.MLPModel.forward runs on the MI355X only; there is no CPU fallback')
        assert x.shape[1:] == (1, self.nfeatures), x.shape
        x = x.contiguous().float()
        t = timestep.to(x.device, torch.float32).contiguous()
        if self.differentiable:
            self.native_handle()            # imports parameters changed in place since the last call
            if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
                return _Forward.apply(self, x, t, *self.parameters())
        return self._launch(x, t)
