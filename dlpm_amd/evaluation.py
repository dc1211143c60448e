"""EvaluationManager: the generate-and-dump half of bem/evaluate/EvaluationManager.py.

The reference generates `data_to_generate` images in chunks of `eval.batch_size`; after every chunk it copies
the fp32 samples to the host and calls `torchvision.utils.save_image` once per sample, serially, before the next
chunk starts (EvaluationManager.py:174-196).  Here a chunk's samples stay on the GPU, are quantised to 8-bit RGB
by `dlpm_images_to_rgb8`, cross PCIe on a side stream into pinned memory (3 bytes/pixel), and are encoded and
written by native threads (`dlpm_png_write_rgb8`) while the next chunk is sampling.  File names and pixel values
are the reference's (`<gen_data_path>/<i>.png`, i counting over all chunks).  With the Philox generator the whole
dump is one `dataset_stream()`: sample i is the same whatever the chunk size, so `device_batch` may enlarge the
chunks beyond `eval.batch_size` without changing a pixel.

Of the metrics half, any Inception forward is out of scope (the network needs weights nobody can ship); `fid` is filled by
`evaluate_fid` with the Frechet distance of the features the caller brings, or of the flattened samples (`evaluate_metrics_2d` appends
the reference's own 0.0 for a 2-D config).  Built are: `losses`, which `evaluate_loss` fills with the reference's own objective
(GenerativeLevyProcess.training_losses: the DLPM loss, or LIM's own for a LIM method), forward only, on held-out samples; `mmd`,
which `evaluate_mmd` fills with the reference's multi-bandwidth Gaussian MMD between generated and real samples; and `precision` / `recall` / `f_1_pr`, which `evaluate_prd` fills with
the reference's PRD figures (EvaluationManager.py:157-168, :218-221) from a k-means clustering on the device; `wass`, which
`evaluate_wass` fills with the reference's histogram earth mover's distance (EvaluationManager.py:146-151); the reference's whole
2-D branch from one generation, `evaluate_metrics_2d`; and PRDC from features -- `precision`, `recall`, `density`, `coverage`, `f_1_pr`,
`f_1_dc` as the image branch fills them (:215-225) -- which `evaluate_prdc` computes by k-nearest neighbours on the flattened samples
or on the features of a callable the caller brings (dlpm_amd/metrics.py).
"""
import copy
import ctypes as C
import os
import queue
import threading

import numpy as np
import torch

from . import _lib


class ImageDump:
    """[n,C,H,W] fp32 images in [0,1] on the GPU -> `<out_dir>/<first_index+i>.png`, pipelined:
    stream of the caller: quantise -> side stream: D2H into a pinned slot -> worker thread: PNG encode + write."""

    def __init__(self, out_dir, C_, H, W, max_batch, level=6, threads=4, overlap=True, slots=2):
        os.makedirs(out_dir, exist_ok=True)
        self.out_dir, self.shape, self.max_batch = out_dir, (C_, H, W), max_batch
        self.level, self.threads, self.overlap = level, threads, overlap
        self.dev = [torch.empty((max_batch, H, W, 3), dtype=torch.uint8, device='cuda') for _ in range(slots)]
        self.host = [torch.empty((max_batch, H, W, 3), dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self.copy_stream = torch.cuda.Stream()
        self.free = queue.Queue()
        for s in range(slots):
            self.free.put(s)
        self.pending = queue.Queue()
        self.error = None
        self.written = 0
        self.worker = None
        if overlap:
            self.worker = threading.Thread(target=self._run, name='dlpm-png-writer', daemon=True)
            self.worker.start()

    def _write(self, slot, n, first_index):
        _lib.check(_lib.lib().dlpm_png_write_rgb8(self.host[slot].data_ptr(), n, self.shape[1], self.shape[2],
                                                 self.out_dir.encode(), first_index, self.level, self.threads))
        self.written += n

    def _run(self):
        while True:
            item = self.pending.get()
            if item is None:
                return
            slot, n, first_index, done = item
            try:
                done.synchronize()
                if self.error is None:
                    self._write(slot, n, first_index)
            except Exception as e:            # surfaced by submit()/close() on the caller's thread
                self.error = e
            finally:
                self.free.put(slot)

    def submit(self, x, first_index):
        if self.error is not None:
            raise self.error
        n = x.shape[0]
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape[1:]) == self.shape and n <= self.max_batch, x.shape
        x = x.contiguous()
        slot = self.free.get()                # waits while both slots are still being written
        _lib.check(_lib.lib().dlpm_images_to_rgb8(x.data_ptr(), self.dev[slot].data_ptr(), n, *self.shape,
                                                 _lib.stream_ptr()))
        ready = torch.cuda.Event()
        ready.record()
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(ready)
            self.host[slot][:n].copy_(self.dev[slot][:n], non_blocking=True)
            done = torch.cuda.Event()
            done.record()
        if self.overlap:
            self.pending.put((slot, n, first_index, done))
        else:
            done.synchronize()
            try:
                self._write(slot, n, first_index)
            finally:
                self.free.put(slot)

    def close(self):
        if self.worker is not None:
            self.pending.put(None)
            self.worker.join()
            self.worker = None
        if self.error is not None:
            raise self.error


DEVICE_BATCH = 1024   # images per chunk under device_batch='auto' (the per-sample rate of the image nets is flat beyond it)


def auto_device_batch(models, chw, data_to_generate, reserve=0.5, device=None):
    """Largest power of two <= DEVICE_BATCH (and not beyond the dump) whose network workspaces + state fit in `reserve` of the
    free HBM OF `device` (the GPU the method and its nets live on -- not the process's current device: a sharded evaluation
    runs the method on cuda:k with current device 0).  Nets that cannot tell their workspace (`workspace_bytes(B, image_size)`)
    count as 64 x the state.  The sampler's [T,B] tables, graph pools and the dump's pinned buffers live in the reserve; the
    caller halves the chunk if the first one still runs out of memory (`_evaluate_model`)."""
    free, _ = torch.cuda.mem_get_info(device)
    b = 1
    while b * 2 <= min(DEVICE_BATCH, max(1, int(data_to_generate))):
        b *= 2
    state = 4 * chw[0] * chw[1] * chw[2]
    while b > 1:
        need = 4 * b * state
        for m in (models or {}).values():
            wb = getattr(m, 'workspace_bytes', None)
            need += wb(b, chw[1]) if wb is not None else 64 * b * state
        if need <= reserve * free:
            break
        b //= 2
    return b


class EvaluationManager:
    """Constructor and entry points of bem/evaluate/EvaluationManager.py:33-118; `_evaluate_model` covers the
    generation + image-dump part (:174-196) and the 2-D generation call (:135)."""

    def __init__(self, method, gen_manager, dataloader, verbose=True, logger=None, is_image=False, gen_data_path=None,
                 real_data_path=None, overlap=True, png_level=6, png_threads=4, device_batch='auto', **kwargs):
        self.method, self.gen_manager, self.dataloader = method, gen_manager, dataloader
        self.verbose, self.logger, self.is_image = verbose, logger, is_image
        self.gen_data_path, self.real_data_path = gen_data_path, real_data_path
        self.overlap, self.png_level, self.png_threads = overlap, png_level, png_threads
        self.device_batch = device_batch
        self.kwargs = kwargs
        self.evals = None
        self.reset()

    def reset(self, keep_losses=False, keep_evals=False):
        old = self.evals or {}
        e = {}
        for k in ('losses', 'losses_batch'):                                        # EvaluationManager.py:60-77
            e[k] = old[k] if keep_losses else np.array([], dtype=np.float32)
        for k in ('wass', 'mmd', 'precision', 'recall', 'density', 'coverage', 'f_1_pr', 'f_1_dc', 'fid', 'fig'):
            e[k] = old[k] if keep_evals else []
        e['grad_norm'] = old['grad_norm'] if keep_evals else np.array([], dtype=np.float32)
        if keep_evals and 'w1' in old:                                              # evaluate_w1's own key: there only once filled
            e['w1'] = old['w1']
        self.evals = e

    def evaluate_loss(self, models, data, batch_size, per_timestep=False, class_labels=None, **loss_kwargs):
        """Held-out denoising loss of `models['default']` on `data`: the Proposition-9 loss of the reference
        (training_losses_dlpm, GenerativeLevyProcess.py:612-677) without gradients, as a Python float appended to
        `evals['losses']` (the key the reference fills from training).

        `data`: float32 [N, C, H, W] / [N, 1, F] tensor or array already in the net's range, or an iterable of such batches
        (an (x, label) pair counts as x); it is cut into chunks of `batch_size`.  `loss_kwargs`: lploss, loss_monte_carlo,
        monte_carlo_outer, monte_carlo_inner, clamp_a, clamp_eps as training_losses_dlpm.  `class_labels` [N]: labels of a
        class-conditional net, sliced with the chunks.

        The whole pass is one dataset_stream(): sample i draws the same (t, a, z) whatever the chunking, its terms go to the
        slot of an [outer * inner * N] device buffer that ONE call on all N samples would put them in, and the estimator runs
        once at the end -- so with rng='philox' the figure is bit-identical for every batch_size.  (rng='reference' continues the
        host streams chunk by chunk, as successive reference calls would.)  One non-finite check for the whole pass.
        `per_timestep=True` returns (loss, t[N] int32, terms[outer * inner * N]) on the host.

        A LIM method (`method.LIM`) is evaluated on its own objective, training_losses_lim (GenerativeLevyProcess.py:680-709), the same
        way: one dataset_stream(), one [N] buffer of per-sample terms, one reduce, bit-identical for every batch_size under Philox;
        `per_timestep=True` returns (loss, t[N] float32, terms[N]).  Its `loss_kwargs` are clamp_a and clamp_eps; the DLPM-only ones
        (lploss, loss_monte_carlo, monte_carlo_*, loss_type) and class labels are refused before any device work."""
        method = self.method
        if method.LIM:
            dlpm_only = sorted(set(loss_kwargs) & {'lploss', 'loss_monte_carlo', 'monte_carlo_outer', 'monte_carlo_inner', 'loss_type'})
            if dlpm_only:
                raise TypeError('evaluate_loss: {} belong to the DLPM loss; training_losses_lim takes clamp_a and clamp_eps'.format(
                    ', '.join(dlpm_only)))
            assert set(loss_kwargs) <= {'clamp_a', 'clamp_eps'}, 'unknown loss arguments {}'.format(
                sorted(set(loss_kwargs) - {'clamp_a', 'clamp_eps'}))
            if class_labels is not None:
                raise NotImplementedError('training_losses_lim takes unconditional nets only: the reference hard-wires y = None '
                                          '(dlpm/methods/GenerativeLevyProcess.py:706)')
        model = models['default']
        if not torch.is_tensor(data) and not isinstance(data, np.ndarray):
            data = [torch.as_tensor(b[0] if isinstance(b, (tuple, list)) else b) for b in data]
            data = torch.cat(data) if data else torch.empty(0)
        data = torch.as_tensor(data)
        N = int(data.shape[0])
        assert N > 0, 'evaluate_loss: no data'
        assert data.dtype == torch.float32, 'evaluate_loss takes float32 data in the net\'s range, got %s' % data.dtype
        if method.LIM:
            return self._evaluate_loss_lim(model, data, N, batch_size, per_timestep, loss_kwargs.get('clamp_a'),
                                           loss_kwargs.get('clamp_eps'))
        kw = dict(loss_type='EPS_LOSS', lploss=2.0, loss_monte_carlo='mean', monte_carlo_outer=1, monte_carlo_inner=1,
                  model_kwargs=None, clamp_a=None, clamp_eps=None)
        assert set(loss_kwargs) <= set(kw), 'unknown loss arguments {}'.format(sorted(set(loss_kwargs) - set(kw)))
        kw.update(loss_kwargs)
        outer, inner = int(kw['monte_carlo_outer']), int(kw['monte_carlo_inner'])
        mk = dict(kw['model_kwargs'] or {})
        class_labels = self._labels(class_labels, N)
        dev = torch.device(method.device)
        batch_size = max(1, int(batch_size))
        terms = t_all = None
        with method.dataset_stream():
            for first in range(0, N, batch_size):
                x = data[first:first + batch_size].to(dev)
                if class_labels is not None:
                    mk['y'] = class_labels[first:first + x.shape[0]]
                lploss, mkc = method._loss_check_args(model, x, kw['loss_type'], kw['lploss'], kw['loss_monte_carlo'], outer, inner, mk)
                if terms is None:
                    method.dlpm.gen_a.setParams(clamp_a=kw['clamp_a'])
                    method.dlpm.gen_eps.setParams(clamp_eps=kw['clamp_eps'])
                    if hasattr(model, 'eval'):
                        model.eval()
                    terms = torch.empty(outer * inner * N, dtype=torch.float32, device=dev)
                    t_all = torch.empty(N, dtype=torch.int32, device=dev)
                with torch.inference_mode():
                    method._loss_terms(model, x, lploss, outer, inner, mkc, kw['clamp_a'], None, out=terms, out_stride=N,
                                       out_offset=first, t_out=t_all[first:first + x.shape[0]])
            with torch.inference_mode():
                loss = float(method._loss_reduce(terms, N, outer, inner, kw['loss_monte_carlo'], check_finite=True))
        self.evals['losses'] = np.append(self.evals['losses'], np.float32(loss))
        if per_timestep:
            return loss, t_all.cpu(), terms.cpu()
        return loss

    def _evaluate_loss_lim(self, model, data, N, batch_size, per_timestep, clamp_a, clamp_eps):
        """evaluate_loss for a LIM method: the same chunk loop inside one dataset_stream(), the per-sample terms written at their
        global slot of one [N] device buffer, one reduce at the end."""
        method = self.method
        dev = torch.device(method.device)
        batch_size = max(1, int(batch_size))
        if dev.type != 'cuda':
            raise NotImplementedError('training_losses_lim runs on the GPU only; there is no CPU fallback')
        terms = t_all = None
        with method.dataset_stream():
            for first in range(0, N, batch_size):
                x = data[first:first + batch_size].to(dev)
                noise = method._lim_check_args(model, x)
                if terms is None:
                    method.dlpm.gen_a.setParams(clamp_a=clamp_a)
                    method.dlpm.gen_eps.setParams(clamp_eps=clamp_eps)
                    if hasattr(model, 'eval'):
                        model.eval()
                    terms = torch.empty(N, dtype=torch.float32, device=dev)
                    t_all = torch.empty(N, dtype=torch.float32, device=dev)
                with torch.inference_mode():
                    method._lim_loss_terms(model, x, clamp_eps, noise, out=terms, out_offset=first, t_out=t_all[first:first + x.shape[0]])
            with torch.inference_mode():
                loss = float(method._loss_reduce(terms, N, 1, 1, 'mean', check_finite=True))
        self.evals['losses'] = np.append(self.evals['losses'], np.float32(loss))
        if per_timestep:
            return loss, t_all.cpu(), terms.cpu()
        return loss

    def evaluate_mmd(self, models, real_data, data_to_generate, batch_size, class_labels=None, kernel_mul=2.0, kernel_num=5,
                     fix_sigma=None, return_samples=False, samples=None, **kwargs):
        """Multi-bandwidth Gaussian MMD (the reference's MMD_loss, EvaluationManager.py:153) between `data_to_generate` generated
        samples and `real_data[:data_to_generate]`, as a Python float appended to `evals['mmd']`.

        `real_data`: float32 [N, ...] tensor or array with N >= data_to_generate, in the range GenerationManager leaves its samples in
        ([0, 1] for images, the raw coordinates for 2-D data).  The samples are generated in chunks of `batch_size` like
        `_evaluate_model` -- inside one dataset_stream(), on the device, without declaring a batch -- and every chunk is written after
        GenerationManager's post-processing into one [N, D] device buffer; the metric is ONE dlpm_mmd_f32 call on that buffer.  With
        rng='philox' the figure therefore does not depend on `batch_size`.  `class_labels` and `kwargs` as `_evaluate_model`.
        `return_samples=True` returns (mmd, the generated samples in their own shape, on the device).  `samples=` [N, ...] takes the
        place of the generation, as in `evaluate_prd`."""
        from . import metrics
        real, gen, shape = self._real_and_samples('evaluate_mmd', models, real_data, data_to_generate, batch_size, class_labels, samples,
                                                  kwargs)
        value = metrics.mmd(gen, real, kernel_mul=kernel_mul, kernel_num=kernel_num, fix_sigma=fix_sigma)
        self.evals['mmd'].append(value)
        if return_samples:
            return value, gen.reshape((len(gen),) + shape)
        return value

    @staticmethod
    def _labels(class_labels, N):
        """`class_labels` of the evaluate_* methods as an int64 host tensor of at least N labels; None stays None."""
        if class_labels is None:
            return None
        class_labels = torch.as_tensor(class_labels).to('cpu', torch.int64).reshape(-1)
        assert class_labels.numel() >= N, 'class_labels: %d labels for %d samples' % (class_labels.numel(), N)
        return class_labels

    def _real_and_samples(self, who, models, real_data, data_to_generate, batch_size, class_labels, samples, kwargs, single=None):
        """What every sample metric starts from, with `who` in the messages: the N = data_to_generate samples, given (`samples=`) or
        generated (`_generate_flat`), and `real_data[:N]` beside them.  Returns (real [N, D] on the samples' device, samples [N, D], the
        shape of one sample).  `real_data=None`: the real samples are the generation manager's own, `load_original_data(N)`, as in the
        reference.  `single`: the refusal of N = 1, for the figures that leave the last sample out.  Every refusal comes before the
        generation."""
        N = int(data_to_generate)
        assert N > 0, '%s: data_to_generate must be positive' % who
        if real_data is None:                                                       # EvaluationManager.py:140
            real_data = self.gen_manager.load_original_data(N)
        real = torch.as_tensor(real_data)
        assert real.dtype == torch.float32, '%s takes float32 real_data, got %s' % (who, real.dtype)
        assert real.shape[0] >= N, '%s: %d real samples for %d generated' % (who, real.shape[0], N)
        assert single is None or N >= 2, '%s: %s' % (who, single)
        if samples is not None:
            gen, shape = self._given_samples(who, samples, N)
        else:
            gen, shape = self._generate_flat(models, N, batch_size, self._labels(class_labels, N), kwargs)
        real = real[:N].reshape(N, -1)
        assert real.shape[1] == gen.shape[1], '%s: real samples hold %d values, generated ones %d' % (who, real.shape[1], gen.shape[1])
        return real.to(gen.device), gen, shape

    def _generate_flat(self, models, N, batch_size, class_labels, kwargs):
        """N samples in chunks of `batch_size`, like `_evaluate_model`: inside one dataset_stream(), on the device, without declaring a
        batch, every chunk written after GenerationManager's post-processing into one [N, D] device buffer.  Returns (buffer, the
        shape of one sample).  `class_labels`: None or an int64 host tensor of at least N labels."""
        batch_size = max(1, int(batch_size))
        stream = getattr(self.method, 'dataset_stream', None)
        gen, total = None, 0
        with (stream() if stream is not None else _null()):
            while total < N:
                n = min(batch_size, N - total)
                if class_labels is not None:
                    kwargs['model_kwargs'] = {'y': class_labels[total:total + n]}
                x = self.gen_manager.generate(models, n, to_host=False, declare_batch=False, **kwargs)
                if gen is None:
                    shape = tuple(x.shape[1:])
                    gen = torch.empty((N, x[0].numel()), dtype=torch.float32, device=x.device)
                gen[total:total + n] = x.reshape(n, -1)
                total += n
        return gen, shape

    def evaluate_prd(self, models, real_data, data_to_generate, batch_size, class_labels=None, num_angles=201, num_clusters=None,
                     seed=0, samples=None, **kwargs):
        """PRD precision / recall (the reference's compute_precision_recall_curve + compute_f_beta, EvaluationManager.py:157-168)
        between `real_data[:data_to_generate]` and `data_to_generate` generated samples: appends the max F_8 to `evals['precision']`,
        the max F_1/8 to `evals['recall']` and 2 p r / (p + r) (0 when both vanish, :218-221) to `evals['f_1_pr']`, and returns them as
        {'precision', 'recall', 'f_1_pr'}.  As in the reference the REAL data is the curve's `eval_data`.

        The samples are generated as `evaluate_mmd` generates them (same chunk loop, so the same samples for the same method state),
        or taken from `samples=` (e.g. `evaluate_mmd(..., return_samples=True)[1]`) without generating again.  `num_clusters=None`
        is the reference's rule: 100 above 2500 samples, else 20.  `seed` seeds the k-means++ draws.  `density`, `coverage` and
        `fid` are not touched."""
        from . import metrics
        real, gen, _ = self._real_and_samples('evaluate_prd', models, real_data, data_to_generate, batch_size, class_labels, samples,
                                              kwargs)
        if num_clusters is None:
            num_clusters = 100 if len(gen) > 2500 else 20
        _, _, parts = metrics.prd(real, gen, num_clusters=num_clusters, num_angles=num_angles, seed=seed, return_parts=True)
        p, r = parts['f_beta']
        res = {'precision': p, 'recall': r, 'f_1_pr': (2 * p * r) / (p + r) if p + r > 0 else 0.}
        for k, v in res.items():
            self.evals[k].append(v)
        return res

    @staticmethod
    def _given_samples(who, samples, N):
        """`samples=` of the evaluate_* methods as ([N, D] tensor, the shape of one sample)."""
        gen = torch.as_tensor(samples)
        assert gen.dtype == torch.float32, '%s takes float32 samples, got %s' % (who, gen.dtype)
        assert gen.shape[0] == N, '%s: %d samples given for data_to_generate = %d' % (who, gen.shape[0], N)
        return gen.reshape(N, -1), tuple(gen.shape[1:])

    def evaluate_wass(self, models, real_data, data_to_generate, batch_size, class_labels=None, bins=None, samples=None, **kwargs):
        """The reference's `wass` figure (compute_wasserstein_distance, EvaluationManager.py:146-151) between
        `real_data[:data_to_generate]` and `data_to_generate` generated samples, as a Python float appended to `evals['wass']`: the
        earth mover's distance between the histograms of the two FLATTENED sets, the last sample of each left out as the reference's
        `[:-1]` slice leaves it out (metrics.compute_wasserstein_distance).

        The samples are generated as `evaluate_mmd` generates them, or taken from `samples=`.  `bins=None` is the reference's rule:
        250 bins from 512 samples on, else numpy's 'auto'.  With rng='philox' the figure does not depend on `batch_size`."""
        from . import metrics
        real, gen, _ = self._real_and_samples('evaluate_wass', models, real_data, data_to_generate, batch_size, class_labels, samples,
                                              kwargs, single='the reference leaves the last sample out, so at least 2 are needed')
        if bins is None:
            bins = 250 if len(gen) >= 512 else 'auto'                               # EvaluationManager.py:149
        value = metrics.compute_wasserstein_distance(real, gen, bins=bins)
        self.evals['wass'].append(value)
        return value

    def evaluate_w1(self, models, real_data, data_to_generate, batch_size, class_labels=None, ground='l1_mean', samples=None, **kwargs):
        """The exact W1 between `real_data[:data_to_generate]` and `data_to_generate` generated samples as points (metrics.w1: optimal
        transport with one bin of mass 1 / N per point), as a Python float appended to `evals['w1']` -- a key of this package, created
        on first use.  ground='l1_mean' is the figure the reference's commented-out manual_compute branch (EvaluationManager.py:144-146)
        was meant to put into `wass`; 'euclidean' the textbook W1.  `real_data=None`: samples of the config's own distribution.

        The samples are generated as `evaluate_mmd` generates them, or taken from `samples=`."""
        from . import metrics
        if ground not in metrics.W1_GROUNDS:
            raise ValueError('evaluate_w1: ground must be one of %s, got %r' % (sorted(metrics.W1_GROUNDS), ground))
        real, gen, _ = self._real_and_samples('evaluate_w1', models, real_data, data_to_generate, batch_size, class_labels, samples,
                                              kwargs)
        value = metrics.w1(real, gen, ground=ground)
        self.evals.setdefault('w1', []).append(value)
        return value

    def evaluate_tail(self, models, real_data, data_to_generate, batch_size, class_labels=None, xi=0.95, levels=100, marginal='norm',
                      samples=None, **kwargs):
        """The tail figures (metrics.tail) between `real_data[:data_to_generate]` and `data_to_generate` generated
        samples: the mean squared logarithmic error between their upper quantiles above the level `xi` and the Hill tail index of
        each set, appended to `evals['msle']`, `evals['tail_index_real']` and `evals['tail_index_gen']` -- keys of this package,
        created on first use -- and returned as a dict under those names.  marginal='norm' takes the norm of every sample, 'abs' every
        scalar.  `real_data=None`: samples of the config's own distribution.

        The samples are generated as `evaluate_mmd` generates them, or taken from `samples=`; with rng='philox' the figures do not
        depend on `batch_size`.  GenerationManager._post clamps 2-D samples to +-6 and data.quantile_cutoff < 1 clamps the real set: a
        clamp shows up as ties at the top, and a tail that lies wholly on the clamp has index +inf -- choose `xi` below it."""
        from . import metrics
        metrics._tail_check(torch.zeros(2, 1), torch.zeros(2, 1), xi, levels, marginal)     # the refusals, before the generation
        real, gen, _ = self._real_and_samples('evaluate_tail', models, real_data, data_to_generate, batch_size, class_labels, samples,
                                              kwargs)
        t = metrics.tail(real, gen, xi=xi, levels=levels, marginal=marginal)
        res = {'msle': t['msle'], 'tail_index_real': t['tail_index_first'], 'tail_index_gen': t['tail_index_second']}
        for k, v in res.items():
            self.evals.setdefault(k, []).append(v)
        return res

    def evaluate_prdc(self, models, real_data, data_to_generate, batch_size, class_labels=None, nearest_k=5, features=None, samples=None,
                      **kwargs):
        """k-nearest-neighbour precision, recall, density and coverage (the `prdc` package's compute_prdc, the last step of
        bem/evaluate/fid_score.py:303-336) between `real_data[:data_to_generate]` and `data_to_generate` generated samples: appends
        them to `evals['precision']`, `['recall']`, `['density']`, `['coverage']` and their two harmonic means to `['f_1_pr']` and
        `['f_1_dc']` (0 where both terms vanish), as EvaluationManager.py:215-225 does in the image branch, and returns the six as a dict.

        `features`: None -- the flattened samples are the features -- or a callable mapping a float32 GPU batch to [B, F] float32: this
        is where a caller plugs in an embedding (an Inception network with their own weights, any other feature net).  It receives the
        samples in their own shape, [B, C, H, W] with values in [0, 1] as GenerationManager leaves them or [B, 1, 2] for 2-D data, in
        chunks of `batch_size`, and is applied to both sets, chunk by chunk -- it must treat every sample on its own (no batch
        statistics) for the figures not to depend on `batch_size`.  No feature network is built here, and FID is not computed.
        The samples are generated as `evaluate_mmd` generates them, or taken from `samples=`."""
        from . import metrics
        N = int(data_to_generate)
        assert int(nearest_k) == nearest_k and 1 <= nearest_k <= metrics.MAX_NEAREST_K, (
            'evaluate_prdc: nearest_k must be an integer in [1, %d], got %r' % (metrics.MAX_NEAREST_K, nearest_k))
        assert N <= 0 or nearest_k < N, 'evaluate_prdc: nearest_k = %d needs more than %d samples, got %d' % (nearest_k, nearest_k, N)
        assert features is None or callable(features), 'evaluate_prdc: features must be None or a callable, got %r' % (features,)
        real, gen, shape = self._real_and_samples('evaluate_prdc', models, real_data, data_to_generate, batch_size, class_labels, samples,
                                                  kwargs)
        if features is not None:
            real, gen = (self._features(features, t, shape, batch_size) for t in (real, gen))
        fig = metrics.prdc(real, gen, nearest_k=int(nearest_k))
        res = dict(fig, f_1_pr=metrics.f_1(fig['precision'], fig['recall']), f_1_dc=metrics.f_1(fig['density'], fig['coverage']))
        for k, v in res.items():
            self.evals[k].append(v)
        return res

    def evaluate_fid(self, models, real_data, data_to_generate, batch_size, class_labels=None, features=None, real_stats=None,
                     samples=None, **kwargs):
        """Frechet distance (calculate_frechet_distance on np.mean / np.cov statistics, bem/evaluate/fid_score.py:118-171, the `fid` of
        EvaluationManager.py:198-205) between `real_data[:data_to_generate]` and `data_to_generate` generated samples, as a Python float
        appended to `evals['fid']`.
        The name FID belongs to Inception pool3 features: this is the Frechet distance of whatever `features` returns.

        `features`: None -- the flattened samples are the features (at most 4096 values) -- or a callable as in `evaluate_prdc`.
        `real_stats`: None, a pair (mu [F], sigma [F, F]) of float64 arrays or tensors, or the path of an .npz holding `mu` and `sigma`
        (the reference's precomputed-statistics files, compute_statistics_of_path): it takes the place of the real set's statistics,
        and `real_data` may then be None.  The samples are generated as `evaluate_mmd` generates them, or taken from `samples=`."""
        from . import metrics
        N = int(data_to_generate)
        assert N >= 2, 'evaluate_fid: a covariance needs at least 2 samples, got data_to_generate = %d' % N
        assert features is None or callable(features), 'evaluate_fid: features must be None or a callable, got %r' % (features,)
        if real_stats is not None:
            if isinstance(real_stats, (str, os.PathLike)):
                with np.load(real_stats) as z:
                    real_stats = (z['mu'], z['sigma'])
            assert len(real_stats) == 2, 'evaluate_fid: real_stats must be (mu, sigma) or the path of an .npz with mu and sigma'
            mu1, sigma1 = (torch.as_tensor(v) for v in real_stats)
            assert mu1.dtype == torch.float64 and sigma1.dtype == torch.float64, 'evaluate_fid takes float64 real_stats, got %s and %s' % (
                mu1.dtype, sigma1.dtype)
            assert mu1.dim() == 1 and tuple(sigma1.shape) == (mu1.shape[0],) * 2, 'evaluate_fid: real_stats of shapes %s and %s' % (
                tuple(mu1.shape), tuple(sigma1.shape))
            if samples is not None:
                gen, shape = self._given_samples('evaluate_fid', samples, N)
            else:
                gen, shape = self._generate_flat(models, N, batch_size, self._labels(class_labels, N), kwargs)
            real = None
        else:
            real, gen, shape = self._real_and_samples('evaluate_fid', models, real_data, data_to_generate, batch_size, class_labels, samples,
                                                      kwargs)
        if features is not None:
            real, gen = (None if t is None else self._features(features, t, shape, batch_size, who='evaluate_fid') for t in (real, gen))
        if real is not None:
            value = metrics.fd(real, gen)
        else:
            assert gen.shape[1] == mu1.shape[0], 'evaluate_fid: real_stats of %d features, the samples have %d' % (mu1.shape[0], gen.shape[1])
            value = metrics.calculate_frechet_distance(mu1, sigma1, *metrics.feature_statistics(gen))
        self.evals['fid'].append(value)
        return value

    @staticmethod
    def _features(features, flat, shape, batch_size, who='evaluate_prdc'):
        """`features` applied to the [N, D] set `flat` in chunks of `batch_size`, every chunk in the samples' own shape on the GPU:
        an [N, F] float32 device tensor."""
        batch_size = max(1, int(batch_size))
        dev = flat.device if flat.is_cuda else torch.device('cuda', torch.cuda.current_device())
        out = []
        for first in range(0, len(flat), batch_size):
            x = flat[first:first + batch_size].to(dev).reshape((-1,) + tuple(shape))
            f = torch.as_tensor(features(x))
            assert f.dtype == torch.float32 and f.dim() == 2 and f.shape[0] == x.shape[0], (
                '%s: features must return float32 [B, F], got %s %s for a batch of %d' % (who, f.dtype, tuple(f.shape), x.shape[0]))
            out.append(f.to(dev))
        return torch.cat(out)

    def evaluate_metrics_2d(self, models, real_data, data_to_generate, batch_size, class_labels=None, seed=0, **kwargs):
        """The reference's whole evaluation of a 2-D config (EvaluationManager.py:126-168, :218-230) from ONE generation: `wass`, `mmd`,
        `precision`, `recall` and `f_1_pr` as `evaluate_wass` / `evaluate_mmd` / `evaluate_prd` compute them on the same samples, and
        the reference's own constants for the image-only figures: `density` = `coverage` = `fid` = `f_1_dc` = 0.0, `fig` = None.
        Every key is appended to `evals`; the dict is returned with the generated samples (their own shape, on the device) under
        'samples'.  `seed` seeds the k-means++ draws of the PRD clustering."""
        real, gen, shape = self._real_and_samples(
            'evaluate_metrics_2d', models, real_data, data_to_generate, batch_size, class_labels, None, kwargs,
            single='the reference leaves the last sample out of `wass`, so at least 2 are needed')
        N = len(gen)
        samples = gen.reshape((N,) + shape)
        res = {'wass': self.evaluate_wass(models, real, N, batch_size, samples=samples),
               'mmd': self.evaluate_mmd(models, real, N, batch_size, samples=samples)}
        res.update(self.evaluate_prd(models, real, N, batch_size, seed=seed, samples=samples))
        rest = {'density': 0., 'coverage': 0., 'fid': 0., 'f_1_dc': 0., 'fig': None}
        for k, v in rest.items():
            self.evals[k].append(v)
        res.update(rest)
        res['samples'] = samples
        return res

    def generate_default(self, models, nsamples, **kwargs):
        self.gen_manager.generate(models, nsamples, **kwargs)
        return self.gen_manager

    def evaluate_model(self, models, **kwargs):
        tmp_kwargs = copy.deepcopy(self.kwargs)
        tmp_kwargs.update(kwargs)
        return self._evaluate_model(models, **tmp_kwargs)

    def _evaluate_model(self, models, data_to_generate, batch_size, fig_lim=1.5, callback_on_logging=None, class_labels=None,
                        **kwargs):
        """`class_labels`: for a class-conditional net, the [data_to_generate] labels in global sample order; every chunk samples with
        its slice (model_kwargs={'y': ...}), so neither pixels nor labels depend on the chunking, and the image dump writes them to
        `<gen_data_path>/labels.npy` (int64, index i = image i)."""
        if class_labels is not None:
            class_labels = self._labels(class_labels, data_to_generate)[:data_to_generate]
        if not self.is_image:
            if class_labels is not None:
                kwargs['model_kwargs'] = {'y': class_labels}
            self.gen_manager.generate(models, data_to_generate, **kwargs)          # EvaluationManager.py:135
            return {'generated': data_to_generate, 'gen_data_path': None}
        assert self.gen_data_path is not None, 'gen_data_path is needed to save the generated images'
        total = 0
        if data_to_generate != 0:
            _, (data, _) = next(enumerate(self.gen_manager.original_data))
            Cc, H, W = data.shape[1:]
            stream = getattr(self.method, 'dataset_stream', None)
            min_batch = None
            if self.device_batch and stream is not None and getattr(self.method, 'rng', None) == 'philox':
                # inside dataset_stream() the i-th sample does not depend on the chunking, so the chunk can be
                # sized for the GPU (eval.batch_size = 64 leaves an MI355X half idle: the CIFAR net runs at 46 % of its
                # B = 1024 per-sample rate there) without changing any pixel.  'auto' (the default since round 5: a caller
                # that drops the classes in unchanged gets the fast shape) = up to DEVICE_BATCH images, as many as the nets'
                # workspaces leave room for in free HBM; device_batch=0 / None keeps the reference's chunking.
                dev_b = self.device_batch
                if dev_b == 'auto':
                    mdev = torch.device(getattr(self.method, 'device', 'cuda'))
                    dev_b = auto_device_batch(models, [Cc, H, W], data_to_generate, device=mdev if mdev.type == 'cuda' else None)
                    min_batch = batch_size                                          # an OOM on the first chunk halves down to the config's own
                batch_size = max(batch_size, int(dev_b))
            dump = ImageDump(self.gen_data_path, Cc, H, W, min(batch_size, data_to_generate), level=self.png_level,
                             threads=self.png_threads, overlap=self.overlap)
            remaining = data_to_generate
            # (the chunks are sampled with declare_batch=False: the nets keep whatever batch their owner declared -- none by default --
            #  so that a pixel depends neither on the chunking nor on the last chunk's size; tests/test_image_dump.py)
            if self.verbose:
                print('generating {} images for fid computation'.format(remaining))
            ctx = stream() if stream is not None else _null()
            try:
                with ctx:
                    while remaining > 0:                                           # EvaluationManager.py:181-193
                        n = min(batch_size, remaining)
                        if class_labels is not None:
                            kwargs['model_kwargs'] = {'y': class_labels[total:total + n]}
                        try:
                            self.gen_manager.generate(models, n, to_host=False, declare_batch=False, **kwargs)
                        except (torch.cuda.OutOfMemoryError, RuntimeError) as e:
                            # 'auto' sized the chunk from free HBM with a reserve; should the FIRST chunk not fit after all, halve it
                            # (the pixels do not depend on the chunking inside dataset_stream()) instead of failing the dump
                            oom = isinstance(e, torch.cuda.OutOfMemoryError) or 'out of memory' in str(e).lower()
                            if not (oom and total == 0 and min_batch is not None and batch_size // 2 >= max(1, min_batch)):
                                raise
                            batch_size //= 2
                            torch.cuda.empty_cache()
                            if self.verbose:
                                print('device_batch=auto: out of memory, chunk halved to {}'.format(batch_size))
                            continue
                        dump.submit(self.gen_manager.samples, total)
                        total += n
                        remaining -= n
                        if self.verbose:
                            print(remaining, end=' ', flush=True)
            finally:
                dump.close()
            assert data_to_generate == total == dump.written
            if class_labels is not None:
                np.save(os.path.join(self.gen_data_path, 'labels.npy'), class_labels.numpy())
            if self.verbose:
                print('saved generated data in {}.'.format(self.gen_data_path))
        return {'generated': total, 'gen_data_path': self.gen_data_path}


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
