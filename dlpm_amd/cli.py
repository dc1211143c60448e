"""`eval.py --generate`-compatible command line for the sampling path (no dataset / neptune needed).

Covers the reference flags that reach the sampler (script_utils.py:11-12,35-39,56-67,82-83,155-221):
  --config --method --generate --reverse_steps --deterministic --clip --alpha --non_iso --scale --input_scaling --set_seed/--random_seed
  (--class_labels cycle|K: labels of a class-conditional net, i.e. a config with model.class_cond and data.num_classes)
plus the checkpoint to evaluate, resolved like eval.py does (eval.py:21, bem/utils_exp.py:96-139):
  --name N [--models_dir models] [--epoch E]  ->  models/N/<dataset>/model_<exphash>[_<E>].pt
or given directly with --checkpoint FILE; --ema_eval [--ema_index I] evaluates an EMA shadow.
Samples are produced in chunks of eval.batch_size like EvaluationManager (:181-193).
  --eval_loss DATA.npy [--lploss P] [--median OUTER INNER]: instead of generating, the held-out denoising loss of the checkpoint on
  the float32 samples of DATA.npy (already in the net's range), EvaluationManager.evaluate_loss; --lploss / --median as the
  reference's training flags.  The figure does not depend on --batch_size.  With --method lim it is LIM's own objective
  (training_losses_lim), which has no --lploss / --median.
  --eval_mmd REAL.npy --generate N: generate N samples and print the reference's multi-bandwidth Gaussian MMD between them and the
  first N float32 samples of REAL.npy (EvaluationManager.evaluate_mmd; images in [0, 1], 2-D points as they are).  May be combined
  with --out, not with --gen_data_path.  With --rng philox the figure does not depend on --batch_size.
  --eval_prd REAL.npy --generate N [--prd_seed S]: generate N samples and print the reference's PRD figures between the first N float32
  samples of REAL.npy and them (EvaluationManager.evaluate_prd: precision = max F_8, recall = max F_1/8 of the PRD curve, and their
  F_1; 100 clusters above 2500 samples, else 20).  Together with --eval_mmd the samples are generated once and both are printed.
  --eval_wass REAL.npy --generate N [--wass_bins K]: generate N samples and print the reference's `wass` figure between the first N
  float32 samples of REAL.npy and them (EvaluationManager.evaluate_wass: the earth mover's distance between the histograms of the
  flattened sets, the last sample of each left out as the reference does; 250 bins from 512 samples on, else numpy's 'auto').  With
  more than one of --eval_wass / --eval_mmd / --eval_prd / --eval_prdc / --eval_fid / --eval_w1 the samples are generated once and every figure is printed.
  --eval_w1 REAL.npy|dataset --generate N [--w1_ground l1_mean|euclidean]: the exact W1 between the N generated samples and the
  first N real ones as points (`dataset`: N samples of the config's own 2-D distribution); prints `w1 <value> ground <g> over ...`.
  --eval_tail REAL.npy|dataset --generate N [--tail_xi X] [--tail_levels K] [--tail_marginal norm|abs]: the tail figures between the
  first N real samples (`dataset` as for --eval_w1) and the N generated ones (EvaluationManager.evaluate_tail: the mean squared
  logarithmic error between their K upper quantiles above the level X, default 0.95 and 100, and the Hill tail index of each set, on
  the norms of the samples or on every scalar); prints `tail msle <v> index real <a> generated <b> xi <x> over <N> generated vs <M>
  real samples`.  Generated 2-D samples are clamped to +-6: keep X below the clamped fraction.  It shares the one generation with the
  other --eval_* flags.
  --eval_prdc REAL.npy --generate N [--nearest_k K]: generate N samples and print the k-nearest-neighbour precision, recall, density
  and coverage (the `prdc` package's compute_prdc) between the first N float32 samples of REAL.npy and them, with f_1_pr and f_1_dc
  (EvaluationManager.evaluate_prdc on the flattened samples; K = 5 neighbours by default).  A feature network is plugged in through
  the Python call (`features=`), not here.
  --eval_fid REAL.npy|STATS.npz --generate N [--save_fid_stats OUT.npz]: generate N samples and print the Frechet distance
  (calculate_frechet_distance on mean / covariance statistics) between the first N float32 samples of REAL.npy -- or the precomputed
  `mu` / `sigma` of STATS.npz -- and them (EvaluationManager.evaluate_fid on the flattened samples, at most 4096 values each; the name
  FID belongs to Inception features, which come in through the Python call's `features=`).  --save_fid_stats writes the real set's
  `mu` / `sigma` (float64) for later runs.  It shares the one generation with the other --eval_* flags.
  --eval_2d --generate N [--dataset NAME] [--dump_dataset OUT.npy]: the reference's whole 2-D evaluation (EvaluationManager.
  evaluate_metrics_2d: wass, mmd, precision, recall, f_1_pr) of N generated samples against N real samples drawn on the device from the
  config's own `data:` description (dlpm_amd/datasets.py; the draw is keyed by --set_seed), so no data file is needed.  --dataset
  overrides data.dataset (gmm_2, gmm_grid, swiss_roll, sas_grid; gmm_2 gets equal weights when the config's weights are another
  mixture's); --dump_dataset writes the N real samples ([N, 1, dim] float32).
  --train EPOCHS [--save OUT.pt] [--ema_rates MU ...] [--max_batch_per_epoch N] [--grad_clip C]: on a 2-D config, first train the net on
  the device (dlpm_amd.TrainingManager: AdamW at optim.lr, the loss settings of training.<method>, batches of training.batch_size from
  the train split drawn from the config's own `data:` description, keyed by --set_seed) and print `epoch <e> loss <mean loss>` per epoch;
  --save writes a checkpoint in the reference's format, which --checkpoint loads.  With --generate N (and --eval_2d ...) the trained
  net -- with --ema_eval the --ema_index-th EMA -- is then evaluated in the same run; without it the run ends after training.
  --units N / --blocks N / --t_embedding_size N: the 2-D toy net's width, depth and time embedding size, as the reference's flags of
  the same names (script_utils.py:92-102); anything but the shipped 64 units runs on the general MFMA forward, which samples and
  evaluates a checkpoint but does not --train.
"""
import argparse
import os
import sys

import numpy as np
import torch

import dlpm_amd
from dlpm_amd.config import sample_shape


def class_labels(spec, num_classes, n):
    """--class_labels: None, 'cycle' (sample i -> i % K) or an integer k (every sample -> k), as an int64 [n] tensor."""
    if spec is None:
        if num_classes is not None:
            raise SystemExit('the net is class-conditional (model.class_cond): give --class_labels cycle|K')
        return None
    if num_classes is None:
        raise SystemExit('--class_labels needs a class-conditional net (model.class_cond: true, data.num_classes: K)')
    if spec == 'cycle':
        return torch.arange(n, dtype=torch.int64) % num_classes
    k = int(spec)
    if not 0 <= k < num_classes:
        raise SystemExit('--class_labels %d outside [0, %d)' % (k, num_classes))
    return torch.full((n,), k, dtype=torch.int64)


def apply_model_arguments(p, a):
    """--blocks / --units / --t_embedding_size into p['model'], as the reference's script_utils.py:92-102 does."""
    if a.blocks is not None:
        p['model']['nblocks'] = a.blocks
    if a.units is not None:
        p['model']['nunits'] = a.units
    if a.t_embedding_size is not None:
        p['model']['time_emb_size'] = a.t_embedding_size
    return p


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--config', required=True, help='config name (dlpm_amd/configs) or path to a reference-schema YAML')
    ap.add_argument('--method', default=None, choices=['dlpm', 'lim'], help='generative method (script_utils.py:6-7)')
    ap.add_argument('--generate', type=int, default=None, help='number of samples (eval.data_to_generate)')
    ap.add_argument('--reverse_steps', type=int, default=None)
    ap.add_argument('--alpha', type=float, default=None)
    ap.add_argument('--non_iso', action='store_true', help='non-isotropic noise (script_utils.py:26-27)')
    ap.add_argument('--scale', default=None, choices=['scale_preserving', 'scale_exploding'], help='script_utils.py:104-105')
    ap.add_argument('--input_scaling', action='store_true', help='script_utils.py:107-108')
    ap.add_argument('--deterministic', action='store_true', help='DLIM sampling')
    ap.add_argument('--clip', action='store_true', help='clip_denoised')
    ap.add_argument('--set_seed', type=int, default=None)
    ap.add_argument('--random_seed', action='store_true')
    ap.add_argument('--batch_size', type=int, default=None, help='eval.batch_size override')
    ap.add_argument('--checkpoint', default=None, help='reference checkpoint (.pt) with model_parameters / ema_models')
    ap.add_argument('--name', default=None, help='experiment name: checkpoints are looked up under <models_dir>/<name>/')
    ap.add_argument('--models_dir', default='models')
    ap.add_argument('--epoch', type=int, default=None, help='checkpointed epoch to load (default: the latest)')
    ap.add_argument('--ema_eval', action='store_true')
    ap.add_argument('--ema_index', type=int, default=0, help='which EMA shadow (order of training.<method>.ema_rates)')
    ap.add_argument('--synthetic_weights', type=int, default=None, metavar='SEED',
                    help='random init with the zero-initialised tensors re-drawn (benchmarks; NOT the reference init)')
    ap.add_argument('--rng', default='philox', choices=['philox', 'reference'])
    ap.add_argument('--conv', default='auto', choices=['auto', 'f4', 'f2', 'igemm'],
                    help='3x3 convolution generation of the UNet (UNetModel.set_conv_policy): auto = fastest per layer '
                         '(Winograd F(4x4,3x3) where it applies, 1.6e-5 of the reference per forward), f2 / igemm = 3e-6 / '
                         '4e-6 at 1.33x / 2.2x the time; never a function of the batch, so chunking does not change a pixel')
    ap.add_argument('--gemm', default='auto', choices=['auto', 'f32', 'bf16x3'],
                    help='matrix pipe of the 1x1 and stride-2 convolutions (UNetModel.set_gemm_policy): bf16x3 = fp32 operands split '
                         'exactly into three bf16 planes, fp32 accumulate (fp32-grade results, the default where the shape admits it); '
                         'f32 = the fp32 MFMA everywhere')
    ap.add_argument('--out', default=None, help='.npy file for the generated samples')
    ap.add_argument('--gen_data_path', default=None,
                    help='directory for <i>.png files (EvaluationManager image dump); images only')
    ap.add_argument('--device_batch', default='auto',
                    help='with --gen_data_path and --rng philox: sample in chunks of at least this many images (pixels do not '
                         'depend on the chunking).  auto (default) = up to 1024, as many as free HBM holds; 0 = eval.batch_size '
                         'chunks exactly as the reference')
    ap.add_argument('--class_labels', default=None, metavar='cycle|K',
                    help='labels of a class-conditional net (model.class_cond): cycle = sample i gets i %% num_classes, an integer k = '
                         'every sample gets k.  With --gen_data_path they are written to labels.npy next to the images')
    ap.add_argument('--eval_loss', default=None, metavar='DATA.npy',
                    help='held-out denoising loss (the reference\'s training objective, forward only) on the float32 [N, C, H, W] / '
                         '[N, 1, F] samples of this file; prints `loss <value> over <N> samples`')
    ap.add_argument('--lploss', type=float, default=None, help='with --eval_loss: 2 (L2, default), 1 (smooth L1), -1 (squared L2)')
    ap.add_argument('--median', type=int, nargs=2, default=None, metavar=('OUTER', 'INNER'),
                    help='with --eval_loss: median-of-means estimator with these Monte-Carlo counts')
    ap.add_argument('--eval_mmd', default=None, metavar='REAL.npy',
                    help='with --generate N: MMD (the reference\'s MMD_loss, 5 Gaussian kernels) between the N generated samples and the '
                         'first N float32 samples of this file; prints `mmd <value> over <N> generated vs <N> real samples`')
    ap.add_argument('--eval_prd', default=None, metavar='REAL.npy',
                    help='with --generate N: PRD precision / recall (the reference\'s compute_precision_recall_curve + compute_f_beta) '
                         'between the first N float32 samples of this file and the N generated samples; prints `prd precision <p> '
                         'recall <r> f_1_pr <f> over <N> generated vs <N> real samples`')
    ap.add_argument('--prd_seed', type=int, default=0, help='with --eval_prd: seed of the k-means++ draws')
    ap.add_argument('--eval_wass', default=None, metavar='REAL.npy',
                    help='with --generate N: the reference\'s Wasserstein figure (compute_wasserstein_distance: histogram earth mover\'s '
                         'distance of the flattened sets) between the first N float32 samples of this file and the N generated samples; '
                         'prints `wass <value> over <N> generated vs <N> real samples`')
    ap.add_argument('--wass_bins', type=int, default=None, help='with --eval_wass: number of bins (default: 250 from 512 samples on, '
                                                                'else numpy\'s auto rule)')
    ap.add_argument('--eval_w1', default=None, metavar='REAL.npy|dataset',
                    help='with --generate N: the exact Wasserstein-1 distance between the N generated samples and the first N float32 '
                         'samples of this file, as points (optimal transport, one bin per point); `dataset` draws the N real samples '
                         'from the config\'s own 2-D data distribution; prints `w1 <value> ground <g> over <N> generated vs <N> real samples`')
    ap.add_argument('--w1_ground', default='l1_mean', choices=('l1_mean', 'euclidean'),
                    help='with --eval_w1: the distance between two points: the mean absolute difference (the reference\'s manual_compute '
                         'cost, default) or the Euclidean norm')
    ap.add_argument('--eval_tail', default=None, metavar='REAL.npy|dataset',
                    help='with --generate N: the tail figures between the first N float32 samples of this file (`dataset`: N samples of '
                         'the config\'s own 2-D data distribution) and the N generated samples: the mean squared logarithmic error '
                         'between their upper quantiles and the Hill tail index of each set; prints `tail msle <v> index real <a> '
                         'generated <b> xi <x> over <N> generated vs <M> real samples`')
    ap.add_argument('--tail_xi', type=float, default=0.95, help='with --eval_tail: the level in [0.5, 1) the tail starts at (default 0.95)')
    ap.add_argument('--tail_levels', type=int, default=100, help='with --eval_tail: the number of quantile levels (default 100)')
    ap.add_argument('--tail_marginal', default='norm', choices=('norm', 'abs'),
                    help='with --eval_tail: the norm of every sample (default) or the absolute value of every scalar')
    ap.add_argument('--eval_prdc', default=None, metavar='REAL.npy',
                    help='with --generate N: k-nearest-neighbour precision / recall / density / coverage (compute_prdc of the prdc '
                         'package) between the first N float32 samples of this file and the N generated samples, flattened; prints '
                         '`prdc precision <p> recall <r> density <d> coverage <c> f_1_pr <f> f_1_dc <f> over <N> generated vs <N> real '
                         'samples`')
    ap.add_argument('--nearest_k', type=int, default=5, help='with --eval_prdc: the number of neighbours (default 5)')
    ap.add_argument('--eval_fid', default=None, metavar='REAL.npy|STATS.npz',
                    help='with --generate N: Frechet distance between the mean / covariance of the first N float32 samples of REAL.npy (or '
                         'the mu / sigma of STATS.npz) and those of the N generated samples, flattened; prints `fid <value> over <N> '
                         'generated vs <N> real samples` (`vs precomputed statistics` for an .npz)')
    ap.add_argument('--save_fid_stats', default=None, metavar='OUT.npz',
                    help='with --eval_fid REAL.npy: write the real set\'s mu / sigma (float64) to this file')
    ap.add_argument('--eval_2d', action='store_true',
                    help='with --generate N on a 2-D config: wass / mmd / PRD figures against N real samples drawn from the config\'s own '
                         'data distribution; prints `eval_2d wass <w> mmd <m> precision <p> recall <r> f_1_pr <f> over <N> generated vs '
                         '<N> real samples`')
    ap.add_argument('--dataset', default=None, metavar='NAME', help='override data.dataset')
    ap.add_argument('--dump_dataset', default=None, metavar='OUT.npy',
                    help='on a 2-D config: write the --generate N real samples drawn from the config\'s data distribution to this file')
    ap.add_argument('--train', type=int, default=None, metavar='EPOCHS', help='train the 2-D toy net for this many epochs first')
    ap.add_argument('--save', default=None, metavar='OUT.pt', help='with --train: write the checkpoint (reference format) to this file')
    ap.add_argument('--ema_rates', type=float, nargs='+', default=None, help='with --train: EMA rates (default: training.<method>.ema_rates)')
    ap.add_argument('--max_batch_per_epoch', type=int, default=None, help='with --train: stop every epoch after this many batches')
    ap.add_argument('--grad_clip', type=float, default=None, help='with --train: gradient-norm clip (default: training.<method>.grad_clip)')
    ap.add_argument('--blocks', type=int, default=None, help='2-D toy net: number of blocks (model.nblocks; script_utils.py:92-93,200)')
    ap.add_argument('--units', type=int, default=None, help='2-D toy net: hidden units (model.nunits, up to 1024; script_utils.py:95-96,201)')
    ap.add_argument('--t_embedding_size', type=int, default=None,
                    help='2-D toy net: time embedding size (model.time_emb_size, up to 1024; script_utils.py:101-102,206)')
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.train is None and (a.save or a.ema_rates or a.max_batch_per_epoch is not None or a.grad_clip is not None):
        raise SystemExit('--save / --ema_rates / --max_batch_per_epoch / --grad_clip belong to --train EPOCHS')
    if a.save_fid_stats and not (a.eval_fid and not a.eval_fid.endswith('.npz')):
        raise SystemExit('--save_fid_stats needs --eval_fid REAL.npy')
    for flag, value in (('--eval_mmd', a.eval_mmd), ('--eval_prd', a.eval_prd), ('--eval_wass', a.eval_wass), ('--eval_prdc', a.eval_prdc),
                        ('--eval_fid', a.eval_fid), ('--eval_2d', a.eval_2d), ('--dump_dataset', a.dump_dataset), ('--eval_w1', a.eval_w1),
                        ('--eval_tail', a.eval_tail)):
        if value and a.gen_data_path:
            raise SystemExit('%s cannot be combined with --gen_data_path' % flag)
        if value and a.generate is None:
            raise SystemExit('%s needs --generate N' % flag)

    p = dlpm_amd.load_config(a.config)
    p['device'] = 'cuda'
    if a.dataset is not None:
        p['data']['dataset'] = a.dataset
        w = p['data'].get('weights')
        if a.dataset.lower() == 'gmm_2' and w is not None and len(w) != 2:
            # the config's weights belong to the mixture it names; gmm_2 has two components
            print('--dataset gmm_2: the config gives %d weights for another mixture; its two components get equal weights' % len(w),
                  file=sys.stderr)
            p['data']['weights'] = None
    if a.method is not None:
        p['method'] = a.method
    apply_model_arguments(p, a)
    m = p['method']
    if a.eval_loss and m == 'lim' and (a.lploss is not None or a.median is not None):
        ap.error('--lploss / --median belong to the DLPM loss; --method lim evaluates training_losses_lim, which has neither')
    if a.alpha is not None:
        p[m]['alpha'] = a.alpha
    if a.non_iso:
        p[m]['isotropic'] = False
    if a.scale is not None:
        p[m]['scale'] = a.scale
    if a.input_scaling:
        p[m]['input_scaling'] = True
    if a.generate is not None:
        assert a.generate <= p['eval']['real_data'], 'cannot generate more data than the number of real data'
        p['eval']['data_to_generate'] = a.generate
    if a.reverse_steps is not None:
        p['eval'][m]['reverse_steps'] = a.reverse_steps
    if a.deterministic:
        p['eval'][m]['deterministic'] = True
    if a.clip:
        p['eval'][m]['clip_denoised'] = True
    if a.batch_size is not None:
        p['eval']['batch_size'] = a.batch_size
    seed = None if a.random_seed else a.set_seed
    if seed is not None:
        torch.manual_seed(seed)
        np.random.seed(seed)

    model = dlpm_amd.init_model_by_parameter(p)
    path = a.checkpoint
    if path is None and a.name is not None:
        path = dlpm_amd.checkpoint.find_checkpoint(p, os.path.join(a.models_dir, a.name), epoch=a.epoch)
    if path:
        epoch, steps = dlpm_amd.checkpoint.load_into(model, path, ema=a.ema_index if a.ema_eval else None)
        print('loaded %s (epoch %s, %s steps%s)' % (path, epoch, steps, ', ema #%d' % a.ema_index if a.ema_eval else ''),
              file=sys.stderr)
    elif a.synthetic_weights is not None:
        dlpm_amd.rerandomize_(model, a.synthetic_weights)
    if a.conv != 'auto':
        if not hasattr(model, 'set_conv_policy'):
            raise SystemExit('--conv applies to the UNet score networks')
        model.set_conv_policy(a.conv)
    if a.gemm != 'auto':
        if not hasattr(model, 'set_gemm_policy'):
            raise SystemExit('--gemm applies to the UNet score networks')
        model.set_gemm_policy(a.gemm)
    method = dlpm_amd.init_method_by_parameter(p, rng=a.rng, seed=seed or 0)
    if a.train is not None:
        if dlpm_amd.is_image_dataset(p['data']['dataset']):
            raise SystemExit('--train trains the 2-D toy net; training of the UNets is out of scope')
        tr = dict((p.get('training') or {}).get(m) or {})
        ema_rates = a.ema_rates if a.ema_rates else tr.get('ema_rates')
        keys = ('clamp_a', 'clamp_eps') if m == 'lim' else ('lploss', 'loss_monte_carlo', 'monte_carlo_outer', 'monte_carlo_inner',
                                                          'clamp_a', 'clamp_eps')
        kw = {k: tr[k] for k in keys if k in tr}
        train_data = dlpm_amd.get_dataset(p, 'cuda', seed or 0)[0]
        tm = dlpm_amd.TrainingManager({'default': model}, dlpm_amd.ToyLoader(train_data, p['training']['batch_size']), method, None,
                                      (p.get('optim') or {}).get('schedule'), None, ema_rates=ema_rates, p=p, seed=seed or 0)
        done = len(tm.epoch_losses)
        tm.train(a.train, max_batch_per_epoch=a.max_batch_per_epoch, grad_clip=a.grad_clip if a.grad_clip is not None else tr.get('grad_clip'),
                 **kw)
        for e, loss in enumerate(tm.epoch_losses[done:]):
            print('epoch %d loss %.9g' % (e + 1, loss))
        if a.save:
            tm.save(a.save)
            print('saved %s (epoch %d, %d steps)' % (a.save, tm.epochs, tm.total_steps), file=sys.stderr)
        if a.ema_eval:
            if not ema_rates:
                raise SystemExit('--ema_eval after --train needs EMA rates (--ema_rates or training.<method>.ema_rates)')
            model = tm.ema_model(a.ema_index)
        else:
            tm.sync()
        if a.generate is None:
            return tm.epoch_losses
    if a.eval_loss:
        data = np.load(a.eval_loss)
        tr = dict((p.get('training') or {}).get(m) or {})      # a reference-schema YAML carries the loss settings of its training run
        keys = ('clamp_a', 'clamp_eps') if m == 'lim' else ('lploss', 'loss_monte_carlo', 'monte_carlo_outer', 'monte_carlo_inner',
                                                          'clamp_a', 'clamp_eps')
        kw = {k: tr[k] for k in keys if k in tr}
        if a.lploss is not None:
            kw['lploss'] = a.lploss
        if a.median is not None:
            kw.update(loss_monte_carlo='median', monte_carlo_outer=a.median[0], monte_carlo_inner=a.median[1])
        labels = class_labels(a.class_labels, getattr(model, 'num_classes', None), len(data))
        ev = dlpm_amd.EvaluationManager(method, None, None, verbose=False)
        loss = ev.evaluate_loss({'default': model}, data, p['eval']['batch_size'], class_labels=labels, **kw)
        print('loss %.9g over %d samples' % (loss, len(data)))
        return loss
    is_image = dlpm_amd.is_image_dataset(p['data']['dataset'])
    labels = class_labels(a.class_labels, getattr(model, 'num_classes', None), p['eval']['data_to_generate'])
    loader = dlpm_amd.ShapeProbe(sample_shape(p))
    if a.eval_2d or a.dump_dataset or a.eval_w1 == 'dataset' or a.eval_tail == 'dataset':
        if is_image:
            raise SystemExit('--eval_2d / --dump_dataset / --eval_w1 dataset / --eval_tail dataset draw the 2-D toy distributions; %s is an image dataset' % p['data']['dataset'])
        loader = dlpm_amd.ToyLoader(dlpm_amd.get_dataset(p, 'cuda', seed or 0)[0], p['eval']['batch_size'])
    gm = dlpm_amd.GenerationManager(method, loader, is_image, **p['eval'][m])
    if a.dump_dataset:
        np.save(a.dump_dataset, gm.load_original_data(p['eval']['data_to_generate']).cpu().numpy())
    if a.eval_2d:
        N = p['eval']['data_to_generate']
        ev = dlpm_amd.EvaluationManager(method, gm, None, verbose=False, is_image=False)
        res = ev.evaluate_metrics_2d({'default': model}, None, N, p['eval']['batch_size'], class_labels=labels, seed=a.prd_seed)
        print('eval_2d wass %.9g mmd %.9g precision %.9g recall %.9g f_1_pr %.9g over %d generated vs %d real samples' % (
            res['wass'], res['mmd'], res['precision'], res['recall'], res['f_1_pr'], N, N))
        if a.out:
            np.save(a.out, res['samples'].cpu().numpy())
        return res
    if a.eval_mmd or a.eval_prd or a.eval_wass or a.eval_prdc or a.eval_fid or a.eval_w1 or a.eval_tail:
        N = p['eval']['data_to_generate']
        ev = dlpm_amd.EvaluationManager(method, gm, None, verbose=False, is_image=is_image)
        value = samples = None
        files = {}

        def real_of(path):                          # every file is loaded once, whichever figures name it
            if path not in files:
                files[path] = np.load(path)
            return files[path]

        def generated():                            # the samples are generated once, the way evaluate_mmd generates them
            s, shape = ev._generate_flat({'default': model}, N, p['eval']['batch_size'], labels, {})
            return s.reshape((N,) + shape)
        if a.eval_mmd:
            value, samples = ev.evaluate_mmd({'default': model}, real_of(a.eval_mmd), N, p['eval']['batch_size'], class_labels=labels,
                                             return_samples=True)
            print('mmd %.9g over %d generated vs %d real samples' % (value, N, N))
        if a.eval_prd:
            if samples is None:
                samples = generated()
            res = ev.evaluate_prd({'default': model}, real_of(a.eval_prd), N, p['eval']['batch_size'], seed=a.prd_seed, samples=samples)
            print('prd precision %.9g recall %.9g f_1_pr %.9g over %d generated vs %d real samples' % (
                res['precision'], res['recall'], res['f_1_pr'], N, N))
            if value is not None:
                res = dict(res, mmd=value)
            value = res
        if a.eval_wass:
            if samples is None:
                samples = generated()
            w = ev.evaluate_wass({'default': model}, real_of(a.eval_wass), N, p['eval']['batch_size'], bins=a.wass_bins, samples=samples)
            print('wass %.9g over %d generated vs %d real samples' % (w, N, N))
            if value is None:
                value = w
            else:
                value = dict(value if isinstance(value, dict) else {'mmd': value}, wass=w)
        if a.eval_prdc:
            if samples is None:
                samples = generated()
            res = ev.evaluate_prdc({'default': model}, real_of(a.eval_prdc), N, p['eval']['batch_size'], nearest_k=a.nearest_k,
                                   samples=samples)
            print('prdc precision %.9g recall %.9g density %.9g coverage %.9g f_1_pr %.9g f_1_dc %.9g over %d generated vs %d real samples'
                  % (res['precision'], res['recall'], res['density'], res['coverage'], res['f_1_pr'], res['f_1_dc'], N, N))
            if value is None:
                value = res
            else:                                       # beside --eval_prd its PRD figures keep their keys; the k-NN ones go under 'prdc'
                value = dict(value if isinstance(value, dict) else {'mmd' if a.eval_mmd else 'wass': value}, prdc=res)
        if a.eval_fid:
            if samples is None:
                samples = generated()
            if a.eval_fid.endswith('.npz'):
                f = ev.evaluate_fid({'default': model}, None, N, p['eval']['batch_size'], real_stats=a.eval_fid, samples=samples)
                print('fid %.9g over %d generated vs precomputed statistics' % (f, N))
            else:
                real = real_of(a.eval_fid)
                f = ev.evaluate_fid({'default': model}, real, N, p['eval']['batch_size'], samples=samples)
                print('fid %.9g over %d generated vs %d real samples' % (f, N, N))
                if a.save_fid_stats:
                    mu, sigma = dlpm_amd.feature_statistics(torch.as_tensor(real)[:N])
                    np.savez(a.save_fid_stats, mu=mu.cpu().numpy(), sigma=sigma.cpu().numpy())
            if value is None:
                value = f
            else:
                value = dict(value if isinstance(value, dict) else {'mmd' if a.eval_mmd else 'wass': value}, fid=f)
        if a.eval_w1:
            if samples is None:
                samples = generated()
            real = None if a.eval_w1 == 'dataset' else real_of(a.eval_w1)
            w = ev.evaluate_w1({'default': model}, real, N, p['eval']['batch_size'], ground=a.w1_ground, samples=samples)
            print('w1 %.9g ground %s over %d generated vs %d real samples' % (w, a.w1_ground, N, N))
            if value is None:
                value = w
            else:
                value = dict(value if isinstance(value, dict) else {'mmd' if a.eval_mmd else 'wass' if a.eval_wass else 'fid': value}, w1=w)
        if a.eval_tail:
            if samples is None:
                samples = generated()
            real = None if a.eval_tail == 'dataset' else real_of(a.eval_tail)
            res = ev.evaluate_tail({'default': model}, real, N, p['eval']['batch_size'], xi=a.tail_xi, levels=a.tail_levels,
                                   marginal=a.tail_marginal, samples=samples)
            print('tail msle %.9g index real %.9g generated %.9g xi %.9g over %d generated vs %d real samples' % (
                res['msle'], res['tail_index_real'], res['tail_index_gen'], a.tail_xi, N, N))
            if value is None:
                value = res
            else:                                       # beside other figures the three go under 'tail'
                value = dict(value if isinstance(value, dict) else
                             {'mmd' if a.eval_mmd else 'wass' if a.eval_wass else 'fid' if a.eval_fid else 'w1': value}, tail=res)
        if a.out:
            np.save(a.out, samples.cpu().numpy())
        return value
    if a.gen_data_path:
        assert is_image, '--gen_data_path dumps images; 2-D data has no image form'
        ev = dlpm_amd.EvaluationManager(method, gm, None, is_image=True, gen_data_path=a.gen_data_path,
                                        device_batch=a.device_batch if a.device_batch == 'auto' else int(a.device_batch))
        r = ev.evaluate_model({'default': model}, data_to_generate=p['eval']['data_to_generate'],
                              batch_size=p['eval']['batch_size'], class_labels=labels)
        print('wrote %d png files to %s' % (r['generated'], r['gen_data_path']))
        return r
    remaining, chunks = p['eval']['data_to_generate'], []
    while remaining > 0:                                    # EvaluationManager.py:181-193
        n = min(p['eval']['batch_size'], remaining)
        done = p['eval']['data_to_generate'] - remaining
        extra = {} if labels is None else {'model_kwargs': {'y': labels[done:done + n]}}
        chunks.append(gm.generate({'default': model}, n, **extra).clone())
        remaining -= n
        print('generated %d, %d to go' % (n, remaining), file=sys.stderr)
    samples = torch.cat(chunks)
    if a.out:
        np.save(a.out, samples.numpy())
    print('samples %s  mean %.4f  min %.4f  max %.4f' % (tuple(samples.shape), samples.mean(), samples.min(), samples.max()))
    return samples


if __name__ == '__main__':
    main()
