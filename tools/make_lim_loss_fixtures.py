#!/usr/bin/env python3
"""Generate the F22 fixtures (tests/golden/f22_limloss_<case>.npz) by IMPORTING the reference: its own training_losses with LIM=True
(dlpm/methods/GenerativeLevyProcess.py:581-609, :680-709; dlpm/methods/LIM/functions/loss.py:12-41) on a recording model, with every
draw and every intermediate stored.

Runs only where the reference is (DLPM_REFERENCE, as tools/make_fixtures.py, whose import stubs and helpers it shares by importing
that module).  Nothing from the reference is copied.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_lim_loss_fixtures.py [case ...]

Stored per case: x_start, t, the draws a (as drawn, [B]; absent at alpha = 2), z, e, the reference's x_coeff, sigma, x_t, score, the
model output, the scalar loss, meta = [B, alpha, clamp_eps or -1], seed, and the weight digest where a net is used.
np.random.seed / torch.manual_seed(seed) right before the call; x_start = 0.5 * N(0, 1) from a generator of its own.

Asserted at recording time (the tests rest on both):
  * score == -(e / float32(alpha)) bit for bit (-e at alpha = 2);
  * the scalar loss, F.smooth_l1_loss(..., reduction='mean') over all B * D elements, equals the fp64 mean of the per-sample
    means to 2e-7 relative.
Seeds: one per case, chosen so that the clamp of a clamped case bites where the case is large enough for that to be likely."""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _bytecode_dirs():
    root = os.environ.get('DLPM_REFERENCE', '/root/reference')
    return {r for r, _, _ in os.walk(root) if '__pycache__' in r}


_BYTECODE_BEFORE = _bytecode_dirs()

from make_fixtures import (REF, GenerativeLevyProcess, SynthModel, make_unet, ref_mlp, rerandomize, save, weight_digest)  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

import dlpm.methods.LIM.functions.loss as ref_loss  # noqa: E402
import bem.datasets.Distributions as ref_dist  # noqa: E402

UNETS = {'tiny': (3, 32, [1, 2], [2], 4, 1, 16), 'mnist': (1, 32, [1, 2, 2, 2], [2, 4], 4, 2, 32)}     # as f6 / f17

# (case, net, shape, alpha, clamp_eps, seed)
CASES = [
    ('mlp', 'mlp', [32, 1, 2], 1.8, None, 13),
    ('mlp_gauss', 'mlp', [32, 1, 2], 2.0, None, 13),
    ('synth_odd', 'synth', [3, 1, 3, 5], 1.5, 20, 45),          # D = 15: the scalar path; 7 elements clamped under this seed
    ('synth_long', 'synth', [5, 3, 20, 20], 1.7, None, 13),     # D = 1200: more than one pass of a 256-thread workgroup
    ('tiny', 'tiny', [2, 3, 16, 16], 1.8, 50, 319),             # one element clamped under this seed
    ('tiny_b1', 'tiny', [1, 3, 16, 16], 1.8, None, 13),
    ('mnist', 'mnist', [4, 1, 32, 32], 1.7, None, 13),
]


class Rec(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x, t):
        self.x_in, self.t_in = x.clone(), t.clone()
        self.out = self.net(x, t)
        return self.out


def net_of(kind):
    if kind == 'synth':
        return SynthModel(), None
    if kind == 'mlp':
        p = yaml.safe_load(open(os.path.join(REF, 'dlpm/configs/2d_data.yml')))
        p['device'] = 'cpu'
        torch.manual_seed(1)
        net = ref_mlp.MLPModel(p).eval()          # default init under manual_seed(1), as f6 / f17
    else:
        in_ch, mc, mult, attn, heads, res, _ = UNETS[kind]
        torch.manual_seed(1234)
        net = make_unet(in_ch, mc, mult, attn, heads, res).eval()
        rerandomize(net, 4321)
    return net, np.frombuffer(bytes.fromhex(weight_digest(net)), dtype=np.uint8)


def record(name, kind, shape, alpha, clamp_eps, seed):
    net, digest = net_of(kind)
    B = shape[0]
    x_start = 0.5 * torch.randn(shape, generator=torch.Generator().manual_seed(220))
    meth = GenerativeLevyProcess(alpha=alpha, device='cpu', reverse_steps=100, rescale_timesteps=True, LIM=True)
    rec, got = Rec(net), {}
    o_levy, o_randn, o_randn_like, o_rand, o_sl1 = (ref_dist.gen_skewed_levy, torch.randn, torch.randn_like, torch.rand,
                                                     ref_loss.F.smooth_l1_loss)
    o_gen, o_std, o_coeff = meth.dlpm.gen_eps.generate, meth.sde.marginal_std, meth.sde.diffusion_coeff

    def levy(*a, **k):
        got['a'] = o_levy(*a, **k).clone()
        return got['a']

    def randn(*a, **k):
        got['z'] = o_randn(*a, **k).clone()
        return got['z']

    def randn_like(*a, **k):
        got['z'] = o_randn_like(*a, **k).clone()
        return got['z']

    def rand(*a, **k):
        got['u'] = o_rand(*a, **k).clone()
        return got['u']

    def gen(*a, **k):
        got['e'] = o_gen(*a, **k).clone()
        return got['e']

    def std(t):
        got['t'], got['sigma'] = t.clone(), o_std(t).clone()
        return got['sigma']

    def coeff(t):
        got['x_coeff'] = o_coeff(t).clone()
        return got['x_coeff']

    def sl1(output, score, **k):
        got['output'], got['score'] = output.clone(), score.clone()
        return o_sl1(output, score, **k)
    ref_dist.gen_skewed_levy, torch.randn, torch.randn_like, torch.rand, ref_loss.F.smooth_l1_loss = levy, randn, randn_like, rand, sl1
    meth.dlpm.gen_eps.generate, meth.sde.marginal_std, meth.sde.diffusion_coeff = gen, std, coeff
    try:
        np.random.seed(seed)
        torch.manual_seed(seed)
        loss = meth.training_losses({'default': rec}, x_start, clamp_eps=clamp_eps)['loss']
    finally:
        ref_dist.gen_skewed_levy, torch.randn, torch.randn_like, torch.rand, ref_loss.F.smooth_l1_loss = (o_levy, o_randn, o_randn_like,
                                                                                                         o_rand, o_sl1)
    e = got['e'] if alpha != 2.0 else got['z']
    extra = {}
    if alpha != 2.0:
        a = got['a'].reshape(B, -1)
        assert bool((a == a[:, :1]).all())
        extra['a'] = a[:, 0]
    if digest is not None:
        extra['digest'] = digest
    # the two facts the tests rest on
    want_score = -e if alpha == 2.0 else -(e / np.float32(alpha))
    assert torch.equal(got['score'], want_score), '%s: score is not -(e / float32(alpha)) bit for bit' % name
    d = (got['output'].double() - got['score'].double()).reshape(B, -1)
    per = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5).mean(dim=1)
    rel = abs(float(loss) - float(per.mean())) / abs(float(per.mean()))
    assert rel <= 2e-7, '%s: loss differs from the fp64 mean of per-sample means by %.3g relative' % (name, rel)
    assert torch.equal(rec.x_in, x_start * got['x_coeff'].view(-1, *([1] * (len(shape) - 1))) + e * got['sigma'].view(-1, *([1] * (len(shape) - 1))))
    assert torch.equal(rec.t_in, got['t']) and torch.equal(got['t'], got['u'] * (meth.sde.T - 1e-5) + 1e-5)
    clamped = 0 if clamp_eps is None else int((e.abs() == clamp_eps).sum())
    save('f22_limloss_' + name, x_start=x_start, t=got['t'], z=got['z'], e=e, x_coeff=got['x_coeff'], sigma=got['sigma'], x_t=rec.x_in,
         score=got['score'], output=rec.out, loss=loss, seed=np.array(seed),
         meta=np.array([B, alpha, -1 if clamp_eps is None else clamp_eps]), **extra)
    print('   %-12s loss %.6f   loss vs fp64 mean of means %.2g   clamped elements %d' % (name, float(loss), rel, clamped))


if __name__ == '__main__':
    which = sys.argv[1:]
    with torch.no_grad():
        for c in CASES:
            if not which or c[0] in which:
                record(*c)
    assert _bytecode_dirs() <= _BYTECODE_BEFORE, 'bytecode leaked into the reference tree'
