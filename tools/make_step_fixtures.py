#!/usr/bin/env python3
"""Generate the F24 fixtures of the step-level API by IMPORTING the reference:

  tests/golden/f24_two_rv.npz             DLPM.get_two_rv_loss_elements (dlpm/methods/dlpm.py:308-370) with every draw recorded
  tests/golden/f24_step_signatures.json   the public methods of the reference's DLPM and GenerativeLevyProcess with their
                                          parameter names and defaults (data only)

Runs only where the reference is (DLPM_REFERENCE, as tools/make_fixtures.py, whose import stubs and helpers it shares by importing
that module).  Nothing from the reference is copied.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_step_fixtures.py

F24 cases: shapes [5,3,2,2] (D = 12: the 16-byte path) and [4,1,3] (D = 3: the scalar path), T = 12, t = [1,2,5,11,1] (its first B
entries), alpha in {1.7, 2.0}.  The reference draws inside the call -- gen_a.generate twice (a_t_0 before it is zeroed where t == 1,
then a_t_1), torch.randn_like once -- so the generators are wrapped and the draws stored as drawn: a0, a1 as [B] (isotropic: the
value is the same over a sample, asserted), z as [B, ...].  Stored per case <tag> = s<B>_a<alpha>: x0, t, a0, a1, z, the five outputs
x_t, eps_t, m_tilde, Sigma_tilde, lambda, the three primed constants Sigma_prime_t_1, Sigma_prime_t, Gamma_prime (all per-sample
ones as [B], asserted constant over a sample), sqrt_Sigma_prime_t = Sigma_prime_t ** (1/2) as the recording torch build evaluates it
(within 1 ulp of the correctly rounded root but not always equal to it: tests/test_gpu_loss.py) and the schedule g, bg, s, bs.
np.random.seed / torch.manual_seed(seed) right before the call; x0 = N(0, 1) from a generator of its own."""
import inspect
import json
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _bytecode_dirs():
    root = os.environ.get('DLPM_REFERENCE', '/root/reference')
    return {r for r, _, _ in os.walk(root) if '__pycache__' in r}


_BYTECODE_BEFORE = _bytecode_dirs()

from make_fixtures import DLPM, OUT, GenerativeLevyProcess, save  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

T = 12
T_STEPS = [1, 2, 5, 11, 1]
SHAPES = [[5, 3, 2, 2], [4, 1, 3]]
ALPHAS = [1.7, 2.0]
SEED = 24


def per_sample(v, B):
    """[B, ...] constant over each sample -> [B]."""
    v = v.reshape(B, -1)
    assert bool((v == v[:, :1]).all() | (v != v).all()), 'a per-sample quantity varies inside a sample'
    return v[:, 0].clone()


def two_rv():
    arrs = {}
    for shape in SHAPES:
        for alpha in ALPHAS:
            B = shape[0]
            d = DLPM(alpha, 'cpu', T)
            x0 = torch.randn(shape, generator=torch.Generator().manual_seed(240 + B))
            t = torch.tensor(T_STEPS[:B])
            got = {'a': []}
            o_gen, o_randn_like, o_prime = d.gen_a.generate, torch.randn_like, d.compute_two_rv_prime_constants

            def gen(*a, **k):
                v = o_gen(*a, **k)
                got['a'].append(v.clone())          # before a_t_0 is zeroed in place where t == 1
                return v

            def randn_like(*a, **k):
                got['z'] = o_randn_like(*a, **k).clone()
                return got['z']

            def prime(*a, **k):
                got['prime'] = tuple(v.clone() for v in o_prime(*a, **k))
                return got['prime']
            d.gen_a.generate, torch.randn_like, d.compute_two_rv_prime_constants = gen, randn_like, prime
            try:
                np.random.seed(SEED)
                torch.manual_seed(SEED)
                x_t, eps_t, m_tilde, Sigma_tilde, lam = d.get_two_rv_loss_elements(t, x0)
            finally:
                torch.randn_like = o_randn_like
            assert len(got['a']) == 2
            tag = 's%d_a%s_' % (B, str(alpha).replace('.', 'p'))
            sp1, sp, gam = got['prime']
            out = dict(x0=x0, t=t.to(torch.int32), a0=per_sample(got['a'][0], B), a1=per_sample(got['a'][1], B), z=got['z'], x_t=x_t,
                       eps_t=eps_t, m_tilde=m_tilde, Sigma_tilde=per_sample(Sigma_tilde, B), Sigma_prime_t_1=per_sample(sp1, B),
                       Sigma_prime_t=per_sample(sp, B), Gamma_prime=per_sample(gam, B), g=d.gammas, bg=d.bargammas, s=d.sigmas,
                       bs=d.barsigmas)
            out['lambda'] = per_sample(lam, B)
            out['sqrt_Sigma_prime_t'] = per_sample(sp ** (1 / 2), B)
            ieee = np.sqrt(out['Sigma_prime_t'].numpy().astype(np.float64)).astype(np.float32)
            print('   %-10s the recorded root is the correctly rounded one for %d of %d samples' % (
                tag, int((out['sqrt_Sigma_prime_t'].numpy() == ieee).sum()), B))
            # the facts the tests rest on: t == 1 gives Sigma_tilde = 0 and lambda = +inf; the draws there were not zero
            one = t == 1
            assert bool((out['Sigma_tilde'][one] == 0).all()) and bool(torch.isinf(out['lambda'][one]).all())
            assert bool((out['a0'] > 0).all()) and bool(torch.isfinite(out['lambda'][~one]).all())
            for k, v in out.items():
                arrs[tag + k] = v
            print('   %-10s a0 %s' % (tag, out['a0'].numpy()))
    save('f24_two_rv', meta=np.array([T, SEED]), **arrs)


def signatures():
    doc = {}
    for cls in (DLPM, GenerativeLevyProcess):
        methods = {}
        for name, fn in inspect.getmembers(cls, inspect.isfunction):
            if name.startswith('_') and name != '__init__':
                continue
            params = []
            for p in list(inspect.signature(fn).parameters.values())[1:]:          # without self
                d = p.default
                if d is inspect.Parameter.empty:
                    params.append([p.name])
                else:
                    params.append([p.name, d if isinstance(d, (bool, int, float, str, type(None))) else repr(d)])
            methods[name] = params
        doc[cls.__name__] = methods
    path = os.path.join(OUT, 'f24_step_signatures.json')
    with open(path, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote f24_step_signatures.json: %s' % {k: len(v) for k, v in doc.items()})


if __name__ == '__main__':
    with torch.no_grad():
        two_rv()
    signatures()
    assert _bytecode_dirs() <= _BYTECODE_BEFORE, 'bytecode leaked into the reference tree'
