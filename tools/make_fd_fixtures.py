#!/usr/bin/env python3
"""Write tests/golden/f21_fd.npz, the fixture family of the Frechet distance (tests/test_fd_cpu.py holds the recipes of the rows, the
oracle `np_fd` and the error model).  Per case: the oracle's fd and its four terms, `ref_fd` = np.cov + calculate_frechet_distance
RUN FROM THE REFERENCE (--reference DIR, the checkout that holds bem/evaluate/fid_score.py) and ref_dev = |ref_fd - fd|, scale =
tr sigma1 + tr sigma2, z = the null directions, the seed and the recipe, and the rows themselves up to F = 64.

fid_score.py imports the `prdc` package (and torchvision, PIL, ...) at module level, which need not be installed: an empty stand-in
module goes into sys.modules for each one that is missing (only calculate_frechet_distance is called, which needs numpy and scipy).
Usage: python tools/make_fd_fixtures.py --reference /path/to/reference"""
import argparse
import importlib
import inspect
import os
import sys
import types

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)


class _StandIn(types.ModuleType):
    """An empty module whose every attribute is another stand-in: enough for `import a.b as c` and `from a import b`."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return _StandIn(self.__name__ + '.' + name)

    def __call__(self, *a, **k):
        return self

    def __mro_entries__(self, bases):
        return (object,)


def reference_function(path, tries=32):
    """calculate_frechet_distance of the reference.  Whatever fid_score.py imports at module level and this machine lacks (prdc,
    torchvision, ...) is replaced by a stand-in and named on stderr; numpy and scipy, which the function itself uses, must be real."""
    sys.path.insert(0, os.path.abspath(path))
    for _ in range(tries):
        try:
            mod = importlib.import_module('bem.evaluate.fid_score')
            break
        except ModuleNotFoundError as e:
            assert e.name and e.name.split('.')[0] not in ('numpy', 'scipy', 'bem'), e
            print('stand-in for the missing module %s' % e.name, file=sys.stderr)
            sys.modules[e.name] = _StandIn(e.name)
    else:
        raise SystemExit('fid_score.py still does not import')
    assert mod.np is np and not isinstance(mod.linalg, _StandIn)
    return mod.calculate_frechet_distance


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'f21_fd.npz'))
    a = ap.parse_args()
    import test_fd_cpu as t
    ref = reference_function(a.reference)
    cases = [('gauss',) + c for c in t.FULL_CASES] + [('gauss',) + t.NULL_GAUSS, ('const',) + t.NULL_CONST, ('hadamard',) + t.HADAMARD]
    out = {'names': np.array([t.case_name(*c) for c in cases])}
    doc = inspect.getdoc(t.rows_of)
    for kind, n1, n2, F in cases:
        name, seed = t.case_name(kind, n1, n2, F), t.seed_of(kind, n1, n2, F)
        real, fake = t.rows_of(kind, seed, n1, n2, F)
        o = t.np_fd(real, fake)
        ref_fd = float(np.real(ref(*t.np_stats(real), *t.np_stats(fake))))
        out[name + '.meta'] = np.array([n1, n2, F, seed, t.KINDS[kind]], np.int64)
        out[name + '.fd'] = np.float64(o['fd'])
        out[name + '.terms'] = np.array([o['mean_term'], o['tr1'], o['tr2'], o['tr_sqrt']])
        out[name + '.ref_fd'] = np.float64(ref_fd)
        out[name + '.ref_dev'] = np.float64(abs(ref_fd - o['fd']))
        out[name + '.scale'] = np.float64(o['tr1'] + o['tr2'])
        out[name + '.z'] = np.int64(o['z'])
        out[name + '.digest'] = np.array([real.astype(np.float64).sum(), fake.astype(np.float64).sum()])
        out[name + '.recipe'] = np.array('%s (tests/test_fd_cpu.py rows_of): %s' % (kind, doc))
        if F <= t.STORED_ROWS_MAX_F:
            out[name + '.real'], out[name + '.fake'] = real, fake
        bound = t.bound_of(F, abs(ref_fd - o['fd']), o['tr1'] + o['tr2'], o['z'], o['tr1'], o['tr2'])
        print('%-22s fd %.17g  ref_dev %.3g  z %d  scale %.6g  bound %.3g' % (name, o['fd'], abs(ref_fd - o['fd']), o['z'],
                                                                           o['tr1'] + o['tr2'], bound))
    np.savez_compressed(a.out, **out)
    print('wrote %s (%d bytes)' % (a.out, os.path.getsize(a.out)))


if __name__ == '__main__':
    main()
