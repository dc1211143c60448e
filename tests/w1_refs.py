"""Host mirror of the exact W1 of dlpm_amd/csrc/w1.hip, shared by tests/test_w1_cpu.py, tests/test_gpu_w1.py,
tools/make_w1_fixtures.py and tools/bench_w1.py: the fp64 cost as an explicit loop over d, the quantisation, and the integer
auction round for round, returning the permutation, the prices, and the round and phase counts the kernels must reproduce bit for
bit.  Also the case table of the tests, the recipes of its inputs, and the oracles (scipy's linear_sum_assignment, brute force)."""
import functools
import itertools
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'f26_w1.npz')
GROUNDS = ('l1_mean', 'euclidean')
MAX_TABLE_ROUNDS = 40000

# The case table: name -> (n, D, seed).  Every n of {1, 2, 3, 17, 63, 64, 65, 257} (63 / 64 / 65 are the cost kernels' 64-wide tile
# edge and its neighbours) with every D of {1, 2, 3, 16, 17, 40} (2 | 4 | 16 | 17: the register forms' boundaries and the LDS-panel
# form, 40: a second, partial panel); D = 5 and 8 at n = 17 and 65, the one register form (rows padded to 8 values) that list does not
# reach; one case at 512.  Both grounds run on the same inputs, and every case runs under both.  The seeds are fixed here;
# tools/make_w1_fixtures.py refuses a table whose mirror needs more than MAX_TABLE_ROUNDS rounds anywhere.
NS, DS = (1, 2, 3, 17, 63, 64, 65, 257), (1, 2, 3, 16, 17, 40)
CASES = {'n%d_d%d' % (n, D): (n, D, 1000 * n + D) for n in NS for D in DS}
CASES.update({'n%d_d%d' % (n, D): (n, D, 1000 * n + D) for n in (17, 65) for D in (5, 8)})
CASES['n512_d2'] = (512, 2, 512002)
PAIRS = [(name, g) for name in CASES for g in GROUNDS]      # the (case, ground) pairs the tests run: all of them


def case_inputs(name):
    """x ~ N(0, 1), y ~ 1.2 N(0, 1) + 0.3, float32 [n, D], from the case's seed."""
    n, D, seed = CASES[name]
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, D)).astype(np.float32)
    y = (1.2 * g.standard_normal((n, D)) + 0.3).astype(np.float32)
    return x, y


def costs(x, y, ground):
    """c [n, n] float64: one accumulator per pair, d ascending, every operation rounded on its own; then / D or sqrt."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    assert x.ndim == 2 and x.shape == y.shape and ground in GROUNDS
    D = x.shape[1]
    acc = np.zeros((x.shape[0], y.shape[0]), np.float64)
    for d in range(D):
        diff = x[:, d].astype(np.float64)[:, None] - y[:, d].astype(np.float64)[None, :]
        acc = acc + (np.abs(diff) if ground == 'l1_mean' else diff * diff)
    return acc / np.float64(D) if ground == 'l1_mean' else np.sqrt(acc)


def quantise(c):
    """(q int64 [n, n], e, cmax): e = 23 - floor(log2 cmax), q = rint(c 2^e) (ties to even, as llrint); all 0 when cmax == 0."""
    cmax = float(c.max())
    assert math.isfinite(cmax)
    if cmax == 0.0:
        return np.zeros(c.shape, np.int64), 0, 0.0
    e = 23 - (math.frexp(cmax)[1] - 1)
    return np.rint(np.ldexp(c, e)).astype(np.int64), e, cmax


def auction(q):
    """The integer forward auction with eps-scaling in synchronous rounds on q [n, n]: (perm int32 [n], prices int64 [n], rounds,
    phases).  Benefits a = -q (n + 1); eps_0 = max(1, C // 2), eps_{k+1} = max(1, eps_k // 4), C = qmax (n + 1)."""
    q = np.asarray(q, np.int64)
    n = q.shape[0]
    a = -q * (n + 1)
    C = int(q.max()) * (n + 1)
    eps = max(1, C // 2)
    prices = np.zeros(n, np.int64)
    lowest = np.iinfo(np.int64).min
    rounds = phases = 0
    while True:
        phases += 1
        assigned = np.full(n, -1, np.int64)          # person -> object
        owner = np.full(n, -1, np.int64)             # object -> person
        bidders = np.arange(n)
        while len(bidders):
            rounds += 1
            v = a[bidders] - prices[None, :]
            rows = np.arange(len(bidders))
            j1 = v.argmax(axis=1)                    # the first maximum: lowest j on ties
            w1 = v[rows, j1]
            if n > 1:
                v[rows, j1] = lowest
                w2 = v.max(axis=1)
            else:
                w2 = w1
            bid = prices[j1] + (w1 - w2) + eps
            order = np.lexsort((bidders, -bid, j1))  # by object, then highest bid, then lowest person
            first = np.ones(len(order), bool)
            first[1:] = j1[order][1:] != j1[order][:-1]
            win = order[first]
            objs, persons = j1[win], bidders[win]
            prev = owner[objs]
            assigned[prev[prev >= 0]] = -1
            owner[objs] = persons
            assigned[persons] = objs
            prices[objs] = bid[win]
            bidders = np.flatnonzero(assigned < 0)
        if eps == 1:
            return assigned.astype(np.int32), prices, rounds, phases
        eps = max(1, eps // 4)


def value(c, perm):
    """(1 / n) sum_i c[i, perm[i]], exactly rounded (math.fsum)."""
    n = c.shape[0]
    return math.fsum(c[np.arange(n), perm].tolist()) / n


@functools.lru_cache(maxsize=None)
def mirror(name, ground):
    """Everything the device call must reproduce for table case `name`: a dict of x, y, c, q, e, cmax, perm, prices, rounds, phases,
    integer_cost, w.  Built once per process and shared; treat as read-only."""
    x, y = case_inputs(name)
    return mirror_of(x, y, ground)


def mirror_of(x, y, ground):
    c = costs(x, y, ground)
    q, e, cmax = quantise(c)
    perm, prices, rounds, phases = auction(q)
    n = len(perm)
    return dict(x=x, y=y, c=c, q=q, e=e, cmax=cmax, perm=perm, prices=prices, rounds=rounds, phases=phases,
                integer_cost=int(q[np.arange(n), perm].sum()), w=value(c, perm))


def scipy_optimum(m):
    """(sum, perm) of the optimal assignment of the matrix m by scipy.optimize.linear_sum_assignment."""
    from scipy.optimize import linear_sum_assignment
    r, s = linear_sum_assignment(m)
    assert (r == np.arange(m.shape[0])).all()
    return m[r, s], s


def brute_optimum(m):
    """The least sum_i m[i, s(i)] over ALL permutations s (n <= 7): an oracle that shares nothing with scipy.  Exact for integer m;
    for float m the sums are exactly rounded."""
    n = m.shape[0]
    assert n <= 7
    exact = np.issubdtype(m.dtype, np.integer)
    best = None
    for s in itertools.permutations(range(n)):
        terms = [m[i, s[i]] for i in range(n)]
        t = int(sum(int(v) for v in terms)) if exact else math.fsum(float(v) for v in terms)
        best = t if best is None or t < best else best
    return best


def w_bound(e, n, cmax):
    """0 <= W - W_opt <= 2^-e + n 2^-52 cmax: every cost is within 2^-e / 2 of q 2^-e, plus the fp64 summation."""
    return math.ldexp(1.0, -e) + n * 2.0 ** -52 * cmax


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(FIXTURE)
    return {k: z[k] for k in z.files}
