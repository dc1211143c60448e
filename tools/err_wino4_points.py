#!/usr/bin/env python3
"""Which interpolation points for F(4x4,3x3)?  (round 4, VERDICT r03 next #1b)

The kernel's error is the fp32 rounding of the K-loop's Winograd-domain partial sums (tools/err_wino4_emulation.py), whose size the
point set fixes.  Diagonal rescalings of G / B^T / A^T are (to first order) irrelevant in floating point -- scaling V by s and U
by 1/s leaves every relative rounding error where it was -- so the knob is the points themselves.  The family {0, +-a, +-b, inf}
keeps the kernel's VALU count: B^T rows (d4 - b^2 d2) +- a (d3 - b^2 d1), (d4 - a^2 d2) +- b (d3 - a^2 d1), the even/odd sharing of
A^T; with a = 1 not one instruction changes, only constants.  Asymmetric sets (Barabasz et al.: {0, -1, 1, 1/2, -2, inf} ...) lose
the even/odd sharing (+4 VALU per 1-D input transform of 12) and are listed for reference only.

NumPy emulation as err_wino4_emulation.py: Cin channels accumulated sequentially in fp32 (one rounding per product, the
pessimistic model of the MFMA chain), transforms in fp32 with one rounding per term, U = G g G^T in fp64 rounded once.

    python tools/err_wino4_points.py > profiles/r04/err_wino4_points.txt

--family 42: the (4, 2) family of the sub-pixel Upsample kernel (k_conv3x3_wino4sp) -- one parity class of a nearest-x2 upsampling 3x3
convolution is a 2x2 convolution of the low-res image (effective filter = taps summed in fp64), run as F(4x4,2x2) on FIVE points: all
finite {0, +-a, +-b} (B^T = rows 0..4 of the (4, 3) matrix, A^T without the inf column), or four finite points + inf.  Same emulation.

    python tools/err_wino4_points.py --family 42 > profiles/wino4_subpixel/err_wino4_points_42.txt"""
import itertools
import sys
import numpy as np
from numpy.polynomial import polynomial as Pl

f32, f64 = np.float32, np.float64


def toom_cook(points, m=4, r=3):
    """A^T [m x n], G [n x r], B^T [n x n] for the finite `points` plus infinity (n = m + r - 1 = len(points) + 1)."""
    n = m + r - 1
    assert len(points) == n - 1
    p = np.array(points, f64)
    AT = np.zeros((m, n))
    G = np.zeros((n, r))
    BT = np.zeros((n, n))
    for j in range(n - 1):
        AT[:, j] = p[j] ** np.arange(m)
        Nj = np.prod([p[j] - p[l] for l in range(n - 1) if l != j])
        G[j] = p[j] ** np.arange(r) / Nj
        BT[j, :n - 1] = Pl.polyfromroots([p[l] for l in range(n - 1) if l != j])
    AT[m - 1, n - 1] = 1
    G[n - 1, r - 1] = 1
    BT[n - 1] = Pl.polyfromroots(p)
    # sign / ordering convention check happens numerically in selfcheck()
    return AT, G, BT


def toom_cook_finite(points, m=4, r=2):
    """A^T [m x n], G [n x r], B^T [n x n] on n = m + r - 1 finite points."""
    n = m + r - 1
    assert len(points) == n
    p = np.array(points, f64)
    AT, G, BT = np.zeros((m, n)), np.zeros((n, r)), np.zeros((n, n))
    for j in range(n):
        AT[:, j] = p[j] ** np.arange(m)
        G[j] = p[j] ** np.arange(r) / np.prod([p[j] - p[l] for l in range(n) if l != j])
        BT[j] = Pl.polyfromroots([p[l] for l in range(n) if l != j])
    return AT, G, BT


def run42(mats, d, e, ref, Cin, Cout, N):
    AT, G, BT = mats
    rng = np.random.default_rng(1)
    dd, gg = rng.standard_normal(5), rng.standard_normal(2)
    assert np.abs(AT @ ((G @ gg) * (BT @ dd)) - np.array([dd[i:i + 2] @ gg for i in range(4)])).max() < 1e-9
    U32 = np.einsum('ia,ocab,jb->ocij', G, e, G).astype(f32)
    V = seq_transform(d.astype(f32), BT, 5)
    M = np.zeros((N, Cout, 5, 5), f32)
    for c in range(Cin):
        M = (M + V[:, None, c] * U32[None, :, c]).astype(f32)
    err = seq_transform(M, AT, 4) - ref
    return np.abs(err).max(), np.sqrt((err ** 2).mean())


def main42():
    Cin, Cout, N = 256, 16, 64
    sym = [(0.6875, 1.5), (1, 2), (0.5, 1.25), (0.5, 1), (0.75, 1.5), (0.625, 1.25), (1, 1.5), (2 ** -0.5, 2 ** 0.5), (0.5, 1.5), (0.75, 1.25)]
    sets = [('{0, +-%g, +-%g}' % ab, toom_cook_finite([0, ab[0], -ab[0], ab[1], -ab[1]])) for ab in sym]
    for pts in ([0, 1, -1, 2], [0, 0.6875, -0.6875, 1.5], [0, 1, -1, 0.5], [0, 0.5, -0.5, 1.5]):
        sets.append(('{%s, inf}' % ', '.join('%g' % v for v in pts), toom_cook(pts, 4, 2)))
    rows = [[name, [], []] for name, _ in sets]
    for seed in (0, 1):
        rng = np.random.default_rng(seed)
        z = rng.standard_normal((N, Cin, 5, 5))
        d = z / (1 + np.exp(-z))
        g = rng.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)
        e = np.zeros((Cout, Cin, 2, 2))          # class (0, 0): rows (g0, g1 + g2), columns likewise
        for i in range(3):
            for j in range(3):
                e[:, :, min(i, 1), min(j, 1)] += g[:, :, i, j]
        d64 = d.astype(f32).astype(f64)
        ref = np.zeros((N, Cout, 4, 4))
        for i in range(4):
            for j in range(4):
                ref[:, :, i, j] = np.einsum('ncab,ocab->no', d64[:, :, i:i + 2, j:j + 2], e)
        for k, (name, mats) in enumerate(sets):
            mx, rms = run42(mats, d, e, ref, Cin, Cout, N)
            rows[k][1].append(mx)
            rows[k][2].append(rms)
        yr = np.sqrt((ref ** 2).mean())
    print('F(4x4,2x2) point sets (one parity class of an upsampling 3x3); %d channels, silu(N(0,1)) inputs, |Y| rms %.3f; fp32 emulation against the float64 convolution, two seeds' % (Cin, yr))
    print('%-30s %-10s %-10s %-10s %-10s' % ('points', 'max s0', 'max s1', 'rms s0', 'rms s1'))
    for name, mx, rms in rows:
        print('%-30s %-10.3g %-10.3g %-10.3g %-10.3g   [rms x%.2f vs %s]' % (name, mx[0], mx[1], rms[0], rms[1], np.mean(rms) / np.mean(rows[0][2]), rows[0][0]))


def selfcheck(AT, G, BT):
    rng = np.random.default_rng(1)
    d, g = rng.standard_normal(6), rng.standard_normal(3)
    y = AT @ ((G @ g) * (BT @ d))
    ref = np.array([d[i:i + 3] @ g for i in range(4)])
    return np.abs(y - ref).max()


def seq_transform(M, T, n_out):
    T32 = T.astype(f32)
    Z = np.zeros(M.shape[:2] + (n_out, M.shape[3]), f32)
    for i in range(n_out):
        acc = np.zeros(M.shape[:2] + (M.shape[3],), f32)
        for a in range(T.shape[1]):
            if T32[i, a] != 0:
                acc = (acc + T32[i, a] * M[:, :, a, :]).astype(f32)
        Z[:, :, i, :] = acc
    Y = np.zeros(M.shape[:2] + (n_out, n_out), f32)
    for j in range(n_out):
        acc = np.zeros(M.shape[:2] + (n_out,), f32)
        for b in range(T.shape[1]):
            if T32[j, b] != 0:
                acc = (acc + T32[j, b] * Z[:, :, :, b]).astype(f32)
        Y[:, :, :, j] = acc
    return Y


def run(points, d, g, ref, Cin, Cout, N):
    AT, G, BT = toom_cook(points)
    assert selfcheck(AT, G, BT) < 1e-9, points
    U32 = np.einsum('ia,ocab,jb->ocij', G, g, G).astype(f32)
    V = seq_transform(d.astype(f32), BT, 6)
    M = np.zeros((N, Cout, 6, 6), f32)
    for c in range(Cin):
        M = (M + V[:, None, c] * U32[None, :, c]).astype(f32)
    Y = seq_transform(M, AT, 4)
    e = Y - ref
    # size of the Winograd-domain sums relative to the result: sum_ij |A_i||A_j| rms(M_ij) / rms(Y)
    amp = np.einsum('i,j,ij->', np.abs(AT).sum(0), np.abs(AT).sum(0), np.sqrt((M.astype(f64) ** 2).mean((0, 1)))) / np.sqrt((ref ** 2).mean())
    return np.abs(e).max(), np.sqrt((e ** 2).mean()), amp


def main():
    Cin, Cout, N = 256, 16, 64
    rows = []
    for seed in (0, 1):
        rng = np.random.default_rng(seed)
        z = rng.standard_normal((N, Cin, 6, 6))
        d = z / (1 + np.exp(-z))
        g = rng.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)
        d64 = d.astype(f32).astype(f64)
        ref = np.zeros((N, Cout, 4, 4))
        for i in range(4):
            for j in range(4):
                ref[:, :, i, j] = np.einsum('ncab,ocab->no', d64[:, :, i:i + 3, j:j + 3], g)
        sym = [(1, 2), (1, 0.5), (0.5, 2), (1, 1.5), (1, 0.75), (0.5, 1.5), (0.75, 1.5), (1, 3), (0.5, 1), (0.5, 0.75), (0.75, 1.25),
               (2 ** -0.5, 2 ** 0.5), (0.6, 1.2), (0.5, 1.25), (0.625, 1.25), (0.75, 2), (0.875, 1.75), (1, 1.75), (1, 1.25), (0.75, 1)]
        sets = [('{0, +-%g, +-%g, inf}' % ab, [0, ab[0], -ab[0], ab[1], -ab[1]], 'same VALU' if ab[0] == 1 else 'same VALU in the loop, +3 in the epilogue') for ab in sym]
        sets += [('{0, 1, -1, 1/2, -2, inf}', [0, 1, -1, 0.5, -2], 'asymmetric: +4 VALU per 1-D input transform'),
                 ('{0, 1, -1, 2, -1/2, inf}', [0, 1, -1, 2, -0.5], 'asymmetric'),
                 ('{0, 1, -1, 1/2, -3, inf}', [0, 1, -1, 0.5, -3], 'asymmetric'),
                 ('{0, 1, -1, 1/2, -3/2, inf}', [0, 1, -1, 0.5, -1.5], 'asymmetric')]
        for k, (name, pts, note) in enumerate(sets):
            mx, rms, amp = run(pts, d, g, ref, Cin, Cout, N)
            if seed == 0:
                rows.append([name, note, [mx], [rms], amp])
            else:
                rows[k][2].append(mx)
                rows[k][3].append(rms)
        yr = np.sqrt((ref ** 2).mean())
    print('F(4x4,3x3) point sets; %d channels, silu(N(0,1)) inputs, |Y| rms %.3f; fp32 emulation against the float64 direct convolution, two seeds' % (Cin, yr))
    print('%-30s %-10s %-10s %-10s %-10s %-8s %s' % ('points', 'max s0', 'max s1', 'rms s0', 'rms s1', 'amp', 'cost'))
    base = rows[0]
    for name, note, mx, rms, amp in rows:
        print('%-30s %-10.3g %-10.3g %-10.3g %-10.3g %-8.1f %s   [rms x%.2f vs {0,+-1,+-2,inf}]' % (name, mx[0], mx[1], rms[0], rms[1], amp, note, np.mean(rms) / np.mean(base[3])))


if __name__ == '__main__':
    main42() if sys.argv[1:] == ['--family', '42'] else main()
