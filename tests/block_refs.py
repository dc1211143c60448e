"""Float64 references, the judge and the seeded cases of the fused whole-block kernels (k_resblock_small, k_resblock_wino4_img,
k_resblock_wino4_img16, k_attnblock_small, k_attnblock16).  No GPU here: tests/test_block_refs_cpu.py checks this module on the CPU,
tests/test_gpu_fused_blocks.py launches the kernels on what it builds.

References.  res_block64 / attn_block64 evaluate the block in torch.float64 from the very tensors the kernel receives (fp32 inputs and
weights, widened), GroupNorm written out as (x - mean) * rstd with min(32, C) groups and eps 1e-5.  affine_floor64 is the same
block in float64 except that every GroupNorm is x * A + B with the exact float64 per-(image, channel) A and B rounded to fp32 -- the
coefficient form all five kernels use (for GroupNorm-2 the kernels fold the scale-shift row in: A = gamma rstd (1 + scale),
B = (beta - mean gamma rstd) (1 + scale) + shift; the floor folds it the same way).  Its distance from the reference is an error no
implementation of that form can avoid; it matters where |mean| >> std (test_gpu_gn_stats.py, CANCEL_CHAIN_BOUND).

The judge.  judge(got, want64, ref32, floor64) = max|got - want64| / max(max|ref32 - want64|, max|floor64 - want64|): the kernel's
error in units of the error of the same block in plain fp32 torch on the CPU (oracle.nets, same inputs), or of the form floor where
that is larger.  The code under test does not appear in its own bound.  A non-finite output gives inf.
"""
import functools
import hashlib
import math

import torch
import torch.nn.functional as F

import small_block_weights as sbw
from oracle import nets

M_CAP = 8.0      # no per-kernel bound on the judge's ratio may exceed this (twice the worst conceivable benign ratio)
# kernel -> (bound of the benign and sharp cases, bound of the cancellation cases): twice the largest ratio measured on MI355X, see the
# tables in tests/test_gpu_fused_blocks.py
M_BOUND = {'res_small': (2 * 3.160, 2 * 2.286),
           'res_img32': (2 * 2.999, 2 * 1.206),
           'res_img16': (2 * 2.751, 2 * 1.322),
           'attn_small': (2 * 0.970, 2 * 1.475),
           'attn16': (2 * 0.844, 2 * 0.860)}


# ---------------------------------------------------------------------------------------------------------------- references
def _group_stats(x, groups):
    B, C = x.shape[:2]
    xg = x.reshape(B, groups, -1)
    mean = xg.mean(-1)
    var = ((xg - mean[..., None]) ** 2).mean(-1)
    rep = C // groups
    shape = (B, C) + (1,) * (x.dim() - 2)
    return mean.repeat_interleave(rep, 1).reshape(shape), (1.0 / torch.sqrt(var + 1e-5)).repeat_interleave(rep, 1).reshape(shape)


def _chan(v, x):
    return v.double().reshape((1, -1) + (1,) * (x.dim() - 2))


def gn_exact(x, w, b, scale=None, shift=None):
    """GroupNorm(min(32, C) groups, eps 1e-5) in the dtype of x, then optionally * (1 + scale) + shift (scale, shift: [B, C, 1, 1])."""
    mean, rstd = _group_stats(x, min(32, x.shape[1]))
    y = (x - mean) * rstd * _chan(w, x) + _chan(b, x)
    return y if scale is None else y * (1 + scale) + shift


def gn_affine32(x, w, b, scale=None, shift=None):
    """The same as x * A + B with the exact float64 coefficients stored in fp32 (the kernels' form)."""
    mean, rstd = _group_stats(x, min(32, x.shape[1]))
    A = rstd * _chan(w, x)
    Bc = _chan(b, x) - mean * A
    if scale is not None:
        A, Bc = A * (1 + scale), Bc * (1 + scale) + shift
    return x * A.float().double() + Bc.float().double()


def _d(sd):
    return {k: v.double() for k, v in sd.items()}


def _res(sd, x, ss, gn, want_h=False):
    w = _d(sd)
    x, ss = x.double(), ss.double()
    co = w['in_layers.2.weight'].shape[0]
    h = F.conv2d(nets.silu(gn(x, w['in_layers.0.weight'], w['in_layers.0.bias'])), w['in_layers.2.weight'], w['in_layers.2.bias'], padding=1)
    scale, shift = ss[:, :co, None, None], ss[:, co:2 * co, None, None]
    a = nets.silu(gn(h, w['out_layers.0.weight'], w['out_layers.0.bias'], scale, shift))
    y = F.conv2d(a, w['out_layers.3.weight'], w['out_layers.3.bias'], padding=1)
    skip = F.conv2d(x, w['skip_connection.weight'], w['skip_connection.bias']) if 'skip_connection.weight' in w else x
    return (skip + y, h) if want_h else skip + y


def res_block64(sd, x, ss, want_h=False):
    """The ResBlock (use_scale_shift_norm) in float64.  sd: the block's own keys (in_layers.0.weight, ...); x: [B, Cin, H, W];
    ss: [B, 2 Cout], the scale | shift row as the kernels receive it.  want_h: also the first convolution's output."""
    return _res(sd, x, ss, gn_exact, want_h)


def _attn(sd, x, heads, gn):
    w = _d(sd)
    x = x.double()
    B, C = x.shape[:2]
    flat = x.reshape(B, C, -1)
    T = flat.shape[2]
    qkv = F.conv1d(gn(flat, w['norm.weight'], w['norm.bias']), w['qkv.weight'], w['qkv.bias']).reshape(B * heads, -1, T)
    ch = qkv.shape[1] // 3
    q, k, v = qkv[:, :ch], qkv[:, ch:2 * ch], qkv[:, 2 * ch:]
    sc = 1 / math.sqrt(math.sqrt(ch))
    logits = torch.einsum('bct,bcs->bts', q * sc, k * sc)
    e = torch.exp(logits - logits.max(-1, keepdim=True).values)
    probs = e / e.sum(-1, keepdim=True)
    a = torch.einsum('bts,bcs->bct', probs, v).reshape(B, -1, T)
    out = flat + F.conv1d(a, w['proj_out.weight'], w['proj_out.bias'])
    return out.reshape(x.shape), logits, probs


def attn_block64(sd, x, heads):
    """The AttentionBlock in float64: (out, logits [B heads, T queries, T keys], softmax rows).  qkv channel order: [head][q | k | v][ch]."""
    return _attn(sd, x, heads, gn_exact)


def affine_floor64(sd, x, ss=None, heads=None):
    """The block in float64 with every GroupNorm as x * A + B, A and B exact but stored in fp32: a ResBlock when ss is given, an
    AttentionBlock when heads is."""
    if ss is not None:
        return _res(sd, x, ss, gn_affine32)
    return _attn(sd, x, heads, gn_affine32)[0]


def judge(got, want64, ref32, floor64=None):
    got, want64 = got.double(), want64.double()
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    err = (got - want64).abs().max().item()
    e32 = (ref32.double() - want64).abs().max().item()
    e_floor = (floor64.double() - want64).abs().max().item() if floor64 is not None else 0.0
    return err / max(e32, e_floor)


def softmax_no_max_fp32(sd, x, heads):
    """What a kernel without max subtraction would compute: the fp32 oracle's AttentionBlock with softmax as exp(w) / sum exp(w)."""
    B, C = x.shape[:2]
    flat = x.reshape(B, C, -1)
    qkv = F.conv1d(nets.group_norm(flat, sd['norm.weight'], sd['norm.bias']), sd['qkv.weight'], sd['qkv.bias'])
    qkv = qkv.reshape(B * heads, -1, qkv.shape[2])
    ch = qkv.shape[1] // 3
    sc = 1 / math.sqrt(math.sqrt(ch))
    e = torch.exp(torch.einsum('bct,bcs->bts', qkv[:, :ch] * sc, qkv[:, ch:2 * ch] * sc))
    a = torch.einsum('bts,bcs->bct', e / e.sum(-1, keepdim=True), qkv[:, 2 * ch:]).reshape(B, -1, flat.shape[2])
    return (flat + F.conv1d(a, sd['proj_out.weight'], sd['proj_out.bias'])).reshape(x.shape)


# ---------------------------------------------------------------------------------------------------------------- the shapes
# Every (C0 | C1) the host checks of the three C entry points accept (read from res_small_ok, res_img_ok, res_img_residual_ok,
# igemm_supported and dlpm_res*block*_f32 / dlpm_attnblock_small_f32 in unet.hip):
#   dlpm_resblock_small_f32 (k_resblock_small<8 | 4>, 64 output channels): C0 + C1 = 64 without skip weights or = 128 with them, each
#     source a multiple of 4.  The multiples of 4 are 16 + 32 splits per size; the kernel treats them alike (a float4 quad of the
#     staging loop lies in one source), so the list has the ends and the middle: 4 | 60 and 124 | 4 are the extreme pitches.
#   dlpm_resblock_img_f32 at 32x32 (k_resblock_wino4_img, 32 output channels): 32 | 0 without skip weights; with them every
#     C0 + C1 <= 128 in multiples of 32 per source (the skip convolution is an implicit GEMM of 32-channel chunks).
#   dlpm_resblock_img_f32 at 16x16 (k_resblock_wino4_img16, 64 output channels): 64 | 0 without skip weights; with them the same
#     multiples of 32 with C0 + C1 != 64.  (32 | 32 is refused either way: without skip weights by res_img_residual_ok, with them
#     because C0 + C1 = the output channels.)
#   dlpm_attnblock_small_f32: 64 channels, 4 heads, 4x4 / 8x8 (k_attnblock_small<4 | 8>) and 16x16 (k_attnblock16).  Nothing to sweep.
RES_SMALL_SPLITS = [(64, 0), (32, 32), (4, 60), (64, 64), (128, 0), (96, 32), (32, 96), (124, 4)]
RES_IMG32_SPLITS = [(32, 0), (64, 0), (32, 32), (96, 0), (64, 32), (32, 64), (128, 0), (64, 64), (96, 32), (32, 96)]
RES_IMG16_SPLITS = [(64, 0), (32, 0), (96, 0), (128, 0), (64, 32), (32, 64), (64, 64), (96, 32), (32, 96)]
# cancellation kinds: the shapes tests/test_gpu_kernels.py runs, plus one new split per kernel (the last of each list)
RES_SMALL_CANCEL = [(64, 0, 8), (64, 0, 4), (64, 64, 8), (64, 64, 4), (96, 32, 4)]
RES_IMG32_CANCEL = [(32, 0), (32, 32), (64, 32), (32, 96)]
RES_IMG16_CANCEL = [(64, 0), (64, 64), (64, 32), (32, 64)]
RES_KINDS = ('cancel_gn1', 'cancel_gn2', 'cancel_out')
ATTN_KINDS = ('cancel_gn1', 'cancel_out')

KERNELS = ('res_small', 'res_img32', 'res_img16', 'attn_small', 'attn16')


def _name(kernel, c0, c1, hs, kind):
    return '%s_%d_%d_h%d_%s' % (kernel, c0, c1, hs, kind)


def _cases():
    out = []
    for hs in (8, 4):
        out += [('res_small', c0, c1, hs, 'benign') for c0, c1 in RES_SMALL_SPLITS]
    out += [('res_img32', c0, c1, 32, 'benign') for c0, c1 in RES_IMG32_SPLITS]
    out += [('res_img16', c0, c1, 16, 'benign') for c0, c1 in RES_IMG16_SPLITS]
    for hs in (4, 8, 16):
        k = 'attn16' if hs == 16 else 'attn_small'
        out += [(k, 64, 0, hs, 'benign'), (k, 64, 0, hs, 'sharp')]
    for kind in RES_KINDS:
        out += [('res_small', c0, c1, hs, kind) for c0, c1, hs in RES_SMALL_CANCEL]
        out += [('res_img32', c0, c1, 32, kind) for c0, c1 in RES_IMG32_CANCEL]
        out += [('res_img16', c0, c1, 16, kind) for c0, c1 in RES_IMG16_CANCEL]
    for kind in ATTN_KINDS:
        for hs in (4, 8, 16):
            out.append(('attn16' if hs == 16 else 'attn_small', 64, 0, hs, kind))
    return {_name(*c): c for c in out}


CASES = _cases()
BENIGN = [n for n, c in CASES.items() if c[4] in ('benign', 'sharp')]
CANCEL = [n for n, c in CASES.items() if c[4].startswith('cancel_')]
BATCH = 3
HEADS = 4
SHARP_KBIAS = 30.0


def cout_of(kernel):
    return 32 if kernel == 'res_img32' else 64


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:3], 'big')


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


class Case:
    """Inputs of one launch.  ResBlocks: x [B, C0 + C1, H, H], emb [B, 128], ss = the block's emb_layers of it (fp32, as the host
    computes it), sd.  AttentionBlocks: x, sd."""

    def __init__(self, name):
        self.name = name
        self.kernel, self.c0, self.c1, self.hs, self.kind = CASES[name]
        self.is_res = self.kernel.startswith('res')
        self.cin, self.cout = self.c0 + self.c1, cout_of(self.kernel)
        s = _seed(name)
        kind, B, hs = self.kind, BATCH, self.hs
        if self.is_res:
            sd = sbw._draw(sbw._shapes_res(self.cin, 128, self.cout), sbw.RES_KEYS, s)
        else:
            sd = sbw._draw(sbw._shapes_attn(), sbw.ATTN_KEYS, s)
        x = sbw.seeded_input((B, self.cin, hs, hs), s + 1)
        if kind == 'cancel_gn1':
            x = 100.0 + 0.05 * _randn((B, self.cin, hs, hs), s + 1) + 0.3 * _randn((B, self.cin, 1, 1), s + 3)
        elif kind == 'cancel_gn2':
            sd['in_layers.2.weight'] = 0.05 * sd['in_layers.2.weight']
            sd['in_layers.2.bias'] = 100.0 + 0.3 * _randn((self.cout,), s + 3)
        elif kind == 'cancel_out':
            last = 'out_layers.3' if self.is_res else 'proj_out'
            sd[last + '.weight'] = 0.05 * sd[last + '.weight']
            sd[last + '.bias'] = 100.0 + 0.3 * _randn((self.cout,), s + 3)
            if 'skip_connection.weight' in sd:
                sd['skip_connection.weight'] = 0.05 * sd['skip_connection.weight']
            else:
                x = 0.05 * _randn((B, self.cin, hs, hs), s + 1)
        elif kind == 'sharp':
            rows = (torch.arange(3 * 64) % 48) < 32       # the q and k rows of every head
            sd['qkv.weight'] = torch.where(rows[:, None, None], 6.0 * sd['qkv.weight'], sd['qkv.weight'])
            bias = torch.where(rows, 6.0 * sd['qkv.bias'], sd['qkv.bias']).reshape(HEADS, 3, 16).clone()
            # The x 6 recipe alone leaves every row maximum positive (+17 .. +40 over the seeds tried, and on the recorded F13 / F14
            # inputs): a query's own neighbourhood always has an aligned key.  A common offset SHARP_KBIAS u (|u| = 1) on a head's k
            # bias adds the row constant q_i . u SHARP_KBIAS / 4 to the logits of query i -- the softmax is unchanged, the kernel sees
            # rows that lie wholly far below zero (and others far above): the third condition of `conditions`.
            u = _randn((HEADS, 16), s + 3)
            bias[:, 1] += SHARP_KBIAS * u / u.norm(dim=1, keepdim=True)
            sd['qkv.bias'] = bias.reshape(-1)
        self.sd, self.x = sd, x.contiguous()
        if self.is_res:
            self.emb = _randn((B, 128), s + 2)
            self.ss = F.linear(nets.silu(self.emb), sd['emb_layers.1.weight'], sd['emb_layers.1.bias'])

    def with_sd(self, repl):
        """A copy of the state dict with the tensors of `repl` replaced."""
        sd = dict(self.sd)
        sd.update(repl)
        return sd

    # -- the three evaluations the judge needs (of any state dict with this case's inputs)
    def want64(self, sd=None):
        sd = sd or self.sd
        return res_block64(sd, self.x, self.ss) if self.is_res else attn_block64(sd, self.x, HEADS)[0]

    def ref32(self, sd=None):
        sd = sd or self.sd
        with torch.no_grad():
            return nets.res_block(sd, '', self.x, self.emb) if self.is_res else nets.attention_block(sd, '', self.x, HEADS)

    def floor64(self, sd=None):
        sd = sd or self.sd
        return affine_floor64(sd, self.x, ss=self.ss) if self.is_res else affine_floor64(sd, self.x, heads=HEADS)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def refs(name):
    """(want64, ref32, floor64 or None) of a case, computed once and never modified.  Cancellation kinds carry the floor."""
    c = case(name)
    return c.want64(), c.ref32(), (c.floor64() if c.kind.startswith('cancel_') else None)


def ratio(name, got):
    return judge(got, *refs(name))


# ---------------------------------------------------------------------------------------------------------------- conditions
def group_mean_over_std(x):
    """min over (image, group) of |mean| / std, GroupNorm's groups."""
    g = min(32, x.shape[1])
    xg = x.double().reshape(x.shape[0], g, -1)
    return (xg.mean(-1).abs() / xg.std(-1, unbiased=False)).min().item()


def conditions(name):
    """What makes a sharp / cancel case what it claims to be, as numbers (asserted in test_block_refs_cpu.py)."""
    c = case(name)
    if c.kind == 'sharp':
        _, logits, probs = attn_block64(c.sd, c.x, HEADS)
        rowmax = logits.max(-1).values
        return {'over89': (rowmax > 89).double().mean().item(), 'soft': (probs.max(-1).values < 0.99).double().mean().item(),
                'min_rowmax': rowmax.min().item()}
    if c.kind == 'cancel_gn1':
        return {'mean_over_std': group_mean_over_std(c.x)}
    if c.kind == 'cancel_gn2':
        return {'mean_over_std': group_mean_over_std(res_block64(c.sd, c.x, c.ss, want_h=True)[1])}
    if c.kind == 'cancel_out':
        y = refs(name)[0].reshape(BATCH, c.cout, -1)
        return {'mean_abs_min': y.mean(-1).abs().min().item(), 'mean_abs_max': y.mean(-1).abs().max().item(), 'std_max': y.std(-1).max().item()}
    return {}


# ---------------------------------------------------------------------------------------------------------------- the net
def net_case(B=2):
    """The `mnist` net of test_host_mirror.UNETS with seeded x, t: (net, state dict, x, t)."""
    from test_host_mirror import UNETS, build_unet
    net, _ = build_unet('mnist')
    g = torch.Generator().manual_seed(20260)
    x, t = torch.randn(B, UNETS['mnist']['in_ch'], 32, 32, generator=g), torch.rand(B, generator=g)
    return net, {k: v.detach() for k, v in net.state_dict().items()}, x, t


def flat_feats(y, feats):
    """[(name, tensor)] in forward order: down 0.., middle, up 0.., out."""
    return ([('down %d' % i, f) for i, f in enumerate(feats['down'])] + [('middle', feats['middle'])] +
            [('up %d' % i, f) for i, f in enumerate(feats['up'])] + [('out', y)])


def net_forwards(sd, x, t):
    """The oracle's forward in fp32 and in float64: two lists of (name, tensor)."""
    with torch.no_grad():
        f32 = flat_feats(*nets.unet_forward(sd, x, t, HEADS, return_feats=True))
        sd64 = {k: v.double() for k, v in sd.items()}
        f64 = flat_feats(*nets.unet_forward(sd64, x.double(), t.double(), HEADS, return_feats=True))
    return f32, f64
