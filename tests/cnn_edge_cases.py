"""The cases of tests/test_cnn_edge_ref.py (CPU) and tests/test_gpu_cnn_edges.py (GPU): the
smallest shapes at which the stem, front, 1x1-head and fused-tail kernels of
csrc/fvp_conv.hip can go wrong, their seeded inputs, and the production packers' output for
them (fvp.backbone.FvpPoseResNet, fvp.cnn.FvpCNN._compile_front7 / _compile_tail,
fvp.cnn.ConvLayer), packed on the CPU so that both tests see the same bits.

Stems (8 x 32 output tiles, stride 2): images smaller than the filter, H in {15, 16, 17} x W
in {63, 64, 65} (exact tiles, one row / column past them, both parities: 2 or 3 rows of
bottom / right padding), a 2 x 3 tile grid over 3 images; C = 1 .. 3 (fp32), 1 .. 4 (bf16).
Front layers (tiles 8 x 16 fp32, 8 x 32 bf16, stride 1): H in {8, 9} x W in {16, 17, 32, 33},
tiny maps, a non-square grid over 3 images; C at the channel-quad edges of the fp32 loader
and the 8-channel halves of the bf16 loader.
1x1 head: every instantiation (Cin -> t4 = 4, 8, 16), pixel counts around one block of 256
and blocks that straddle images, pitches at and above 4 t4, channel offsets.
Fused tail: every (Cpi, Cs) pair of Cpi in {16, 48, 64, 80, 128} (1, 3, 4, 5, 8 K steps; 5 is
the first with weights loaded per item) x Cs in {1, 20, 29, 32}, the other values cycled so
that every Cps rule, J, W and H appears.

Draws (chosen before any kernel ran; the bf16 cap of cnn_edge_ref may move a seed on, from
pre and tol alone): stem images uniform in (0, 1), front maps max(N(0, 1), 0), 7x7 weights
(N(0, 1) + 0.5) / sqrt(49 C) with every other output channel negated, scale in [0.5, 1.5),
shift N(0, 0.5); the BatchNorm layers get running statistics that fold to those.
"""
import collections
import functools
import itertools
import types

import numpy as np

import cnn_edge_ref as E

Case7 = collections.namedtuple("Case7", "kernel N C H W")
Case1 = collections.namedtuple("Case1", "Cin Cout relu N H W pitch")
CaseOff = collections.namedtuple("CaseOff", "Cin Cout c0 C Cp N H W")
CaseTail = collections.namedtuple("CaseTail", "Cpi Cs Cps J N H W")


# ---- the 7x7 kernels ---------------------------------------------------------------------
def cases7(name):
    k = E.KERNELS[name]
    if k.stride == 2:
        chans = (1, 2, 3, 4) if k.bf16 else (1, 2, 3)
        out = [Case7(name, 1, 3, 1, 1), Case7(name, 2, 1, 2, 3)]
        out += [Case7(name, 2, c, h, w) for h in (15, 16, 17) for w in (63, 64, 65) for c in chans]
        out += [Case7(name, 3, c, 17, 131) for c in sorted({3, chans[-1]})]
        return tuple(out)
    chans = (1, 3, 4, 5, 8, 9, 15, 16)
    out = [Case7(name, 1, 1, 1, 1), Case7(name, 3, 5, 5, 3)]
    # every C on the ragged 9 x 17 / 9 x 33 maps, and cycled over the other shapes
    shapes = [(h, w) for h in (8, 9) for w in (16, 17, 32, 33)]
    out += [Case7(name, 2, c, h, w) for (h, w), c in zip(shapes, itertools.cycle(chans))]
    out += [Case7(name, 2, c, 9, 17 if k.tw == 16 else 33) for c in chans]
    out.append(Case7(name, 3, 15, 9, 49))  # 2 x 4 tiles of 8 x 16
    if k.tw == 32:
        out.append(Case7(name, 3, 15, 9, 65))  # (2 x 2 tiles of 8 x 32 above:) 2 x 3
    return tuple(dict.fromkeys(out))


def id7(c):
    return f"{c.kernel}-N{c.N}-C{c.C}-{c.H}x{c.W}"


def walk_base7(name):
    """The ragged case the persistent walk repeats along N (conv_front7_bf16 has no walk: one
    tile per block)."""
    k = E.KERNELS[name]
    assert name != "front7_bf16"
    return Case7(name, 2, 3, 17, 65) if k.stride == 2 else Case7(name, 2, 15, 9, 17)


def _seed7(c):
    return ((sorted(E.KERNELS).index(c.kernel) * 8 + c.N) * 32 + c.C) * 100003 + c.H * 257 + c.W


def _draw7(c, seed):
    k = E.KERNELS[c.kernel]
    rng = np.random.default_rng(seed)
    if k.stride == 2:
        x = (1.0 - rng.random((c.N, c.C, c.H, c.W))).astype(np.float32)  # (0, 1]: no zero on a border
    else:
        x = np.maximum(rng.standard_normal((c.N, c.C, c.H, c.W)), 0).astype(np.float32)
    w = ((rng.standard_normal((k.cout, c.C, 7, 7)) + 0.5) / np.sqrt(49 * c.C)).astype(np.float32)
    w[1::2] *= -1
    scale = rng.uniform(0.5, 1.5, k.cout)
    shift = rng.standard_normal(k.cout) * 0.5
    return x, w, scale, shift, rng


def _bn(cout, scale, shift, rng, bias=None):
    """An eval BatchNorm2d with non-trivial running statistics that folds (after a conv with
    `bias`) to scale and shift: s = gamma / sqrt(var + eps), shift = (bias - mean) s + beta."""
    import torch
    import torch.nn as nn

    bn = nn.BatchNorm2d(cout).eval()
    mean, var = rng.uniform(-0.2, 0.2, cout), rng.uniform(0.5, 1.5, cout)
    b = np.zeros(cout) if bias is None else np.asarray(bias, np.float64)
    with torch.no_grad():
        bn.running_mean.copy_(torch.from_numpy(mean))
        bn.running_var.copy_(torch.from_numpy(var))
        bn.weight.copy_(torch.from_numpy(scale * np.sqrt(var + bn.eps)))
        bn.bias.copy_(torch.from_numpy(shift - (b - mean) * scale))
    return bn


def _pack7(c, w, scale, shift, rng):
    """The production packer's (wpack, scale, shift) CPU tensors for one 7x7 layer."""
    import torch
    import torch.nn as nn

    import cnn_arch
    from fvp import cnn
    from fvp.backbone import FvpPoseResNet

    k = E.KERNELS[c.kernel]
    dtype = torch.bfloat16 if k.bf16 else torch.float32
    if k.stride == 2:  # a PoseResNet of nothing but its stem
        m = nn.Module()
        m.conv1 = nn.Conv2d(c.C, 64, 7, 2, 3, bias=False)
        m.bn1 = _bn(64, scale, shift, rng)
        m.maxpool = nn.MaxPool2d(3, 2, 1)
        for name in ("layer1", "layer2", "layer3", "layer4", "deconv_layers"):
            setattr(m, name, nn.Sequential())
        m.final_layer = nn.Conv2d(64, 1, 1)
        with torch.no_grad():
            m.conv1.weight.copy_(torch.from_numpy(w))
        bb = FvpPoseResNet(m.eval(), dtype)
        wp = bb.stem7 if k.bf16 else bb.stem7_f32
        assert wp is not None and (bb.stem7_f32 is None) == k.bf16
        return wp, bb.stem.scale, bb.stem.shift
    blk = cnn_arch.Basic2DBlock(c.C, 16, 7).eval()
    bias = rng.standard_normal(16) * 0.05
    with torch.no_grad():
        blk.block[0].weight.copy_(torch.from_numpy(w))
        blk.block[0].bias.copy_(torch.from_numpy(bias))
    blk.block[1] = _bn(16, scale, shift, rng, bias)
    seq = nn.Sequential(blk)
    f = cnn.FvpCNN.__new__(cnn.FvpCNN)
    f.module, f.front, f.front7 = types.SimpleNamespace(front_layers=seq), cnn._Plan(seq, dtype), None
    f._compile_front7(dtype)
    assert f.front7 is not None and f.front7[0] == k.fn
    return f.front7[1], f.front7[2].scale, f.front7[2].shift


@functools.lru_cache(maxsize=None)
def data7(c, tries=64):
    """dict(x, w, scale, shift: numpy fp32, the folded values the packed layer holds; wpack,
    scale_t, shift_t: the packer's CPU tensors; ref, tol, pre: float64; share, seed).  bf16
    kernels: the first draw from the case's seed on whose cap holds (ref and tol decide)."""
    k = E.KERNELS[c.kernel]
    for seed in range(_seed7(c), _seed7(c) + tries):
        x, w, scale, shift, rng = _draw7(c, seed)
        wp, sc, sh = _pack7(c, w, scale, shift, rng)
        scale, shift = sc[:k.cout].numpy().copy(), sh[:k.cout].numpy().copy()
        ref, tol, pre = E.ref7(k, x, w, scale, shift)
        share = E.wide_share(pre, tol) if k.bf16 else 0.0
        if share <= E.CAP:
            return dict(x=x, w=w, scale=scale, shift=shift, wpack=wp, scale_t=sc, shift_t=sh, ref=ref, tol=tol, pre=pre,
                        share=share, seed=seed)
    raise AssertionError(f"no draw of {id7(c)} within the cap")


# ---- the 1x1 head ------------------------------------------------------------------------
CIN1, COUT1 = (1, 15, 16, 17, 32, 33, 50, 64), (1, 15, 33, 64)
PIXELS1 = ((1, 1, 1), (1, 1, 255), (1, 1, 256), (1, 1, 257), (3, 7, 13))  # (N, H, W); 3 x 91: blocks straddle images


def cases1(cin):
    out = []
    for i, (cout, relu, (n, h, w)) in enumerate(itertools.product(COUT1, (0, 1), PIXELS1)):
        out.append(Case1(cin, cout, relu, n, h, w, 4 * E.t4_of(cin) + (0, 4, 16)[(i + cin) % 3]))
    return tuple(out)


def cases_off():
    """The channel-offset call FvpCNN._conv1x1_nchw(y, c0, o): o reads channels c0 .. c0 + Cin - 1
    of an Act of C channels at pitch Cp (CenterNet's merged heads: Cin = 32 at c0 = 32 of 64)."""
    return (CaseOff(15, 15, 16, 31, 32, 3, 7, 13), CaseOff(32, 2, 36, 68, 68, 3, 7, 13),
            CaseOff(20, 33, 16, 40, 48, 1, 1, 257), CaseOff(50, 64, 36, 90, 100, 2, 5, 9),
            CaseOff(16, 1, 36, 52, 52, 3, 7, 13), CaseOff(32, 15, 16, 64, 64, 1, 1, 255))


def layer1(cin, cout, seed):
    """(conv, bn) of a 1x1 layer on the CPU: weights N(0, 1) / sqrt(Cin), folded scale in
    +-[0.5, 1.5), shift N(0, 0.5)."""
    import torch
    import torch.nn as nn

    rng = np.random.default_rng(seed)
    conv = nn.Conv2d(cin, cout, 1).eval()
    bias = rng.standard_normal(cout) * 0.05
    scale = rng.uniform(0.5, 1.5, cout) * np.where(np.arange(cout) % 3 == 2, -1.0, 1.0)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(rng.standard_normal((cout, cin, 1, 1)) / np.sqrt(cin)))
        conv.bias.copy_(torch.from_numpy(bias))
    return conv, _bn(cout, scale, rng.standard_normal(cout) * 0.5, rng, bias)


@functools.lru_cache(maxsize=None)
def packed1(cin, cout):
    """The ConvLayer (CPU) of a head: its wpack holds 4 t4 rows (cpi), zero past Cin."""
    from fvp import cnn

    conv, bn = layer1(cin, cout, 7000 + 97 * cin + cout)
    layer = cnn.ConvLayer(conv, bn, cpi=max(-(-cin // 16) * 16, 4 * E.t4_of(cin)))
    assert layer.wpack.shape[1] >= 4 * E.t4_of(cin)
    return conv, layer


def rows1(seed, n, h, w, cp):
    """NHWC rows [N, H, W, Cp]: finite random values in every channel, the padding included."""
    return np.random.default_rng(seed).standard_normal((n, h, w, cp)).astype(np.float32)


def nchw(rows, c0, cin):
    return np.ascontiguousarray(rows[..., c0:c0 + cin].transpose(0, 3, 1, 2))


# ---- the fused tail ----------------------------------------------------------------------
def cases_tail():
    out = []
    cs_all, j_all, hw_all = (1, 20, 29, 32), (1, 15, 16), ((1, 32), (3, 32), (1, 96), (3, 96))
    for i, (cpi, cs) in enumerate(itertools.product((16, 48, 64, 80, 128), cs_all)):
        tight = -(-cs // 4) * 4
        h, w = hw_all[(i + i // 4) % 4]
        out.append(CaseTail(cpi, cs, tight if (i + i // 4) % 2 == 0 else 32, j_all[(i + i // 4) % 3], 2, h, w))
    return tuple(out)


def id_tail(c):
    return f"{c.Cpi}-{c.Cs}({c.Cps})-{c.J}-N{c.N}-{c.H}x{c.W}"


def walk_bases_tail():
    """A one-K-step case and the first with weights loaded per item, cheap to repeat along N."""
    return CaseTail(16, 1, 4, 15, 2, 1, 32), CaseTail(80, 20, 20, 1, 2, 3, 96)


def modules_tail(c):
    """(up, head, head_bn) on the CPU: Upsample2DBlock(Cpi, Cs, 2, 2), Conv2d(Cs, J, 1) and a
    BatchNorm after it, so that the head's scale is not 1."""
    import torch
    import torch.nn as nn

    import cnn_arch

    rng = np.random.default_rng(9000 + (c.Cpi * 37 + c.Cs) * 17 + c.J)
    up = cnn_arch.Upsample2DBlock(c.Cpi, c.Cs, 2, 2).eval()
    bias = rng.standard_normal(c.Cs) * 0.05
    with torch.no_grad():
        up.block[0].weight.copy_(torch.from_numpy(rng.standard_normal((c.Cpi, c.Cs, 2, 2)) / np.sqrt(c.Cpi)))
        up.block[0].bias.copy_(torch.from_numpy(bias))
    up.block[1] = _bn(c.Cs, rng.uniform(0.5, 1.5, c.Cs), rng.standard_normal(c.Cs) * 0.5, rng, bias)
    head, hbn = layer1(c.Cs, c.J, 9500 + c.Cs * 17 + c.J)
    return up, head, hbn


def compile_tail(up, head, hbn):
    """FvpCNN._compile_tail on these modules (on whatever device they are): the FvpCNN stand-in
    with .tail, .out and .encdec, as tests/test_cnn.py builds it."""
    from fvp import cnn

    f = cnn.FvpCNN.__new__(cnn.FvpCNN)
    f.module = types.SimpleNamespace(encoder_decoder=types.SimpleNamespace(decoder_upsample1=up), output_layer=head)
    f.encdec = types.SimpleNamespace(parts={"decoder_upsample1": cnn._Plan(up)})
    f.out = cnn.ConvLayer(head, hbn)
    f.tail = f._compile_tail()
    assert f.tail is not None
    return f


@functools.lru_cache(maxsize=None)
def data_tail(c):
    """dict(x [N, Cpi, H, W], skip [N, Cs, 2H, 2W], skip_rows [N, 2H, 2W, Cps] (finite random
    values in the padding channels), w, scale, shift, wh, hscale, hshift: numpy; f: the packed
    stand-in (CPU); ref, tol: float64)."""
    up, head, hbn = modules_tail(c)
    f = compile_tail(up, head, hbn)
    rng = np.random.default_rng(9900 + (c.Cpi * 37 + c.Cs) * 17 + c.J)
    x = rng.standard_normal((c.N, c.Cpi, c.H, c.W)).astype(np.float32)
    skip_rows = rng.standard_normal((c.N, 2 * c.H, 2 * c.W, c.Cps)).astype(np.float32)
    skip = np.ascontiguousarray(skip_rows[..., :c.Cs].transpose(0, 3, 1, 2))
    layer = f.tail[1]
    d = dict(x=x, skip=skip, skip_rows=skip_rows, w=up.block[0].weight.detach().numpy(),
             scale=layer.scale[:c.Cs].numpy().copy(), shift=layer.shift[:c.Cs].numpy().copy(),
             wh=head.weight.detach().numpy()[:, :, 0, 0], hscale=f.out.scale[:c.J].numpy().copy(),
             hshift=f.out.shift[:c.J].numpy().copy(), f=f)
    d["ref"], d["tol"] = E.ref_tail(*tail_args(d))
    return d


def tail_args(d):
    return tuple(d[k] for k in ("x", "w", "scale", "shift", "skip", "wh", "hscale", "hshift"))
