"""Cases, float64 references and geometric masks for the convolution family's treatment of
non-finite activations (faster-voxelpose_amd/csrc/fvp_conv.hip, fvp_wino.hip, fvp_c2c.hip).
Not a conftest: the CPU tests (test_cnn_nonfinite_model.py) and the GPU tests
(test_gpu_cnn_nonfinite.py) import it.  Plain torch / numpy, no GPU.

Every case runs N images (or columns) and poisons ONE input element of image 1 with NaN or
+Inf.  The reference is always a deep copy of the seeded module in float64 on the CPU (never
torch's GPU convolution: MIOpen spreads an Inf beyond the windows that hold it,
tests/test_backbone.py::test_stem7_f32_vs_torch).  For single layers the set of outputs that
may change is known from the geometry alone (``window_mask``); Winograd kernels transform whole
input patches, so they may widen it to the tiles whose patch holds the element
(``wino_tile_mask`` / ``wino_deconv_tile_mask``), and no further.

References are cached and shared: callers must not write into what they get.
"""
from __future__ import annotations

import copy
import functools
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn

REL_F32, REL_BF16 = 2e-5, 2e-2  # tests/test_cnn.py: REL, and the bf16-operand bar
VALUES = {"nan": float("nan"), "inf": float("inf")}
POISONED = 1  # the image (column) that holds the poisoned element


def poison(x: torch.Tensor, where, value: float) -> torch.Tensor:
    """A copy of x with x[where] = value."""
    y = x.clone()
    y[tuple(where)] = value
    return y


def reference(module: nn.Module, *inputs: torch.Tensor):
    """module's forward in float64 on the CPU (a deep copy: the caller's module is untouched)."""
    m = copy.deepcopy(module).cpu().double().eval()
    with torch.no_grad():
        return m(*(t.detach().cpu().double() for t in inputs))


def classes(t: torch.Tensor):
    """(isnan, == +inf, == -inf)"""
    return torch.isnan(t), t == float("inf"), t == float("-inf")


# ------------------------------------------------------------------------------------ geometry
def window_mask(in_hw, pix, k: int, stride: int, pad: int, transposed: bool = False) -> np.ndarray:
    """bool [Ho][Wo]: the outputs of a k x k convolution (stride, zero padding; transposed: a
    ConvTranspose2d) whose window holds input pixel pix."""
    def axis(n, p):
        if transposed:  # output o = i * stride - pad + tap
            no = (n - 1) * stride - 2 * pad + k
            o = np.arange(no)
            t = o + pad - p * stride
        else:           # input i = o * stride - pad + tap
            no = (n + 2 * pad - k) // stride + 1
            o = np.arange(no)
            t = p - (o * stride - pad)
        return (t >= 0) & (t < k)

    return np.outer(axis(in_hw[0], pix[0]), axis(in_hw[1], pix[1]))


def wino_tile_mask(hw, pix) -> np.ndarray:
    """F(2x2, 3x3) (conv_wino_kernel): tile (ty, tx) writes outputs (2ty .. 2ty+1, 2tx .. 2tx+1)
    from the 4 x 4 input patch (2ty-1 .. 2ty+2, 2tx-1 .. 2tx+2); every output of every tile whose
    patch holds pix."""
    def axis(n, p):
        o = np.arange(n)
        t = o // 2
        return (2 * t - 1 <= p) & (p <= 2 * t + 2)

    return np.outer(axis(hw[0], pix[0]), axis(hw[1], pix[1]))


def wino_deconv_tile_mask(in_hw, pix) -> np.ndarray:
    """ConvTranspose2d(4, 2, 1) by F(2x2, 2x2) per output parity (deconv_wino_kernel): for
    parity r, class-space tile T writes outputs 2 (2T + d) + r, d in {0, 1}, from input rows
    2T - 1 + r .. 2T + 1 + r; every output of every (class, tile) whose patch holds pix."""
    def axis(n, p):
        o = np.arange(2 * n)
        r, t = o & 1, (o >> 1) // 2
        lo = 2 * t - 1 + r
        return (lo <= p) & (p <= lo + 2)

    return np.outer(axis(in_hw[0], pix[0]), axis(in_hw[1], pix[1]))


# -------------------------------------------------------------------------------- single layers
@dataclass(frozen=True)
class Layer:
    """conv (+ BN) (+ residual) (+ ReLU) on n x cin x hw; the poisoned channel is cin // 2."""
    cin: int
    cout: int
    k: int
    hw: tuple
    seam: tuple              # the interior poisoned position
    seam2: tuple | None = None  # a second one (the other column parity of a stride-2 kernel)
    stride: int = 1
    pad: int | None = None   # default (k - 1) // 2
    transposed: bool = False
    res: str | None = None   # "pre": relu(y + r), "post": relu(y) + r
    bias: bool = True
    bn: bool = True
    relu: bool = True
    bf16: bool = False       # the input is rounded to bf16; REL_BF16
    seed: int = 0
    n: int = 2
    source: str | None = None  # "stem7" / "front7": the conv and BN of a seeded network

    @property
    def padding(self):
        return (self.k - 1) // 2 if self.pad is None else self.pad

    @property
    def out_hw(self):
        k, s, p = self.k, self.stride, self.padding
        if self.transposed:
            return tuple((n - 1) * s - 2 * p + k for n in self.hw)
        return tuple((n + 2 * p - k) // s + 1 for n in self.hw)

    @property
    def rel(self):
        return REL_BF16 if self.bf16 else REL_F32

    def positions(self) -> dict:
        """corner, last row and column, interior seam -- the last one moved onto the stride grid
        where a 1 x 1 strided kernel would otherwise never read it."""
        H, W = self.hw
        last = (H - 1, W - 1)
        if self.k == 1 and self.stride > 1:
            last = tuple(v - v % self.stride for v in last)
        pos = {"corner": (0, 0), "last": last, "seam": self.seam}
        if self.seam2 is not None:
            pos["seam2"] = self.seam2
        return pos

    def where(self, pos: str):
        return (POISONED, self.cin // 2) + tuple(self.positions()[pos])

    def window(self, pos: str) -> np.ndarray:
        return window_mask(self.hw, self.positions()[pos], self.k, self.stride, self.padding, self.transposed)


LAYERS = {
    # ConvLayer under the conv_kernel fixture: ragged tiles and the halo kernel's 16-wide seam
    "conv_k3": Layer(16, 32, 3, (9, 18), (4, 15), res="pre", seed=101),
    "conv_k7": Layer(15, 16, 7, (13, 10), (6, 8), seed=102),
    "conv_k1": Layer(32, 15, 1, (6, 7), (3, 4), seed=103),
    "conv_k5": Layer(40, 70, 5, (9, 11), (4, 8), res="pre", seed=104),
    "splitk": Layer(128, 128, 3, (16, 16), (7, 8), res="pre", seed=105),
    "deconv2": Layer(64, 32, 2, (5, 7), (2, 4), stride=2, pad=0, transposed=True, res="post", seed=106),
    "deconv4": Layer(48, 32, 4, (5, 7), (2, 3), stride=2, pad=1, transposed=True, bias=False, seed=107),
    "s2_k3": Layer(32, 64, 3, (11, 9), (5, 4), stride=2, pad=1, bias=False, seed=108),
    "s2_k1": Layer(64, 32, 1, (9, 7), (4, 4), stride=2, pad=0, bias=False, seed=109),
    "bf16_32": Layer(32, 32, 3, (9, 18), (4, 15), bf16=True, seed=110),
    "bf16_64": Layer(64, 64, 3, (9, 18), (4, 15), bias=False, bf16=True, seed=111),
    # the stem: (20, 41) is the pixel tests/test_backbone.py poisons; (20, 40) has the other column parity,
    # the one a stride-2 kernel's padded eighth tap (column 2 ox + 4) lands on
    "stem7": Layer(3, 64, 7, (37, 70), (20, 41), seam2=(20, 40), stride=2, pad=3, bias=False, seed=8,
                   source="stem7"),
    "stem7_bf16": Layer(3, 64, 7, (37, 70), (20, 41), seam2=(20, 40), stride=2, pad=3, bias=False, bf16=True,
                        seed=8, source="stem7"),
    "front7": Layer(15, 16, 7, (13, 20), (7, 16), seed=65, source="front7"),
    "front7_bf16": Layer(15, 16, 7, (13, 20), (7, 16), bf16=True, seed=65, source="front7"),
    "head1x1": Layer(32, 15, 1, (6, 7), (3, 4), bn=False, relu=False, seed=112),
    "head1x1_relu": Layer(32, 15, 1, (6, 7), (3, 4), bn=False, seed=112),
}


@functools.lru_cache(maxsize=None)
def source_net(source: str, seed: int) -> nn.Module:
    """The seeded network a "stem7" / "front7" layer is cut from (the GPU tests compile it)."""
    import cnn_arch
    from fvp import synthetic

    m = cnn_arch.PoseResNet(18, 15).eval() if source == "stem7" else cnn_arch.P2PNet(15, 15).eval()
    m.load_state_dict(synthetic.seeded_state_dict(m, seed))
    return m


@functools.lru_cache(maxsize=None)
def layer_module(name: str) -> nn.Sequential:
    """Sequential(conv[, BN]) of a case, seeded, eval mode, on the CPU."""
    from fvp import synthetic

    c = LAYERS[name]
    if c.source == "stem7":
        m = source_net(c.source, c.seed)
        return nn.Sequential(m.conv1, m.bn1).eval()
    if c.source == "front7":
        blk = source_net(c.source, c.seed).front_layers[0].block
        return nn.Sequential(blk[0], blk[1]).eval()
    if c.transposed:
        conv = nn.ConvTranspose2d(c.cin, c.cout, c.k, c.stride, c.padding, bias=c.bias)
    else:
        conv = nn.Conv2d(c.cin, c.cout, c.k, c.stride, c.padding, bias=c.bias)
    seq = nn.Sequential(conv, nn.BatchNorm2d(c.cout)) if c.bn else nn.Sequential(conv)
    seq.eval()
    seq.load_state_dict(synthetic.seeded_state_dict(seq, c.seed))
    return seq


@functools.lru_cache(maxsize=None)
def layer_inputs(name: str):
    """(x, r): the clean input in [-0.5, 0.5) (bf16 cases: rounded to bf16) and the residual or None."""
    c = LAYERS[name]
    g = torch.Generator().manual_seed(c.seed)
    x = torch.rand((c.n, c.cin) + c.hw, generator=g) - 0.5
    if c.bf16:
        x = x.to(torch.bfloat16).float()
    r = torch.rand((c.n, c.cout) + c.out_hw, generator=g) if c.res else None
    return x, r


def layer_forward(c: Layer, seq: nn.Module, x, r):
    y = seq(x)
    if c.res == "pre":
        return torch.relu(y + r)
    if c.res == "post":
        return torch.relu(y) + r
    return torch.relu(y) if c.relu else y


@functools.lru_cache(maxsize=None)
def layer_reference(name: str, pos: str | None, value: str | None) -> torch.Tensor:
    """float64 [n][cout][Ho][Wo] of the case with the element at `pos` set to VALUES[value]
    (pos None: the clean input)."""
    c = LAYERS[name]
    x, r = layer_inputs(name)
    if pos is not None:
        x = poison(x, c.where(pos), VALUES[value])
    seq = copy.deepcopy(layer_module(name)).double()
    with torch.no_grad():
        return layer_forward(c, seq, x.double(), None if r is None else r.double())


# ---- P2PNet's fused tail: Upsample2DBlock(48, 20, 2, 2) + skip, then Conv2d(20, 16, 1) ----------
# 3 x 32 pixels into the upsample: fvp_up2_head_nchw takes rows of W % 32 == 0 only, so 32 is
# the narrowest input that reaches it (FvpCNN._tail_nchw returns None for W = 8).
TAIL_SHAPE = dict(n=2, cin=48, cmid=20, j=16, hw=(3, 32))
TAIL_POSITIONS = {
    "input": {"corner": (0, 0), "last": (2, 31), "seam": (1, 16)},     # of x [n][48][3][32]
    "skip": {"corner": (0, 0), "last": (5, 63), "seam": (3, 32)},      # of skip [n][20][6][64]
}


@functools.lru_cache(maxsize=None)
def tail_modules():
    import cnn_arch
    from fvp import synthetic

    s = TAIL_SHAPE
    up = cnn_arch.Upsample2DBlock(s["cin"], s["cmid"], 2, 2).eval()
    head = nn.Conv2d(s["cmid"], s["j"], 1).eval()
    up.load_state_dict(synthetic.seeded_state_dict(up, 113))
    head.load_state_dict(synthetic.seeded_state_dict(head, 114))
    return up, head


@functools.lru_cache(maxsize=None)
def tail_inputs():
    s = TAIL_SHAPE
    g = torch.Generator().manual_seed(115)
    h, w = s["hw"]
    x = torch.rand((s["n"], s["cin"], h, w), generator=g) - 0.3
    skip = torch.rand((s["n"], s["cmid"], 2 * h, 2 * w), generator=g)
    return x, skip


def tail_where(which: str, pos: str):
    s = TAIL_SHAPE
    return (POISONED, (s["cin"] if which == "input" else s["cmid"]) // 2) + TAIL_POSITIONS[which][pos]


def tail_poisoned(which: str | None, pos: str | None, value: str | None):
    x, skip = tail_inputs()
    if which == "input":
        x = poison(x, tail_where(which, pos), VALUES[value])
    elif which == "skip":
        skip = poison(skip, tail_where(which, pos), VALUES[value])
    return x, skip


def tail_window(which: str, pos: str) -> np.ndarray:
    """The output pixels (of 6 x 64) the poisoned element reaches: the 2 x 2 the transposed
    convolution scatters an input pixel to, or the one pixel of a skip element (the head is 1 x 1)."""
    h, w = TAIL_SHAPE["hw"]
    p = TAIL_POSITIONS[which][pos]
    if which == "input":
        return window_mask((h, w), p, 2, 2, 0, transposed=True)
    m = np.zeros((2 * h, 2 * w), bool)
    m[p] = True
    return m


@functools.lru_cache(maxsize=None)
def tail_reference(which: str | None, pos: str | None, value: str | None) -> torch.Tensor:
    up, head = tail_modules()
    x, skip = tail_poisoned(which, pos, value)
    up, head = copy.deepcopy(up).double(), copy.deepcopy(head).double()
    with torch.no_grad():
        return head(up(x.double()) + skip.double())


# ------------------------------------------------------------------------------- whole networks
@dataclass(frozen=True)
class Net:
    kind: str          # "p2p" / "centernet" / "c2c" / "resnet18"
    shape: tuple       # the input
    where: tuple       # the NaN element (image POISONED)
    full: bool         # the reference's image POISONED is NaN everywhere (else: partly)
    seed: int
    bf16: bool = False

    @property
    def rel(self):
        return REL_BF16 if self.bf16 else REL_F32


NETS = {
    "p2p": Net("p2p", (2, 15, 64, 64), (1, 3, 5, 6), False, 11),
    # 40^2 pools to 10^2, where six 3 x 3 layers reach every pixel from any start: fully NaN
    "centernet": Net("centernet", (2, 15, 40, 40), (1, 3, 5, 6), True, 12),
    "c2c_20_end": Net("c2c", (3, 15, 20), (1, 7, 19), True, 14),
    "c2c_20_mid": Net("c2c", (3, 15, 20), (1, 7, 9), True, 14),
    "c2c_64_end": Net("c2c", (3, 15, 64), (1, 7, 63), False, 14),
    "c2c_64_mid": Net("c2c", (3, 15, 64), (1, 7, 31), True, 14),   # mid-column: the field spans all 64
    "resnet18": Net("resnet18", (2, 3, 64, 96), (1, 0, 3, 3), True, 3),
    "resnet18_bf16": Net("resnet18", (2, 3, 64, 96), (1, 0, 3, 3), True, 3, bf16=True),
}


@functools.lru_cache(maxsize=None)
def net_module(kind: str, seed: int) -> nn.Module:
    import cnn_arch
    from fvp import synthetic

    m = {"p2p": lambda: cnn_arch.P2PNet(15, 15), "centernet": lambda: cnn_arch.CenterNet(15, 1),
         "c2c": lambda: cnn_arch.C2CNet(15, 1), "resnet18": lambda: cnn_arch.PoseResNet(18, 15)}[kind]().eval()
    m.load_state_dict(synthetic.seeded_state_dict(m, seed))
    return m


@functools.lru_cache(maxsize=None)
def net_input(name: str, poisoned: bool) -> torch.Tensor:
    c = NETS[name]
    x = torch.rand(c.shape, generator=torch.Generator().manual_seed(c.seed + len(c.shape)))
    if c.bf16:
        x = x.to(torch.bfloat16).float()
    return poison(x, c.where, VALUES["nan"]) if poisoned else x


@functools.lru_cache(maxsize=None)
def net_reference(name: str, poisoned: bool) -> tuple:
    """The float64 outputs (a tuple: CenterNet has two) on the clean or the poisoned input."""
    c = NETS[name]
    x = net_input(name, poisoned)
    if c.kind == "centernet":  # CenterNet.forward takes [B][J][X][Y][Z] and starts with max over Z
        x = x.unsqueeze(4)
    y = reference(net_module(c.kind, c.seed), x)
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)
