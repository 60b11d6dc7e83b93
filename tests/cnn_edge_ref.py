"""Float64 references, derived bounds, criteria and fp32 emulations with planted faults for
the hand-tiled kernels at the two ends of the networks (csrc/fvp_conv.hip): the 7x7 stems
(conv_stem7_f32 / _bf16, stride 2), the 7x7 front layers (conv_front7_f32 / _bf16, stride
1), the NCHW 1x1 head (conv1x1_nchw<4|8|16>) and P2PNet's fused tail (up2_head_nchw).
numpy / torch-CPU only.  tests/test_cnn_edge_ref.py pins this file on the CPU,
tests/test_gpu_cnn_edges.py holds the kernels to it; the cases are tests/cnn_edge_cases.py.

Reference and bound: tests/conv_ref.py's, tol = c (K + 8) u (|scale| Babs + |shift| [+
|skip|]), u = 2^-24, c = 1 (fp32 operands), 2 (bf16 operands, the reference taken on the
bf16-rounded operands).  K is the products of one output over the channel pitch the kernel
walks: 49 x 4 = 196 for the stems (the real count at C = 4, an upper bound below: zero rows
and zero taps add no rounding), 49 x 16 = 784 for the front layers, 4 t4 = 16 / 32 / 64 for
the 1x1 head (its fma chain: t4 float4s per pixel).  The fused tail has two stages, both
first order:

    y_ref = relu(scale D + shift) + skip                  tol_y = conv_ref.tolerance(mode 1, Cpi)
    ref   = hscale sum_co y_ref Wh + hshift
    tol   = |hscale| sum_co |Wh| tol_y + (32 + 8) u (|hscale| sum_co (|y_ref| + tol_y) |Wh| + |hshift|)

(the head's error from y's error, plus the head's own 32 product-adds on values that large).

Criteria.  fp32 outputs: |got - ref| <= tol on every element; an element that is not finite
(a NaN left from the pre-fill: never written) counts as infinite error.  bf16 outputs: with
pre = reference(..., relu=False) on bf16-rounded operands, g is right iff

    bf16(max(pre - tol, 0)) <= g <= bf16(max(pre + tol, 0))

bf16() being Tensor.to(torch.bfloat16) (monotone, like the ReLU: g is the bf16 rounding of
the ReLU of some value within the derived bound).  The interval is taken before the ReLU: an
element the ReLU cuts has the one-value interval [0, 0].  Cap (half_ref.CAP, a condition on
a case): at most that share of a case's elements may have an interval of more than one value.

Emulations.  emulate7 / emulate1x1 / emulate_tail evaluate the operations in float32 (torch
CPU; bf16 operands rounded first, their products exact in fp32) and take a planted fault.
Inputs are read as the GPU test lays them out: a contiguous tensor with NaN beyond its end.
FAULTS7 (stems and front layers):
  tap    the tap (ky, kx) = (6, 6) is dropped
  wrap   a column x >= W reads on in the flat tensor (the next row's first pixels) instead of padding
  plane  a plane c >= C (below the kernel's plane count) reads the next image's first planes
         instead of zero: their weights are zero, so only the NaN after the last image shows
  swap   tile x and y change places in the decode (y = t % tiles_x, x = t / tiles_x)
  seam   the first tile of image 1 is computed from image 0
  row    the last output row of the last tile is not written
  ho     (stems) Ho = H / 2 for odd H
  rtz    (bf16 outputs) the conversion rounds toward zero
FAULTS1X1:  wrow  the weight row Cin (a padding row) is 1;  pixel  the last pixel of image 0
is written to image 1's plane.
FAULTS_TAIL:  skip1  the skip is left out of the last real channel;  class  the parity
classes (ry, rx) 1 and 2 change places;  noskip  the head reads y before the skip is added.
"""
import collections

import numpy as np
import torch
import torch.nn.functional as F

import conv_ref as R
import half_ref as HR

U = R.U
CAP = HR.CAP

# planes: the input planes the kernel's loader visits (zero past C); cpi: the bound's channel pitch
Kernel = collections.namedtuple("Kernel", "name fn stride th tw planes cpi cout bf16")
KERNELS = {k.name: k for k in (
    Kernel("stem7_f32", "fvp_conv_stem7_f32", 2, 8, 32, 3, 4, 64, False),
    Kernel("stem7_bf16", "fvp_conv_stem7_bf16", 2, 8, 32, 4, 4, 64, True),
    Kernel("front7_f32", "fvp_conv_front7_f32", 1, 8, 16, 16, 16, 16, False),
    Kernel("front7_bf16", "fvp_conv_front7_bf16", 1, 8, 32, 16, 16, 16, True),
)}

FAULTS7 = ("tap", "wrap", "plane", "swap", "seam", "row", "ho", "rtz")
FAULTS1X1 = ("wrow", "pixel")
FAULTS_TAIL = ("skip1", "class", "noskip")


def out_hw7(k, H, W):
    return (H - 1) // k.stride + 1, (W - 1) // k.stride + 1


def tiles7(k, H, W):
    """(tiles_y, tiles_x) of one image."""
    ho, wo = out_hw7(k, H, W)
    return -(-ho // k.th), -(-wo // k.tw)


# ---- criteria ----------------------------------------------------------------------------
def ratio(got, ref, tol):
    """Elementwise err / tol, infinite where got is not finite."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    err[~np.isfinite(err)] = np.inf
    return err / tol


def bf16(a):
    """float array -> bf16 values (Tensor.to(torch.bfloat16): nearest even) as float64."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(torch.bfloat16).double().numpy()


def bf16_rtz(a):
    """float32 array -> bf16 values rounded toward zero (the planted fault), as float64."""
    bits = np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return bits.view(np.float32).astype(np.float64)


def interval(pre, tol):
    return bf16(np.maximum(pre - tol, 0)), bf16(np.maximum(pre + tol, 0))


def inside(g, pre, tol):
    """Elementwise: the bf16 values g (any float array) meet the criterion (a NaN never does)."""
    g = np.asarray(g, np.float64)
    lo, hi = interval(pre, tol)
    return (lo <= g) & (g <= hi)


def wide_share(pre, tol):
    lo, hi = interval(pre, tol)
    return float(np.mean(lo != hi))


# ---- the 7x7 kernels ---------------------------------------------------------------------
def ref7(k, x, w, scale, shift):
    """(ref, tol, pre) float64 [N, Cout, Ho, Wo]: with and without the ReLU (bf16 kernels: on
    bf16-rounded operands)."""
    kw = dict(stride=(k.stride, k.stride), pad=(3, 3), bf16=k.bf16)
    pre = R.reference(x, w, scale, shift, 0, relu=False, **kw)
    return np.maximum(pre, 0), R.tolerance(x, w, scale, shift, 0, cpi=k.cpi, **kw), pre


def faults7(k, N, C, H, W):
    """The planted faults that show on a case of this shape."""
    ty, tx = tiles7(k, H, W)
    f = ["wrap", "row"]
    if H >= 4 and W >= 4:  # else the tap reads padding at every output
        f.append("tap")
    if C < k.planes:
        f.append("plane")
    if ty != tx:
        f.append("swap")
    if N >= 2:
        f.append("seam")
    if k.stride == 2 and H % 2:
        f.append("ho")
    ho, wo = out_hw7(k, H, W)
    if k.bf16 and N * ho * wo * k.cout >= 512:  # (half of the positive elements round the other way)
        f.append("rtz")
    return f


def emulate7(k, x, w, scale, shift, fault=None):
    """float32 evaluation of a 7x7 kernel, [N, Cout, Ho, Wo]: float32 (fp32 kernels) or the
    bf16 values as float64 (bf16 kernels); NaN where the fault leaves an element unwritten or
    lets the NaN beyond the input reach it."""
    assert fault is None or fault in FAULTS7, fault
    f32 = np.float32
    xo, wo_ = (R.bf16_round(x), R.bf16_round(w)) if k.bf16 else (np.asarray(x, f32), np.asarray(w, f32))
    n, c, h, wd = xo.shape
    s = k.stride
    ho, wo = out_hw7(k, h, wd)
    xp = np.zeros((n, c, h + 6, wd + 6), f32)  # the padding, spelled out
    xp[:, :, 3:3 + h, 3:3 + wd] = xo
    if fault == "wrap":
        flat = np.concatenate([xo.reshape(-1), np.full(3, np.nan, f32)])
        row0 = np.arange(n * c * h).reshape(n, c, h) * wd
        for d in range(3):
            xp[:, :, 3:3 + h, 3 + wd + d] = flat[row0 + wd + d]
    wt = wo_.copy()
    if fault == "tap":
        wt[:, :, 6, 6] = 0
    poison = np.isnan(xp)
    acc = F.conv2d(torch.from_numpy(np.where(poison, f32(0), xp)), torch.from_numpy(wt), stride=s).numpy()
    bad = F.conv2d(torch.from_numpy(poison.any(axis=1, keepdims=True).astype(f32)), torch.ones(1, 1, 7, 7),
                   stride=s).numpy() > 0
    if fault == "plane":  # every window holds a pixel of the image; past the last image it reads NaN (x 0 = NaN)
        assert c < k.planes
        bad[n - 1] = True
    assert acc.dtype == f32 and acc.shape == (n, k.cout, ho, wo)
    v = np.maximum(acc * np.asarray(scale, f32)[None, :, None, None] + np.asarray(shift, f32)[None, :, None, None], 0)
    assert v.dtype == f32
    out = (bf16_rtz(v) if fault == "rtz" else bf16(v)) if k.bf16 else v.copy()
    out[np.broadcast_to(bad, out.shape)] = np.nan
    ty, tx = tiles7(k, h, wd)
    if fault == "swap":  # each tile is right for the origin it decodes; the origins are the wrong set
        done = {(t % tx, t // tx) for t in range(ty * tx)}
        for y in range(ty):
            for xx in range(tx):
                if (y, xx) not in done:
                    out[:, :, y * k.th:(y + 1) * k.th, xx * k.tw:(xx + 1) * k.tw] = np.nan
    if fault == "seam":
        assert n > 1
        out[1, :, :k.th, :k.tw] = out[0, :, :k.th, :k.tw]
    if fault == "row":
        out[n - 1, :, ho - 1, (tx - 1) * k.tw:] = np.nan
    if fault == "ho":  # fewer rows, written at their own pitch into the buffer of the right size
        assert s == 2 and h % 2
        part = np.ascontiguousarray(out.transpose(0, 2, 3, 1)[:, :h // 2]).reshape(-1)
        buf = np.full(out.size, np.nan, out.dtype)
        buf[:part.size] = part
        out = np.ascontiguousarray(buf.reshape(n, ho, wo, k.cout).transpose(0, 3, 1, 2))
    return out


# ---- the 1x1 head ------------------------------------------------------------------------
def t4_of(cin):
    return 4 if cin <= 16 else 8 if cin <= 32 else 16


def ref1x1(x, w, scale, shift, relu):
    """(ref, tol) float64 [N, Cout, H, W]; x [N, Cin, H, W], w [Cout, Cin]."""
    w = np.asarray(w)[:, :, None, None]
    return (R.reference(x, w, scale, shift, 0, relu=bool(relu)),
            R.tolerance(x, w, scale, shift, 0, cpi=4 * t4_of(x.shape[1])))


def emulate1x1(rows, c0, cin, w, scale, shift, relu, fault=None):
    """float32 [N, Cout, H, W] from the NHWC rows [N, H, W, Cp] as the kernel is given them
    (every channel, the ones outside c0 .. c0 + cin - 1 included)."""
    assert fault is None or fault in FAULTS1X1, fault
    xt = torch.from_numpy(np.ascontiguousarray(rows[..., c0:c0 + cin], np.float32))
    acc = torch.einsum("nhwc,jc->njhw", xt, torch.from_numpy(np.asarray(w, np.float32)))
    if fault == "wrow":
        assert cin < 4 * t4_of(cin)
        acc = acc + torch.from_numpy(np.ascontiguousarray(rows[..., c0 + cin], np.float32))[:, None]
    v = acc * torch.from_numpy(np.asarray(scale, np.float32))[None, :, None, None] \
        + torch.from_numpy(np.asarray(shift, np.float32))[None, :, None, None]
    out = (torch.relu(v) if relu else v).numpy().copy()
    assert out.dtype == np.float32
    if fault == "pixel":
        assert out.shape[0] > 1
        out[1, :, -1, -1] = out[0, :, -1, -1]
        out[0, :, -1, -1] = np.nan
    return out


# ---- the fused tail ----------------------------------------------------------------------
def ref_tail(x, w, scale, shift, skip, wh, hscale, hshift):
    """(ref, tol) float64 [N, J, 2H, 2W]; x [N, Cpi, H, W], w [Cpi, Cs, 2, 2] (ConvTranspose2d),
    skip [N, Cs, 2H, 2W], wh [J, Cs]."""
    cpi = x.shape[1]
    assert cpi % 16 == 0
    y = R.reference(x, w, scale, shift, 1, relu=True, res_post=skip)
    ty = R.tolerance(x, w, scale, shift, 1, res_post=skip, cpi=cpi)
    wh = np.asarray(wh, np.float64)
    hs, hb = (np.asarray(v, np.float64)[None, :, None, None] for v in (hscale, hshift))
    ref = hs * np.einsum("nchw,jc->njhw", y, wh) + hb
    tol = np.abs(hs) * np.einsum("nchw,jc->njhw", ty, np.abs(wh)) \
        + (32 + 8) * U * (np.abs(hs) * np.einsum("nchw,jc->njhw", np.abs(y) + ty, np.abs(wh)) + np.abs(hb))
    return ref, tol


def emulate_tail(x, w, scale, shift, skip, wh, hscale, hshift, fault=None):
    """The two stages in float32, [N, J, 2H, 2W]."""
    assert fault is None or fault in FAULTS_TAIL, fault
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))  # noqa: E731
    wt = t(w)
    if fault == "class":
        wt = wt.clone()
        wt[:, :, 0, 1], wt[:, :, 1, 0] = t(w)[:, :, 1, 0], t(w)[:, :, 0, 1]
    y = F.conv_transpose2d(t(x), wt, stride=2) * t(scale)[None, :, None, None] + t(shift)[None, :, None, None]
    y = torch.relu(y)
    sk = t(skip).clone()
    if fault == "skip1":
        sk[:, -1] = 0
    if fault != "noskip":
        y = y + sk
    z = torch.einsum("nchw,jc->njhw", y, t(wh)) * t(hscale)[None, :, None, None] + t(hshift)[None, :, None, None]
    assert z.dtype == torch.float32
    return z.numpy()
