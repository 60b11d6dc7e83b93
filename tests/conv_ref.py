"""Float64 reference and a worst-case error bound for the implicit-GEMM convolution kernels
of csrc/fvp_conv.hip -- conv_mfma_kernel (per tap), conv_halo_kernel, conv_bf16_kernel and
conv_dma_kernel -- numpy / torch-CPU only.  tests/test_conv_ref.py pins this file on the
CPU, tests/test_gpu_conv_routes.py holds the kernels to it.

Operation.  mode 0: Conv2d(stride, padding); mode 1: ConvTranspose2d(2, 2); mode 2:
ConvTranspose1d(2, 2) on rows of height 1; mode 3: ConvTranspose2d(4, 2, 1).  Weights in
torch's layout ([Cout, Cin, KH, KW]; transposed [Cin, Cout, kh, kw]), x [N, Cin, H, W].

Reference.  reference() = relu?(scale conv(x) + shift + res_pre) + res_post in float64 from
the float32 values as they are (scale / shift: the folded per-channel values the layer
holds), the convolution by torch.nn.functional.conv2d / conv_transpose2d in float64
(checked against conv_def, loops over the definition, in tests/test_conv_ref.py).  bf16
operands: x and w are first rounded to bf16 (round to nearest even, what the kernels' casts
and Tensor.to(torch.bfloat16) both do); their products are exact in fp32.

Bound.  With Babs = conv(|x|, |w|) and K = KH KW Cpi products per output (KH = KW = 2 for
mode 3, 1 for modes 1 and 2; Cpi the padded input channels), u = 2^-24,

    tol = c (K + 8) u (|scale| Babs + |shift| + |res_pre| + |res_post|),   c = 1 (fp32), 2 (bf16)

the first-order worst case of K roundings of partial sums in any summation order (each
partial sum is at most Babs in magnitude; split-K's extra adds and the epilogue's few are
the + 8); c = 2 allows a matrix instruction that chops its internal adds.  ReLU is
1-Lipschitz.  Derived, not measured: an error above it is a defect of the kernel.

Emulation.  emulate() evaluates the same sums in float32, one rounding per product-add, in
the kernels' orders: "tap" (tap-major, channels within: per-tap, bf16 and DMA kernels),
"chunk" (16-channel chunk-major, taps within: the halo kernel), split-K slices of the K
chunks summed in z order -- and takes a planted fault (FAULTS).  It shows on the CPU that a
correct fp32 evaluation stays inside tol and that each fault leaves it.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
REL = 2e-5  # tests/test_cnn.py's criterion: max error of the output's max magnitude

FAULTS = ("tap", "chunk", "row", "shift", "res", "parity", "seam", "twice")


def rup(x, m):
    return (x + m - 1) // m * m


def bf16_round(a):
    """float32 array rounded to bf16 (nearest even), as float32."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def w4(w, mode):
    """Weights as 4-D float array (ConvTranspose1d's [Cin, Cout, 2] -> [Cin, Cout, 1, 2])."""
    w = np.asarray(w)
    return w[:, :, None, :] if w.ndim == 3 else w


def out_hw(H, W, KH, KW, mode, stride, pad):
    if mode == 0:
        return (H + 2 * pad[0] - KH) // stride[0] + 1, (W + 2 * pad[1] - KW) // stride[1] + 1
    return (H if mode == 2 else 2 * H), 2 * W


def k_products(w, mode, cpi):
    """K of the bound: products per output element over the padded input channels."""
    w = w4(w, mode)
    taps = {0: w.shape[2] * w.shape[3], 1: 1, 2: 1, 3: 4}[mode]
    return taps * cpi


def conv_raw(x, w, mode, stride=(1, 1), pad=(0, 0)):
    """The convolution without bias in float64 (torch CPU): [N, Cout, Ho, Wo]."""
    xt = torch.from_numpy(np.asarray(x, np.float64))
    wt = torch.from_numpy(np.asarray(w4(w, mode), np.float64))
    if mode == 0:
        y = F.conv2d(xt, wt, stride=tuple(stride), padding=tuple(pad))
    elif mode == 1:
        y = F.conv_transpose2d(xt, wt, stride=2)
    elif mode == 2:
        y = F.conv_transpose2d(xt, wt, stride=(1, 2))
    else:
        y = F.conv_transpose2d(xt, wt, stride=2, padding=1)
    return y.numpy()


def conv_def(x, w, mode, stride=(1, 1), pad=(0, 0)):
    """The same from the definitions, loops over taps and pixels in float64 (tiny shapes):
    Conv2d  out[co][oy][ox] = sum x[ci][oy sy - py + ky][ox sx - px + kx] w[co][ci][ky][kx];
    ConvTranspose  out[co][iy s - p + ky][ix s' - p + kx] += x[ci][iy][ix] w[ci][co][ky][kx]."""
    x, w = np.asarray(x, np.float64), np.asarray(w4(w, mode), np.float64)
    n, _, h, wd = x.shape
    kh, kw = w.shape[2:]
    ho, wo = out_hw(h, wd, kh, kw, mode, stride, pad)
    out = np.zeros((n, w.shape[0] if mode == 0 else w.shape[1], ho, wo))
    if mode == 0:
        for oy in range(ho):
            for ox in range(wo):
                for ky in range(kh):
                    for kx in range(kw):
                        y, xx = oy * stride[0] - pad[0] + ky, ox * stride[1] - pad[1] + kx
                        if 0 <= y < h and 0 <= xx < wd:
                            out[:, :, oy, ox] += x[:, :, y, xx] @ w[:, :, ky, kx].T
        return out
    s, p = ((2, 2), 0) if mode == 1 else ((1, 2), 0) if mode == 2 else ((2, 2), 1)
    for iy in range(h):
        for ix in range(wd):
            for ky in range(kh):
                for kx in range(kw):
                    y, xx = iy * s[0] - p + ky, ix * s[1] - p + kx
                    if 0 <= y < ho and 0 <= xx < wo:
                        out[:, :, y, xx] += x[:, :, iy, ix] @ w[:, :, ky, kx]
    return out


def epilogue(acc, scale, shift, relu, res_pre, res_post):
    v = acc * scale[None, :, None, None] + shift[None, :, None, None]
    if res_pre is not None:
        v = v + res_pre.astype(v.dtype)
    if relu:
        v = np.maximum(v, 0)
    if res_post is not None:
        v = v + res_post.astype(v.dtype)
    return v


def _operands(x, w, bf16):
    return (bf16_round(x), bf16_round(w)) if bf16 else (np.asarray(x, np.float32), np.asarray(w, np.float32))


def reference(x, w, scale, shift, mode, stride=(1, 1), pad=(0, 0), relu=True, res_pre=None, res_post=None,
              bf16=False):
    """float64 [N, Cout, Ho, Wo].  bf16: bf16 operands (x and w rounded first)."""
    x, w = _operands(x, w, bf16)
    f64 = np.float64
    return epilogue(conv_raw(x, w, mode, stride, pad), np.asarray(scale, f64), np.asarray(shift, f64), relu,
                    None if res_pre is None else np.asarray(res_pre, f64),
                    None if res_post is None else np.asarray(res_post, f64))


def tolerance(x, w, scale, shift, mode, stride=(1, 1), pad=(0, 0), res_pre=None, res_post=None, bf16=False,
              cpi=None):
    """The elementwise bound of the module docstring, float64, shaped as the output."""
    x, w = _operands(x, w, bf16)
    cpi = rup(x.shape[1], 16) if cpi is None else cpi
    t = np.abs(np.asarray(scale, np.float64))[None, :, None, None] * conv_raw(np.abs(x), np.abs(w), mode, stride, pad)
    t = t + np.abs(np.asarray(shift, np.float64))[None, :, None, None]
    for r in (res_pre, res_post):
        if r is not None:
            t = t + np.abs(np.asarray(r, np.float64))
    return (2 if bf16 else 1) * (k_products(w, mode, cpi) + 8) * U * t


def close_ratio(got, ref):
    """tests/test_cnn.py's criterion as a ratio: max error over REL of the output scale."""
    scale = max(float(np.abs(ref).max()), 1e-6)
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / scale / REL


# ---- fp32 emulation of the kernels' accumulation -----------------------------------------
def _groups(w, mode, stride, pad):
    """The GEMMs of one launch: [(taps, output slice)] with taps = [(dy, dx, Wt [Cout, Cin])]:
    GEMM-row pixel (y, x) reads input (y sy + dy, x sx + dx).  Mode 0 is one group; modes 1
    and 2 one 1x1 tap per output parity; mode 3 four 2x2 convolutions, group g = 2 ry + rx,
    tap (i, j) = W[ci][co][3 - 2i - ry][3 - 2j - rx] at input (y - 1 + ry + i, x - 1 + rx + j)."""
    w = w4(w, mode)
    if mode == 0:
        return [([(ky - pad[0], kx - pad[1], w[:, :, ky, kx]) for ky in range(w.shape[2]) for kx in range(w.shape[3])],
                 (slice(None), slice(None)))]
    if mode == 1:
        return [([(0, 0, w[:, :, dy, dx].T)], (slice(dy, None, 2), slice(dx, None, 2)))
                for dy in (0, 1) for dx in (0, 1)]
    if mode == 2:
        return [([(0, 0, w[:, :, 0, dx].T)], (slice(None), slice(dx, None, 2))) for dx in (0, 1)]
    return [([(ry + i - 1, rx + j - 1, w[:, :, 3 - 2 * i - ry, 3 - 2 * j - rx].T) for i in (0, 1) for j in (0, 1)],
             (slice(ry, None, 2), slice(rx, None, 2))) for ry in (0, 1) for rx in (0, 1)]


def _shifted(x, dy, dx, hm, wm, sy, sx):
    """[N, Cin, hm, wm]: x at (y sy + dy, x sx + dx), zero outside."""
    n, c, h, w = x.shape
    out = np.zeros((n, c, hm, wm), x.dtype)
    ys = [y for y in range(hm) if 0 <= y * sy + dy < h]
    xs = [v for v in range(wm) if 0 <= v * sx + dx < w]
    if ys and xs:
        out[:, :, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = \
            x[:, :, ys[0] * sy + dy:ys[-1] * sy + dy + 1:sy, xs[0] * sx + dx:xs[-1] * sx + dx + 1:sx]
    return out


def emulate(x, w, scale, shift, mode, stride=(1, 1), pad=(0, 0), relu=True, res_pre=None, res_post=None,
            bf16=False, cpi=None, order="tap", kc=16, ks=1, bn=64, fault=None):
    """The kernels' accumulation in float32; float32 [N, Cout, Ho, Wo] (NaN where the fault
    leaves an element unwritten, as the GPU test pre-fills its output).
    order "tap" | "chunk"; kc: K depth of one chunk; ks: split-K slices (of the kc-deep chunk
    sequence, slice z = chunks [z n / ks, (z + 1) n / ks), summed in z order); bn: column tile
    (fault "shift").  Faults, planted in image 0 unless said otherwise:
      tap     the tap that reads the pixel itself (offset 0, 0) is not added on output row 0
      chunk   the last K chunk is not added
      row     the last GEMM row (last pixel of the last image) is not written
      shift   the channels of the last column tile are rotated by one
      res     res_pre and res_post change places
      parity  (mode 3) parity groups 1 and 2 change places
      seam    the first GEMM row of image 1 is computed from image 0
      twice   (ks > 1) the last split-K slice is added twice"""
    assert fault is None or fault in FAULTS, fault
    f32 = np.float32
    x, w = _operands(x, w, bf16)
    n, cin, h, wd = x.shape
    cpi = rup(cin, 16) if cpi is None else cpi
    groups = _groups(w, mode, stride, pad)
    if fault == "parity":
        assert mode == 3
        groups = [(groups[i][0], groups[j][1]) for i, j in ((0, 0), (1, 2), (2, 1), (3, 3))]
    kh, kw = w4(w, mode).shape[2:]
    ho, wo = out_hw(h, wd, kh, kw, mode, stride, pad)
    hm, wm = (ho, wo) if mode == 0 else (h, wd)
    sy, sx = stride if mode == 0 else (1, 1)
    cout = groups[0][0][0][2].shape[0]
    acc = np.zeros((n, cout, ho, wo), f32)
    for taps, osl in groups:
        # the K sequence: (tap, channel) pairs in the kernel's order, in chunks of kc (padding
        # channels are zeros: they add nothing and are left out, but count in the chunking)
        if order == "tap":
            seq = [(t, c) for t in range(len(taps)) for c in range(cpi)]
        else:
            seq = [(t, c) for c0 in range(0, cpi, 16) for t in range(len(taps)) for c in range(c0, c0 + 16)]
        chunks = [seq[i:i + kc] for i in range(0, len(seq), kc)]
        if fault == "chunk":
            dropped, chunks = chunks[-1], chunks[:-1] + [[]]
        xs = [_shifted(x, dy, dx, hm, wm, sy, sx) for dy, dx, _ in taps]
        t0 = [(dy, dx) for dy, dx, _ in taps].index((0, 0))
        parts = []
        for z in range(ks):
            part = np.zeros((n, cout, hm, wm), np.float64)  # holds float32 values
            for chunk in chunks[z * len(chunks) // ks:(z + 1) * len(chunks) // ks]:
                for t, c in chunk:
                    if c >= cin:
                        continue
                    term = taps[t][2][None, :, c, None, None].astype(np.float64) * xs[t][:, None, c].astype(np.float64)
                    if fault == "tap" and t == t0:
                        term[0, :, 0, :] = 0
                    part = (part + term).astype(f32).astype(np.float64)  # one rounding per product-add
            parts.append(part)
        if fault == "chunk":  # (only image 0 loses it)
            full = parts[-1]
            for t, c in dropped:
                if c < cin:
                    term = taps[t][2][None, :, c, None, None].astype(np.float64) * xs[t][:, None, c].astype(np.float64)
                    term[0] = 0
                    full = (full + term).astype(f32).astype(np.float64)
            parts[-1] = full
        if fault == "twice":
            assert ks > 1
            parts.append(parts[-1])
        tot = parts[0]
        for p in parts[1:]:
            tot = (tot + p).astype(f32).astype(np.float64)
        if fault == "seam":
            assert n > 1
            tot[1, :, 0, 0] = tot[0, :, 0, 0]
        acc[(slice(None), slice(None)) + osl] = tot.astype(f32)
    if fault == "res":
        assert res_pre is not None and res_post is not None
        res_pre, res_post = res_post, res_pre
    # the epilogue in float32: acc * scale + shift (+ res_pre), ReLU, (+ res_post)
    out = epilogue(acc, np.asarray(scale, f32), np.asarray(shift, f32), relu,
                   None if res_pre is None else np.asarray(res_pre, f32),
                   None if res_post is None else np.asarray(res_post, f32))
    assert out.dtype == f32
    if fault == "shift":
        c0 = (cout - 1) // bn * bn
        out[:, c0:] = np.roll(out[:, c0:], 1, axis=1)
    if fault == "row":
        out[-1, :, -1, -1] = np.nan
    return out
