"""Float64 references and a worst-case error bound for the two Winograd kernels of
csrc/fvp_wino.hip (numpy / torch-CPU only; tests/test_wino_ref.py pins this file on the
CPU, tests/test_gpu_wino_grids.py holds the kernels to it).

Reference.  conv3x3_ref / deconv4s2_ref evaluate Conv2d(3, 1, 1) / ConvTranspose2d(4, 2, 1)
from their definitions in float64, then the eval BatchNorm with the conv bias, then
``+ res_pre``, the optional ReLU and ``+ res_post`` (the epilogue of fvp_conv2d_nhwc_ex).

Bound.  The kernels compute out = A^T [ sum_c (G w_c G^T) . (B^T d_c B) ] A per 2 x 2 tile.
Running the same algorithm with every matrix and operand replaced by its absolute value,

    Babs = |A^T| [ sum_c |G w_c G^T| . (|B^T| |d_c| |B|) ] |A|,

bounds the magnitude of every intermediate that reaches an output, so one fp32 rounding
anywhere on the way moves the output by at most u Babs (u = 2^-24).  An output passes
through at most Cpi accumulation roundings, 2 for the input transform, 1 for the fp32
rounding of U = G w G^T, 4 for the output transform and a few for the BatchNorm fold and the
epilogue, so

    tol = (Cpi + 16) u (|scale| Babs + |shift| + |res_pre| + |res_post|)

with scale / shift the float64 BatchNorm fold.  ReLU is 1-Lipschitz, so the same tol holds
after it.  The bound is derived, not measured: an error above it is a defect of the kernel.

Emulation.  emulate() runs both algorithms in numpy with a float32 rounding after every
operation, in the operation order of the kernels (U from float64, rounded once), and takes
a planted fault: "drop" (one transform position of one input channel of one tile is lost),
"swap" (two tiles of one block change places) and "wrap" (the pixel past the right image
edge is read from the next row of the NHWC tensor, not as zero).  It exists to show on the
CPU that a correct fp32 evaluation stays inside tol and that each fault leaves it.
"""
import numpy as np

U = 2.0 ** -24
REL = 2e-5  # tests/test_cnn.py's criterion: max error of the output's max magnitude

# F(2x2, 3x3): the matrices in the head comment of csrc/fvp_wino.hip
CONV_BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
CONV_G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
CONV_AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
# F(2x2, 2x2) per output parity: the matrices in the comment above deconv_wino_kernel
DECONV_BT = np.array([[1, -1, 0], [0, 1, 0], [0, -1, 1]], np.float64)
DECONV_G = np.array([[1, 0], [1, 1], [0, 1]], np.float64)
DECONV_AT = np.array([[1, 1, 0], [0, 1, 1]], np.float64)

FAULTS = ("drop", "swap", "wrap")


def rup(x, m):
    return (x + m - 1) // m * m


def params(conv, bn):
    """The float32 parameters of a conv (+ eval BatchNorm) as numpy arrays, unchanged."""
    p = {"w": conv.weight.detach().cpu().numpy(), "transposed": conv.weight.shape[2] == 4}
    cout = p["w"].shape[1 if p["transposed"] else 0]
    p["bias"] = conv.bias.detach().cpu().numpy() if conv.bias is not None else np.zeros(cout, np.float32)
    for k, t in (("gamma", bn.weight), ("beta", bn.bias), ("mean", bn.running_mean), ("var", bn.running_var)):
        p[k] = t.detach().cpu().numpy()
    p["eps"] = float(bn.eps)
    return p


def bn_fold(p, dtype=np.float64):
    """(scale, shift) of the conv bias and the eval BatchNorm, in ``dtype`` (float32: the
    operation sequence of fvp.cnn.ConvLayer)."""
    f = {k: p[k].astype(dtype) for k in ("bias", "gamma", "beta", "mean", "var")}
    scale = f["gamma"] / np.sqrt(f["var"] + dtype(p["eps"]))
    return scale, (f["bias"] - f["mean"]) * scale + f["beta"]


def epilogue(acc, scale, shift, relu, res_pre, res_post):
    v = acc * scale[None, :, None, None] + shift[None, :, None, None]
    if res_pre is not None:
        v = v + res_pre.astype(v.dtype)
    if relu:
        v = np.maximum(v, 0)
    if res_post is not None:
        v = v + res_post.astype(v.dtype)
    return v


# ---- the operations from their definitions -------------------------------------------------
def _gemm_taps(xp, w_taps, offsets, h, wd):
    """sum over taps t of w_taps[t] [Cout, Cin] applied to xp [N, Cin, ., .] shifted by
    offsets[t], as one GEMM over (tap, channel): [N, Cout, h, wd]."""
    n, c = xp.shape[:2]
    cols = np.stack([xp[:, :, i:i + h, j:j + wd] for i, j in offsets], axis=1)  # [N][taps][Cin][h][wd]
    cols = cols.transpose(1, 2, 0, 3, 4).reshape(len(offsets) * c, n * h * wd)
    wm = np.concatenate(w_taps, axis=1)  # [Cout][taps * Cin]
    return np.matmul(wm, cols).reshape(-1, n, h, wd).transpose(1, 0, 2, 3)


def _pad1(x):
    x = np.asarray(x, np.float64)
    xp = np.zeros(x.shape[:2] + (x.shape[2] + 2, x.shape[3] + 2))
    xp[:, :, 1:-1, 1:-1] = x
    return xp


def conv3x3_raw(x, w):
    """Conv2d(3, stride 1, padding 1) without bias in float64: x [N, Cin, H, W], w [Cout, Cin, 3, 3];
    out[y][x] = sum w[i][j] in[y - 1 + i][x - 1 + j]."""
    w = np.asarray(w, np.float64)
    taps = [(i, j) for i in range(3) for j in range(3)]
    return np.ascontiguousarray(_gemm_taps(_pad1(x), [w[:, :, i, j] for i, j in taps], taps, x.shape[2], x.shape[3]))


def deconv4s2_scatter(x, w):
    """ConvTranspose2d(4, stride 2, padding 1) without bias in float64 from its definition:
    x [N, Cin, H, W], w [Cin, Cout, 4, 4]; out[2 iy - 1 + ky][2 ix - 1 + kx] += x[iy][ix] w[ky][kx]."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, c, h, wd = x.shape
    buf = np.zeros((n, w.shape[1], 2 * h + 2, 2 * wd + 2))  # output position p at index p + 1
    xf = x.reshape(n, c, h * wd)
    for ky in range(4):
        for kx in range(4):
            buf[:, :, ky:ky + 2 * h:2, kx:kx + 2 * wd:2] += \
                np.matmul(w[:, :, ky, kx].T[None], xf).reshape(n, w.shape[1], h, wd)
    return buf[:, :, 1:-1, 1:-1]


def deconv4s2_raw(x, w):
    """The same sum gathered per output pixel (one GEMM per output parity, fast on large
    batches): out[oy][ox] = sum over ky, kx with oy + 1 - ky and ox + 1 - kx even of
    x[(oy + 1 - ky) / 2][(ox + 1 - kx) / 2] w[ky][kx]."""
    w = np.asarray(w, np.float64)
    n, c, h, wd = x.shape
    xp = _pad1(x)
    out = np.zeros((n, w.shape[1], 2 * h, 2 * wd))
    for py in range(2):
        for px in range(2):
            # oy = 2 y + py: ky = py + 1 - 2 dy for iy = y + dy, dy in {-1, 0, 1} where 0 <= ky < 4
            taps = [(dy, dx, py + 1 - 2 * dy, px + 1 - 2 * dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                    if 0 <= py + 1 - 2 * dy < 4 and 0 <= px + 1 - 2 * dx < 4]
            out[:, :, py::2, px::2] = _gemm_taps(xp, [w[:, :, ky, kx].T for _, _, ky, kx in taps],
                                                 [(1 + dy, 1 + dx) for dy, dx, _, _ in taps], h, wd)
    return out


def _ref(raw, x, conv, bn, relu, res_pre, res_post):
    p = params(conv, bn)
    scale, shift = bn_fold(p)
    return epilogue(raw(x, p["w"]), scale, shift, relu, res_pre, res_post)


def conv3x3_ref(x, conv, bn, relu=True, res_pre=None, res_post=None):
    """float64 [N, Cout, H, W]: relu?(BN(conv(x)) + res_pre) + res_post."""
    return _ref(conv3x3_raw, x, conv, bn, relu, res_pre, res_post)


def deconv4s2_ref(x, conv, bn, relu=True, res_pre=None, res_post=None):
    """float64 [N, Cout, 2H, 2W]: relu?(BN(conv_transpose(x)) + res_pre) + res_post."""
    return _ref(deconv4s2_raw, x, conv, bn, relu, res_pre, res_post)


# ---- the Winograd algorithms in float64 ----------------------------------------------------
def _patches(xp, k, ty, tx, oy, ox):
    """[k][k][C][N * ty * tx]: element (r, s) of the k x k patch of tile (i, j) of xp [C][N][.][.],
    xp[oy + 2i + r][ox + 2j + s]."""
    c, n = xp.shape[:2]
    return np.stack([np.stack([xp[:, :, oy + r:oy + r + 2 * ty:2, ox + s:ox + s + 2 * tx:2].reshape(c, n * ty * tx)
                               for s in range(k)]) for r in range(k)])


def _padded(x, ty, tx, wrap=False):
    """x [N][C][H][W] as [C][N][2 ty + 2][2 tx + 2] with one zero row / column before and
    zeros after.  wrap: the pixel past the right edge of row y holds what follows it in
    memory, the first pixel of the next row (of the next image after the last row; zero at
    the end)."""
    n, c, h, w = x.shape
    xp = np.zeros((c, n, 2 * ty + 2, 2 * tx + 2), x.dtype)
    xp[:, :, 1:h + 1, 1:w + 1] = x.transpose(1, 0, 2, 3)
    if wrap:
        xp[:, :, 1:h, w + 1] = xp[:, :, 2:h + 1, 1]
        xp[:, :-1, h, w + 1] = xp[:, 1:, 1, 1]
    return xp


def _classes(transposed):
    return ((0, 0), (0, 1), (1, 0), (1, 1)) if transposed else ((0, 0),)


def _taps(w, transposed, ry, rx):
    """[Cout][Cin][k][k]: the taps one class convolves with (conv: the 3 x 3 kernel; deconv,
    class (ry, rx): g[i][j] = W[ci][co][3 - 2i - ry][3 - 2j - rx])."""
    if not transposed:
        return w
    return w[:, :, [3 - ry, 1 - ry]][:, :, :, [3 - rx, 1 - rx]].transpose(1, 0, 2, 3)


def _scatter(out, y, transposed, ry, rx, ty, tx):
    """Tile outputs y [2][2][Cout][N * ty * tx] of one class into out [N][Cout][.][.] (cropped to it)."""
    co, n = y.shape[2], out.shape[0]
    full = y.reshape(2, 2, co, n, ty, tx).transpose(3, 2, 4, 0, 5, 1).reshape(n, co, 2 * ty, 2 * tx)
    if transposed:
        h, w = out.shape[2] // 2, out.shape[3] // 2
        out[:, :, ry::2, rx::2] = full[:, :, :h, :w]
    else:
        out[...] = full[:, :, :out.shape[2], :out.shape[3]]


def winograd(x, w, absolute=False):
    """The kernels' algorithm in float64 without bias: F(2x2, 3x3) for w [Cout, Cin, 3, 3],
    F(2x2, 2x2) per output parity for w [Cin, Cout, 4, 4].  absolute: Babs, every matrix
    and operand replaced by its absolute value."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    transposed = w.shape[2] == 4
    bt, g, at = (DECONV_BT, DECONV_G, DECONV_AT) if transposed else (CONV_BT, CONV_G, CONV_AT)
    k = bt.shape[0]
    n, c, h, wd = x.shape
    cout = w.shape[1] if transposed else w.shape[0]
    ty, tx = (h + 1) // 2, (wd + 1) // 2
    xp = _padded(x, ty, tx)
    out = np.zeros((n, cout, 2 * h, 2 * wd) if transposed else (n, cout, h, wd))
    if absolute:
        xp, bt, at = np.abs(xp), np.abs(bt), np.abs(at)
    for ry, rx in _classes(transposed):
        u = np.einsum("ai,ocij,bj->aboc", g, _taps(w, transposed, ry, rx), g)
        d = _patches(xp, k, ty, tx, ry, rx)  # [k][k][C][N * tiles]
        # A^T [ sum_c U_c . (B^T d_c B) ] A as one GEMM over (r, s, c): both transforms are linear,
        # so they are applied to U (every factor already made absolute for Babs) --
        # y[i][j] = sum_rsc ( sum_ab At[i][a] At[j][b] U[a][b][o][c] Bt[a][r] Bt[b][s] ) d[r][s][c]
        au = np.einsum("ia,jb,aboc,ar,bs->ijorsc", at, at, np.abs(u) if absolute else u, bt, bt, optimize=True)
        y = np.matmul(au.reshape(4 * cout, k * k * c), d.reshape(k * k * c, -1))
        _scatter(out, y.reshape(2, 2, cout, -1), transposed, ry, rx, ty, tx)
    return out


def tolerance(x, conv, bn, res_pre=None, res_post=None):
    """The elementwise bound of the module docstring, float64, shaped as the output."""
    p = params(conv, bn)
    scale, shift = bn_fold(p)
    cpi = rup(x.shape[1], 16)
    t = np.abs(scale)[None, :, None, None] * winograd(x, p["w"], absolute=True) + np.abs(shift)[None, :, None, None]
    for r in (res_pre, res_post):
        if r is not None:
            t = t + np.abs(r.astype(np.float64))
    return (cpi + 16) * U * t


def close_ratio(got, ref):
    """tests/test_cnn.py's criterion as a ratio: max error over REL of the output scale."""
    scale = max(float(np.abs(ref).max()), 1e-6)
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / scale / REL


# ---- fp32 emulation of the kernels ----------------------------------------------------------
def emulate(x, conv, bn, relu=True, res_pre=None, res_post=None, fault=None):
    """The kernels' operation sequence with a float32 rounding after every operation;
    float32 [N, Cout, Ho, Wo].  fault: None or one of FAULTS, planted in image 0."""
    assert fault is None or fault in FAULTS, fault
    f32 = np.float32
    p = params(conv, bn)
    w = p["w"]
    transposed = p["transposed"]
    g = DECONV_G if transposed else CONV_G
    x = np.asarray(x, f32)
    n, c, h, wd = x.shape
    cout = w.shape[1] if transposed else w.shape[0]
    ty, tx = (h + 1) // 2, max((wd + 1) // 2, 2)  # (>= 2 tile columns, as every block has: "swap" needs two)
    xp = _padded(x, ty, tx, wrap=fault == "wrap")
    acc = np.zeros((n, cout, 2 * h, 2 * wd) if transposed else (n, cout, h, wd), f32)
    for ry, rx in _classes(transposed):
        u = np.einsum("ai,ocij,bj->abco", g, _taps(w.astype(np.float64), transposed, ry, rx), g).astype(f32)
        d = _patches(xp, 3 if transposed else 4, ty, tx, ry, rx)  # [k][k][C][N * tiles], image 0 first
        if transposed:  # e = Bt d, v = e B (deconv_wino_kernel's input transform)
            e = [d[0] - d[1], d[1], d[2] - d[1]]
            v = np.stack([np.stack([er[0] - er[1], er[1], er[2] - er[1]]) for er in e])
        else:           # (conv_wino_kernel's)
            e = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]
            v = np.stack([np.stack([er[0] - er[2], er[1] + er[2], er[2] - er[1], er[1] - er[3]]) for er in e])
        assert v.dtype == f32
        if fault == "drop" and (ry, rx) == (0, 0):  # the position that holds input pixel (0, 0) of tile 0
            v[1, 1, c // 2, 0] = 0
        if fault == "swap":  # tiles 0 and 1
            v[:, :, :, [0, 1]] = v[:, :, :, [1, 0]]
        m = np.zeros(v.shape[:2] + (cout, v.shape[3]), f32)  # [k][k][Cout][N * tiles]
        for ci in range(c):
            m = m + u[:, :, ci, :, None] * v[:, :, ci, None, :]
        assert m.dtype == f32
        if transposed:  # f = At m, y = f A
            f = [m[0] + m[1], m[1] + m[2]]
            y = np.stack([np.stack([fr[0] + fr[1], fr[1] + fr[2]]) for fr in f])
        else:
            f = [(m[0] + m[1]) + m[2], (m[1] - m[2]) - m[3]]
            y = np.stack([np.stack([(fr[0] + fr[1]) + fr[2], (fr[1] - fr[2]) - fr[3]]) for fr in f])
        _scatter(acc, y, transposed, ry, rx, ty, tx)
    scale, shift = bn_fold(p, f32)
    out = epilogue(acc, scale, shift, relu, None if res_pre is None else np.asarray(res_pre, f32),
                   None if res_post is None else np.asarray(res_post, f32))
    assert out.dtype == f32
    return out
