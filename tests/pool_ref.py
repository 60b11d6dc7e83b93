"""Plain references of the memory-movement kernels of the CNNs (csrc/fvp_conv.hip, csrc/fvp_copy.hip):
the max pools, the NCHW <-> NHWC layout passes and the float4 copy.  Their results are exact, so
every comparison against these is bit equality (NaN by position in the pools).

One pool function serves both families: fvp_maxpool_pad_nhwc(K, S, P) directly, fvp_maxpool_nhwc as
K = (KH, KW), S = K, P = 0.  The rule, per output element: the running value starts at -inf; the taps
of the window run in row-major order, taps outside the image are skipped (the same as -inf padding);
a tap b replaces the running value m when `b > m or b != b`.  So the result is the first tap in scan
order that attains the maximum, -0 and +0 count as equal (the earlier one stays), and once a NaN is
met it stays.  bf16 is the same rule on bf16 values held as float32.  Output sizes are floor mode.
tests/test_pool_ref.py pins this to torch's CPU max_pool2d bit for bit on every case of
tests/pool_cases.py.

`fault` plants one wrong variant of the rule (FAULTS); the layout and copy references take theirs
(LAYOUT_FAULTS) the same way.  They exist for tests/test_pool_ref.py, which proves that the case table
tells each of them from the reference.
"""
import numpy as np

FAULTS = ("zero_pad", "start0", "ceil", "drop_row", "drop_col", "origin_y", "origin_x", "s_for_k", "ge", "fmax",
          "nan_first", "image", "swap", "xy")
LAYOUT_FAULTS = ("pitch", "pad", "tail")
PREFILL = 12288.0  # what the tests put where a result belongs: exact in bf16, and no input holds it


def out_size(n, k, s, p, ceil=False):
    """Floor mode: (n + 2p - k) // s + 1.  ceil (a planted fault): torch's ceil_mode size."""
    if not ceil:
        return (n + 2 * p - k) // s + 1
    o = -(-(n + 2 * p - k) // s) + 1
    return o - 1 if (o - 1) * s >= n + p else o


def pool(x, k, s, p, group=4, fault=None):
    """x: float32 [N][H][W][C]; k, s, p: (rows, columns) pairs -> float32 [N][Ho][Wo][C].
    group: the channels a thread owns (4 for fp32, 8 for bf16): only the `swap` fault reads it."""
    x = np.ascontiguousarray(x, np.float32)
    N, H, W, C = x.shape
    (kh, kw), (sh, sw), (ph, pw) = k, s, p
    Ho, Wo = out_size(H, kh, sh, ph, fault == "ceil"), out_size(W, kw, sw, pw, fault == "ceil")
    flat = x.reshape(N, H * W, C)
    if fault == "image":  # the image stride lost: every image reads the first
        flat = np.broadcast_to(flat[:1], flat.shape)
    out = np.empty((N, Ho, Wo, C), np.float32)
    wh, ww = (sh, sw) if fault == "s_for_k" else (kh, kw)
    for y in range(Ho):
        # the rows / columns floor mode drops, taken into the last window
        nky = wh + ((H + 2 * ph - kh) % sh if fault == "drop_row" and y == Ho - 1 else 0)
        for xo in range(Wo):
            nkx = ww + ((W + 2 * pw - kw) % sw if fault == "drop_col" and xo == Wo - 1 else 0)
            m = np.full((N, C), 0.0 if fault == "start0" else -np.inf, np.float32)
            tap = 0
            for ky in range(nky):
                iy = y * sh - ph + ky + (fault == "origin_y")
                for kx in range(nkx):
                    ix = xo * sw - pw + kx + (fault == "origin_x")
                    if 0 <= iy < H and 0 <= ix < W:
                        b = flat[:, ix * H + iy if fault == "xy" else iy * W + ix]
                    elif fault == "zero_pad":
                        b = np.zeros((N, C), np.float32)
                    else:
                        continue
                    with np.errstate(invalid="ignore"):
                        if fault == "ge":
                            take = (b >= m) | (b != b)
                        elif fault == "fmax":
                            take = b > m
                        elif fault == "nan_first":
                            take = (b > m) | ((b != b) & (tap == 0))
                        else:
                            take = (b > m) | (b != b)
                    m = np.where(take, b, m)
                    tap += 1
            out[:, y, xo] = m
    if fault == "swap":  # neighbouring channel groups written to each other's place
        g = C // group
        for a in range(0, g - 1, 2):
            lo = out[..., a * group:(a + 1) * group].copy()
            out[..., a * group:(a + 1) * group] = out[..., (a + 1) * group:(a + 2) * group]
            out[..., (a + 1) * group:(a + 2) * group] = lo
    return out


def same(a, b):
    """The pool criterion: equal shapes, NaN at the same positions, every other element equal as int32."""
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))


def to_bf16_exact(x):
    """float32 values truncated to the nearest-toward-zero bf16 value (NaN and inf stay what they are)."""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


# ---- layouts and the copy: int32 bit patterns ---------------------------------------------
def _drop_tail(out, ref, unit):
    """The `tail` fault: what the last, partial group of `unit` flat elements would write is missing."""
    full = ref.size // unit * unit
    out.reshape(-1)[:full] = ref.reshape(-1)[:full]
    return out


def nchw_to_nhwc(x, cp, prefill, fault=None):
    """x: int32 [N][C][H][W] -> int32 [N][H][W][cp], channels C .. cp-1 zero (+0)."""
    N, C, H, W = x.shape
    ref = np.zeros((N, H, W, cp), np.int32)
    ref[..., :C] = x.transpose(0, 2, 3, 1)
    if fault is None:
        return ref
    out = np.full((N, H, W, cp), prefill, np.int32)
    if fault == "pad":
        out[..., :C] = ref[..., :C]
    elif fault == "pitch":  # pixels C apart instead of cp
        out.reshape(-1)[:N * H * W * C] = x.transpose(0, 2, 3, 1).reshape(-1)
    elif fault == "tail":
        _drop_tail(out, ref, 256)
    return out


def nhwc_to_nchw(x, c, prefill, fault=None):
    """x: int32 [N][H][W][cp] -> int32 [N][c][H][W], channels 0 .. c-1 of every pixel."""
    N, H, W, cp = x.shape
    ref = np.ascontiguousarray(x[..., :c].transpose(0, 3, 1, 2))
    if fault is None:
        return ref
    if fault == "pitch":  # pixels read c apart instead of cp
        return np.ascontiguousarray(x.reshape(-1)[:N * H * W * c].reshape(N, H, W, c).transpose(0, 3, 1, 2))
    out = np.full((N, c, H * W), prefill, np.int32)
    full = H * W // 64 * 64  # `tail`: the pixels past the last whole 64-pixel tile of an image
    out[..., :full] = ref.reshape(N, c, H * W)[..., :full]
    return out.reshape(N, c, H, W)


def copy_f4(x, prefill, fault=None):
    """x: int32 [bytes / 4] -> the same.  `tail`: the last partial block of 256 float4 is missing."""
    if fault is None:
        return x.copy()
    return _drop_tail(np.full(x.shape, prefill, np.int32), x, 1024)
