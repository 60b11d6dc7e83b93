"""The case table of the max-pool, layout and copy kernels (tests/test_pool_ref.py pins it on the
CPU, tests/test_gpu_pools.py runs it on the GPU); the references are in tests/pool_ref.py.

Shapes are the smallest that reach each edge; every case is a few kilobytes except the two at the
grid boundary (3 MB of input).  Which case reaches which kernel:

  fvp_maxpool_nhwc       maxpool_kernel<2,2> <1,2> <2,1> <1,1>: unpadded() with bf16 = False, one
                         set of shapes per (KH, KW); fvp_maxpool2_nhwc is the <2,2> cases again
  fvp_maxpool_nhwc_bf16  maxpool_bf16_kernel<2,2> <1,2> <2,1> <1,1>: unpadded() with bf16 = True
  fvp_maxpool_pad_nhwc   maxpool3s2_kernel: every fp32 (3, 2, 1) case of padded() but the last one
                         (rows of more than one block: W 21, C 100; gridDim.y at its limit:
                         N = 65535 images of one output row); maxpool_pad_kernel: every other fp32
                         geometry, and (3, 2, 1) at N = 65536, one row past the grid limit
  fvp_maxpool_pad_nhwc_bf16  maxpool_pad_bf16_kernel: padded() with bf16 = True
  fvp_nchw_to_nhwc       heatmaps_to_cl_kernel<1|2|4|8> at Cp 4, 8, 16, 32; nchw_to_nhwc_kernel at
                         Cp 12, 20, 48 and 6
  fvp_nhwc_to_nchw       nhwc_to_nchw_tiled_kernel at Cp % 4 == 0 and C <= 128 ((1,16), (15,16),
                         (128,128), (70,80); c0 = 4 of FROM); nhwc_to_nchw_kernel at C = 129, at
                         Cp = 6 and at c0 = 1 (a pointer 4 B off)
  fvp_copy_f4            copy_f4_kernel at 1, 255, 256 and 257 float4; 0 bytes launches nothing

Not in the table: the fast pool's guard at H*W*C/4 >= 2^31 (a 32-GiB input), grids beyond 2^31
blocks, and planar_to_cl_half_kernel (tests/test_gpu_cl_half.py holds it to bits).

Inputs (data()): bf16-exact values, in most cases all negative, so that a border cell padded with 0
instead of -inf differs from the reference; then a sprinkle of +0, -0, +inf, -inf and NaN; then, in
the window of the first output cell, channel 0 holds +0 at the first tap and -0 at the last over
negative values, channel 1 the same with the zeros exchanged, channel 2 a NaN at the first tap,
channel 3 a NaN at the last; and the rows and columns that floor mode drops hold +inf (even
channels) and NaN (odd channels), which may not reach the output.
"""
import zlib
from collections import namedtuple

import numpy as np

import pool_ref as R

# k, s, p: (rows, columns) pairs as tests/pool_ref.pool takes them; pad: the padded entry points
Pool = namedtuple("Pool", "pad bf16 N H W C k s p")

KHKW = ((2, 2), (1, 2), (2, 1), (1, 1))
KSP = ((3, 2, 1), (3, 1, 1), (2, 2, 0), (2, 2, 1), (1, 1, 0), (1, 2, 0), (2, 3, 1), (3, 3, 0), (4, 4, 2), (5, 2, 2))
SIZES = ((1, 1), (2, 2), (4, 6), (5, 7), (8, 3))
GRID_Y = 65535  # the fast (3, 2, 1) kernel has one blockIdx.y per (image, output row)


def _c(bf16, big):
    return ((4, 20), (8, 24))[bf16][big]


def unpadded(bf16):
    out = []
    for i, (kh, kw) in enumerate(KHKW):
        shapes = [(1, kh, kw), (3, 5, 7), (2, 6, 4)] + ([(2, 1, 9)] if kh == 1 else [])
        for j, (n, h, w) in enumerate(shapes):
            out.append(Pool(False, bf16, n, h, w, _c(bf16, (i + j) & 1), (kh, kw), (kh, kw), (0, 0)))
        # more than 256 threads and no multiple of 256, at every window (300 at the fewest)
        out.append(Pool(False, bf16, 5, 9, 11, _c(bf16, 1), (kh, kw), (kh, kw), (0, 0)))
    return out


def padded(bf16):
    out, i = [], 0
    for k, s, p in KSP:
        for h, w in SIZES:
            if h + 2 * p >= k and w + 2 * p >= k:
                out.append(Pool(True, bf16, (1, 3)[i & 1], h, w, _c(bf16, (i >> 1) & 1), (k, k), (s, s), (p, p)))
                i += 1
    if not bf16:
        g = ((3, 3), (2, 2), (1, 1))
        out += [Pool(True, False, 2, 5, 21, 100, *g),          # 11 columns x 25 quads: 275 threads a row
                Pool(True, False, GRID_Y, 1, 3, 4, *g),        # the last grid the fast kernel takes
                Pool(True, False, GRID_Y + 1, 1, 3, 4, *g)]    # the generic kernel
    return out


def pools():
    return unpadded(False) + unpadded(True) + padded(False) + padded(True)


def pool_id(c):
    return (f"{'pad' if c.pad else 'pool'}-{'bf16' if c.bf16 else 'f32'}-{c.N}x{c.H}x{c.W}x{c.C}-"
            f"k{c.k[0]}{c.k[1]}s{c.s[0]}{c.s[1]}p{c.p[0]}{c.p[1]}")


def out_hw(c):
    return R.out_size(c.H, c.k[0], c.s[0], c.p[0]), R.out_size(c.W, c.k[1], c.s[1], c.p[1])


def threads(c):
    ho, wo = out_hw(c)
    return c.N * ho * wo * c.C // (8 if c.bf16 else 4)


def fast(c):
    """fvp_maxpool_pad_nhwc takes maxpool3s2_kernel."""
    return c.pad and not c.bf16 and (c.k[0], c.s[0], c.p[0]) == (3, 2, 1) and c.N * out_hw(c)[0] <= GRID_Y


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def first_window(c):
    """The (row, column) taps inside the image of output cell (0, 0), in scan order."""
    return [(ky - c.p[0], kx - c.p[1]) for ky in range(c.k[0]) for kx in range(c.k[1])
            if 0 <= ky - c.p[0] < c.H and 0 <= kx - c.p[1] < c.W]


def dropped(c):
    """(first dropped row, first dropped column): what lies at or past them is in no window."""
    ho, wo = out_hw(c)
    return (ho - 1) * c.s[0] - c.p[0] + c.k[0], (wo - 1) * c.s[1] - c.p[1] + c.k[1]


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)


def data(c):
    """float32 [N][H][W][C], every value exact in bf16."""
    rng = np.random.default_rng(_seed("pool", *c))
    x = rng.uniform(-4.0, -0.5, (c.N, c.H, c.W, c.C)).astype(np.float32)
    if _seed("sign", *c) % 4 == 0:  # one case in four has both signs
        x *= rng.choice(np.float32([-1.0, 1.0]), x.shape)
    x = R.to_bf16_exact(x)
    hit = rng.random(x.shape) < 0.06
    x[hit] = SPECIALS[rng.integers(0, len(SPECIALS), int(hit.sum()))]
    taps = first_window(c)
    if len(taps) >= 2:
        (y0, x0), (y1, x1) = taps[0], taps[-1]
        for ch in (0, 1):
            for ty, tx in taps:
                x[:, ty, tx, ch] = -1.0 - 0.25 * ch
        x[:, y0, x0, 0], x[:, y1, x1, 0] = 0.0, -0.0
        x[:, y0, x0, 1], x[:, y1, x1, 1] = -0.0, 0.0
        for ty, tx in taps:
            x[:, ty, tx, 2:4] = -2.0
        x[:, y0, x0, 2] = np.nan
        x[:, y1, x1, 3] = np.nan
    dy, dx = dropped(c)
    for ch, v in ((slice(0, None, 2), np.inf), (slice(1, None, 2), np.nan)):
        x[:, max(dy, 0):, :, ch] = v
        x[:, :, max(dx, 0):, ch] = v
    return x


# ---- layouts ----------------------------------------------------------------------------
ToNhwc = namedtuple("ToNhwc", "N C H W Cp")
ToNchw = namedtuple("ToNchw", "N C H W Cp")
From = namedtuple("From", "N C H W Cp c0")  # fvp.cnn.to_nchw_from: C channels from c0 of a Cp pitch

HW = {1: (1, 1), 15: (3, 5), 63: (7, 9), 64: (8, 8), 65: (5, 13), 129: (3, 43)}
TO_NHWC_CCP = ((1, 4), (4, 4), (5, 8), (15, 16), (16, 16), (17, 32), (32, 32), (3, 12), (20, 20), (33, 48), (5, 6))
TO_NCHW_CCP = ((1, 16), (15, 16), (128, 128), (129, 132), (5, 6), (70, 80))
FROM = (From(2, 7, 5, 13, 16, 1), From(2, 12, 5, 13, 16, 4))


def to_nhwc_cases():
    return [ToNhwc((1, 3)[(i + j) & 1], c, *HW[hw], cp) for i, (c, cp) in enumerate(TO_NHWC_CCP)
            for j, hw in enumerate((1, 15, 64, 65))]


def to_nchw_cases():
    return [ToNchw((1, 3)[(i + j) & 1], c, *HW[hw], cp) for i, (c, cp) in enumerate(TO_NCHW_CCP)
            for j, hw in enumerate((1, 63, 64, 65, 129))]


PREFILL_BITS = int(np.float32(R.PREFILL).view(np.int32))


def bits(shape, *key):
    """Random 32-bit patterns (NaN payloads, denormals and both zeros among them), none the prefill."""
    x = np.random.default_rng(_seed("bits", *key)).integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)
    x[x == PREFILL_BITS] = 1
    return x


COPY_BYTES = (0, 16, 16 * 255, 16 * 256, 16 * 257)
