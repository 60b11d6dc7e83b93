"""Heatmap sizes and image borders: the reference side (plain numpy, no GPU).

* tap_classes: where the oracle's bilinear taps fall, 5 classes per axis, from
  the oracle's own fp32 arithmetic (oracle.fvp_oracle.grid_sample:
  ix = (g + 1) * fp32((W - 1) / 2), x0 = floor(ix)).
* planted_grid: a sample grid whose first slots of every camera hit every
  reachable (x class, y class) pair, each coordinate found by search under that
  rounding.
* pair_table / cl_table: the workspace tables the layout passes of
  faster-voxelpose_amd/csrc/fvp_layout.h write, bit for bit, and their decoders.
* pair_layout_model: the three-way choice of fvp::pair_layout_kind.
"""
import functools

import numpy as np

F32 = np.float32

# -- tap classes ------------------------------------------------------------------
# by the top-left tap t = floor(ix) of an axis of n pixels
BELOW, MINUS1, INSIDE, LAST, BEYOND = range(5)   # t < -1 | t == -1 | 0 <= t <= n - 2 | t == n - 1 | t > n - 1
CLASS_NAMES = ("below", "minus1", "inside", "last", "beyond")


def sample_px(g, n):
    """The oracle's unnormalised coordinate (fvp_oracle.grid_sample): (g + 1) * fp32((n - 1) / 2), fp32."""
    return ((np.asarray(g, F32) + F32(1)) * F32((n - 1) / 2)).astype(F32)


def axis_class(g, n):
    t = np.floor(sample_px(g, n))
    return np.where(t < -1, BELOW, np.where(t == -1, MINUS1, np.where(t <= n - 2, INSIDE,
                                                                     np.where(t == n - 1, LAST, BEYOND)))).astype(np.int64)


def tap_classes(sg, W, H):
    """[V, 5, 5] counts of a sample grid [V, N, 2]: [v, x class, y class]."""
    sg = np.asarray(sg, F32)
    cx, cy = axis_class(sg[..., 0], W), axis_class(sg[..., 1], H)
    out = np.zeros((sg.shape[0], 5, 5), np.int64)
    for v in range(sg.shape[0]):
        np.add.at(out[v], (cx[v], cy[v]), 1)
    return out


def _class_range(cls, n):
    """Integer taps t of a class that a coordinate in [-2, 2] can reach: ix lies in [-(n-1)/2, 3(n-1)/2]."""
    lo, hi = int(np.floor(-(n - 1) / 2)), int(np.floor(3 * (n - 1) / 2))
    want = {BELOW: range(lo, -1), MINUS1: (-1,), INSIDE: range(0, n - 1), LAST: (n - 1,),
            BEYOND: range(n, hi + 1)}[cls]
    return [t for t in want if lo <= t <= hi]


def _search(t, frac, n):
    """An fp32 g in [-2, 2] with floor(sample_px(g, n)) == t and a fractional part as close to `frac` as fp32
    allows (frac == 1: the largest below 1), or None: a walk over neighbouring fp32 values from the float64 solution."""
    s = np.float64(F32((n - 1) / 2))
    target = t + min(frac, 1.0 - 2.0 ** -25)
    g = F32(target / s - 1.0)
    best = None
    for step in range(-6, 7):
        c = g
        for _ in range(abs(step)):
            c = np.nextafter(c, F32(np.inf if step > 0 else -np.inf))
        if abs(float(c)) > 2.0:
            continue
        ix = float(sample_px(c, n))
        if np.floor(ix) != t:
            continue
        err = abs(ix - target)
        if best is None or err < best[0]:
            best = (err, c)
    if best is None:
        return None
    g = F32(best[1])
    if frac >= 1.0:   # the last coordinate of the tap: several g round to the largest ix below t + 1
        for _ in range(64):
            up = np.nextafter(g, F32(np.inf))
            if float(up) > 2.0 or np.floor(float(sample_px(up, n))) != t:
                break
            g = up
    return g


FRACS = (0.0, 0.25, 0.5, 1.0)   # 1.0 stands for the largest fp32 below the next integer


@functools.lru_cache(None)
def axis_candidates(n):
    """{class: [g, ...]} of one axis: per class up to eight coordinates in [-2, 2] (the fractional parts FRACS at
    the class's taps nearest to the image, then the next ones), each verified to be of its class under the
    oracle's rounding.  A class missing from the dict cannot be reached within [-2, 2].  (Cached: read-only.)"""
    out = {}
    for cls in range(5):
        taps = _class_range(cls, n)
        if cls == BELOW:
            taps = taps[::-1]                       # nearest to the image first
        if cls == INSIDE and len(taps) > 2:
            taps = [taps[0], taps[-1], taps[len(taps) // 2]]
        got = []
        for t in taps[:3]:
            for f in FRACS:
                g = _search(t, f, n)
                if g is not None and int(axis_class(g, n)) == cls and not any(g == h for h in got):
                    got.append(g)
        if got:
            out[cls] = got[:8]
    return out


def unreachable(n):
    """Names of the tap classes of an axis of n pixels that no coordinate in [-2, 2] reaches."""
    return [CLASS_NAMES[c] for c in range(5) if c not in axis_candidates(n)]


# exact border coordinates: ix == 0 and ix == n - 1 (weight 0 on the missing tap), the clip values of
# project_grid, and the value fvp_pack_grid writes into padding slots
SPECIALS = ((-2.0, -2.0), (2.0, 2.0), (-1.0, -1.0), (1.0, 1.0), (-1.1, -1.1), (1.1, 1.1), (-1.0, 1.0), (1.0, -1.0),
            (-1.1, 1.1), (1.1, -1.1), (-1.0, 0.3), (0.3, 1.0), (2.0, -2.0), (-2.0, 2.0))
MIN_SPECIALS = 8
PER_PAIR = 4


def planted_points(W, H):
    """[M, 2] fp32: the first MIN_SPECIALS of SPECIALS, PER_PAIR points of every reachable (x class, y class)
    pair, then the other SPECIALS."""
    cx, cy = axis_candidates(W), axis_candidates(H)
    pts = [p for p in SPECIALS[:MIN_SPECIALS]]
    for a in sorted(cx):
        for b in sorted(cy):
            for i in range(PER_PAIR):
                # the fractional parts of the two axes run against each other: (0, .25), (.25, .5), ...
                pts.append((cx[a][i % len(cx[a])], cy[b][(i + 1 + a) % len(cy[b])]))
    pts += list(SPECIALS[MIN_SPECIALS:])
    return np.array(pts, F32)


def planted_grid(V, N, W, H, seed):
    """Sample grid [V, N, 2] fp32 within [-2, 2]: every camera's first slots are planted_points(W, H) (each camera
    starts at another point of the list, so a voxel's cameras differ; truncated to N after the class pairs), the
    rest uniform in [-1.1, 1.1]."""
    pts = planted_points(W, H)
    need = MIN_SPECIALS + PER_PAIR * len(axis_candidates(W)) * len(axis_candidates(H))
    assert N >= need, f"{N} voxels cannot hold the {need} planted samples of {W} x {H}"
    m = min(len(pts), N)
    rng = np.random.default_rng(seed)
    sg = rng.uniform(-1.1, 1.1, (V, N, 2)).astype(F32)
    for v in range(V):
        sg[v, :need] = np.roll(pts[:need], 7 * v, axis=0)
        sg[v, need:m] = pts[need:m]
    assert np.isfinite(sg).all() and np.abs(sg).max() <= 2.0
    return sg


# -- the layout choice ---------------------------------------------------------------
VEC8, ROWS, ENTRY = 0, 1, 2
LAYOUT_NAMES = ("vec8", "rows", "entry")


def pair_layout_model(nf, W, addr):
    """fvp_layout.h :246-250 pair_layout_kind: vec8 for W % 8 == 0 at a 16-B aligned address (:247); the row
    kernel for frame groups of even width at a 4-B aligned address whose staged rows, NF * 16 * (W / 2 + 2) * 4
    bytes (:244 pairs_rows_lds), fit 64 KiB (:248); the per-entry kernel otherwise."""
    if W % 8 == 0 and addr % 16 == 0:
        return VEC8
    if nf > 1 and addr % 4 == 0 and W % 2 == 0 and nf * 16 * (W // 2 + 2) * 4 <= 65536:
        return ROWS
    return ENTRY


# -- expected workspace tables ----------------------------------------------------------
def pair_table(hm, nf):
    """The fp16 pixel-pair table of heatmaps [nb, V, J, H, W] (uint16 bit patterns, J <= 16, nb % nf == 0) as
    uint16 [nb / nf, V, H, W + 1, nf, 4, 2, 4]: entry (y, e) of 64 B holds pixels e - 1 and e of row y, lane q's
    16 B = [pixel e - 1: joints 4q .. 4q + 3 | pixel e: joints 4q .. 4q + 3], zeros outside the image and for
    joints >= J; the nf frames of a group interleaved per entry (fvp_layout.h :80-82 the layout, :103-104 the
    two pixels `(j < J && e >= 1) ? src[j * HW + e - 1] : z` and `(j < J && e < W) ? src[j * HW + e] : z`, :108-109
    the halves' order, :115 the store `tab[(((((g * V + v) * H + y) * W1 + e) * NF) + f) * 4 + q]`)."""
    hm = np.asarray(hm)
    assert hm.dtype == np.uint16
    nb, V, J, H, W = hm.shape
    assert J <= 16 and nb % nf == 0
    pad = np.zeros((nb, V, 16, H, W + 2), np.uint16)
    pad[:, :, :J, :, 1:W + 1] = hm
    lo, hi = pad[..., 0:W + 1], pad[..., 1:W + 2]                       # pixels e - 1 and e, [nb, V, 16, H, W + 1]
    t = np.stack([lo, hi], axis=-1)                                     # [nb, V, 16, H, W + 1, 2]
    t = t.reshape(nb // nf, nf, V, 4, 4, H, W + 1, 2)                   # [g, f, V, q, k, H, e, half]
    return np.ascontiguousarray(t.transpose(0, 2, 5, 6, 1, 3, 7, 4))    # [g, V, H, e, f, q, half, k]


def pair_table_decode(tab, J):
    """The heatmaps [nb, V, J, H, W] a pair table holds, from the second pixel of entries 0 .. W - 1; the first
    pixels, entry W's second and the joints >= J are returned as a bool: all as pair_table writes them."""
    g, V, H, W1, nf, _, _, _ = tab.shape
    t = tab.transpose(0, 4, 1, 5, 7, 2, 3, 6).reshape(g * nf, V, 16, H, W1, 2)   # [nb, V, j, H, e, half]
    hm = t[:, :, :J, :, :W1 - 1, 1]
    ok = np.array_equal(t[:, :, :J, :, 1:, 0], hm) and not t[:, :, :, :, 0, 0].any() and \
        not t[:, :, :, :, W1 - 1, 1].any() and not t[:, :, J:].any()
    return hm, ok


def cl_table(hm, j0, J, lpv):
    """The fp32 channels-last table of joints j0 .. j0 + J - 1 of heatmaps [nb, V, Jst, H, W] (fp32 values; fp16
    sources widened exactly) as fp32 [nb, V, H * W, lpv, 4], joints >= J zero: heatmaps_to_cl_kernel with NF = 1
    (fvp_layout.h :63 the source plane `hm + bv * Jst * HW + pix`, :66-69 `o.x = (j + 0 < J) ? ... : 0.f` for
    joints 4q .. 4q + 3, :71 the store `cl[pxg * LPV + q] = o` of pixel pxg = (b V + v) H W + pix)."""
    hm = np.asarray(hm, F32)
    nb, V, Jst, H, W = hm.shape
    assert J <= 4 * lpv and j0 + J <= Jst
    t = np.zeros((nb, V, H * W, 4 * lpv), F32)
    t[..., :J] = hm[:, :, j0:j0 + J].reshape(nb, V, J, H * W).transpose(0, 1, 3, 2)
    return t.reshape(nb, V, H * W, lpv, 4)


def cl_table_decode(tab, J, H, W):
    nb, V, HW, lpv, _ = tab.shape
    t = tab.reshape(nb, V, HW, 4 * lpv)
    return t[..., :J].transpose(0, 1, 3, 2).reshape(nb, V, J, H, W), not t[..., J:].any()
