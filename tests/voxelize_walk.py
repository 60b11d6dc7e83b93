"""A numpy model of where every (block, pass, slot) of a voxelize gather launch
works and stores (voxelize_body and store_stage in csrc/fvp_voxelize.hip):
xcd_remap, the band walk, c0 / ncols, the layer-major slot order, the stage
index ii and the cube index gn, then the epilogue's cube runs and xy cells.

check(...) returns the list of broken properties (empty: the launch writes
every cube and xy element of a frame exactly once, from the stage slot that
holds that voxel, and reads the packed grid inside its bounds).  `fault` plants
one of FAULTS, so a test can show that a table of shapes would see it.
"""
import numpy as np

FAULTS = ("rows_band", "ncols_cols", "gpr_unsnapped", "zl_cl_swapped", "last_pass_unclipped", "n0_without_z")


def xcd_remap(bid, nblk):
    xcd, k = bid % 8, bid // 8
    q, r = nblk // 8, nblk % 8
    return xcd * q + np.minimum(xcd, r) + k


def check(X, Y, Z, lpv, cols, band, col_blocks, groups=1, unsnapped=None, fault=None):
    """groups: frame groups of the launch (blocks = groups * col_blocks)."""
    bad = []
    XY, N, vpp = X * Y, X * Y * Z, 256 // lpv
    nblk = groups * col_blocks
    L = xcd_remap(np.arange(nblk), nblk)
    if not np.array_equal(np.sort(L), np.arange(nblk)):
        bad.append("xcd_remap is not a permutation of the blocks")
    bl = L // col_blocks
    if np.bincount(bl, minlength=groups).tolist() != [col_blocks] * groups:
        bad.append("frame groups do not get col_blocks blocks each")
    cb = np.arange(col_blocks)          # (every group walks the same blocks: one group is enough below)
    if band > 0:
        gpr = Y // (unsnapped if fault == "gpr_unsnapped" else cols)
        per_band = band * max(gpr, 1)
        bi, r = cb // per_band, cb % per_band
        rows = np.full_like(cb, band) if fault == "rows_band" else np.minimum(band, X - bi * band)
        rows = np.maximum(rows, 1)
        gc, xr = r // rows, r % rows
        cb = (bi * band + xr) * gpr + gc
    c0 = cb * cols
    ncols = np.full_like(c0, cols) if fault == "ncols_cols" else np.minimum(cols, XY - c0)
    if (ncols <= 0).any() or (c0 < 0).any():
        return bad + ["a block starts outside the grid"]
    T = ncols * Z
    n0 = c0 if fault == "n0_without_z" else c0 * Z
    passes = -(-(cols * Z) // vpp)
    i = np.arange(passes * vpp)[None, :]                      # slot index over the passes
    live = i < (-(-T // vpp) * vpp)[:, None]                  # the block's own pass loop: i0 < T
    if fault == "last_pass_unclipped":
        valid, sl = live, i + 0 * T[:, None]
    else:
        valid, sl = live & (i < T[:, None]), np.minimum(i, T[:, None] - 1)
    nc = ncols[:, None]
    if fault == "zl_cl_swapped":
        cl = sl // nc
        zl = sl - cl * nc
    else:
        zl = sl // nc
        cl = sl - zl * nc
    ii = cl * Z + zl
    gn = (c0[:, None] + cl) * Z + zl
    # grid reads (every live slot loads, valid or not) stay inside the packed grid
    if (gn[live] < 0).any() or (gn[live] >= N).any():
        bad.append("a grid offset leaves the packed grid")
    # the stage: every slot 0..T-1 written exactly once, by the lane that computed voxel n0 + ii
    cnt = np.zeros((col_blocks, cols * Z + 1), np.int64)
    rows_ix = np.broadcast_to(np.arange(col_blocks)[:, None], ii.shape)
    np.add.at(cnt, (rows_ix[valid], np.minimum(ii[valid], cols * Z)), 1)
    want = (np.arange(cols * Z + 1)[None, :] < T[:, None]).astype(np.int64)
    if not np.array_equal(cnt, want):
        bad.append("a block's stage slots are not written exactly once")
    if not np.array_equal((gn - ii)[valid], np.broadcast_to((c0 * Z)[:, None], ii.shape)[valid]):
        bad.append("a stage slot holds another voxel than the one stored from it")
    # epilogue: cube runs [n0, n0 + T) from stage[0, T); xy cells c0 .. c0 + ncols from stage columns
    cube = np.zeros(N + 1, np.int64)
    e = np.arange(cols * Z)[None, :]
    em = e < T[:, None]
    dst = (n0[:, None] + e)[em]
    np.add.at(cube, np.clip(dst, 0, N), 1)
    if cube[N] or not (cube[:N] == 1).all():
        bad.append("the cube is not written exactly once")
    elif not np.array_equal(np.sort((c0[:, None] * Z + e)[em]), np.arange(N)):
        bad.append("the cube runs hold other voxels than their place")
    xy = np.zeros(XY + 1, np.int64)
    cc = np.arange(cols)[None, :]
    cm = cc < ncols[:, None]
    np.add.at(xy, np.clip((c0[:, None] + cc)[cm], 0, XY), 1)
    if xy[XY] or not (xy[:XY] == 1).all():
        bad.append("the xy plane is not written exactly once")
    return bad
