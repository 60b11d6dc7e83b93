"""float64 references and error bounds for the JLN post-processing kernels
(fvp_soft_argmax, fvp_fuse_poses; include/fvp.h), and the inputs the edge tests
(tests/test_gpu_jln_edges.py, tests/test_jln_ref.py) run them on.

Soft-argmax allowance.  Per row and coordinate, with u = 2^-24, y = beta * x,
m = max y, p the softmax, g the grid coordinate, c = sum p g, o the offset:

    delta = u * (2 max|y| + |m| + 4)       rounding of beta * x, of y - m, and expf (2 ulp)
    n     = ceil(S2 / 256) + 10            terms one thread sums + the reduction tree + the division
    D     = sum p |g - c|,  A = sum p |g|
    bound = 2 * (2 delta D + 2 n u (A + |c|) + 2 u |c + o|)

a worst-case first-order bound on the kernel's fp32 arithmetic (perturbed softmax
weights; fp32 accumulation of numerator and denominator; the division and the
offset add) with a factor 2 for the second-order terms.  maxprob = 1 / sum e is
allowed a relative (n + 4) u + delta.
"""
import math

import numpy as np

from oracle import fvp_oracle as O

U = 2.0 ** -24
BETA = 100.0

# row lengths: one cell; shorter than a thread's four; shorter than one 1024-cell pass; the ends
# of a pass; two passes with and without S2 % 4 == 0; the 4-pass kernel's last length and the
# 8-pass kernel's first (4096 | 4097); 80 x 80 planes; the 8-pass kernel's last length and the
# two-pass streaming kernel's first (8192 | 8193); 96 x 96 planes
S2_LIST = (1, 3, 81, 1023, 1024, 1028, 4096, 4097, 4100, 6400, 8192, 8193, 9216)
# (S2, P, J): the list at P = 2, J = 4, and one launch with P != J for (row / J) % P
CASES = tuple((s2, 2, 4) for s2 in S2_LIST) + ((4097, 3, 5),)
CONSTANT_S2 = (3, 81, 4096, 6400, 9216)
_FIXED_PEAKS = (0, 1, 3, 4, 1019, 1020, 1023, 1024, 4092, 4095, 4096, 4099, 8188, 8191, 8192, 8195)


def peak_cells(S2):
    """The flat indices the rows' peaks cycle through: the ends of a thread's four cells, of a
    256-thread pass, of each kernel's range and of the row itself."""
    cand = _FIXED_PEAKS + (S2 - 1, S2 - 2, S2 - 4, S2 - 5, S2 // 2)
    out = []
    for c in cand:
        if 0 <= c < S2 and c not in out:
            out.append(c)
    return out


def make_case(S2, P=2, J=4, seed=0):
    """features [3, P, J, S2, 1] fp32 (N(0, 0.02) noise, one single-cell peak of 0.15 per row at
    peak [3, P, J]), center_grid [3, S2, 2] fp32 uniform(-1500, 1800) per cell, offset [P, 3]
    fp32 uniform(+-3000)."""
    rng = np.random.default_rng(1000 * seed + S2 + 17 * P + J)
    feat = rng.normal(0.0, 0.02, (3, P, J, S2)).astype(np.float32)
    cells = peak_cells(S2)
    peak = np.array([cells[r % len(cells)] for r in range(3 * P * J)]).reshape(3, P, J)
    np.put_along_axis(feat, peak[..., None], np.float32(0.15), axis=3)
    grid = rng.uniform(-1500.0, 1800.0, (3, S2, 2)).astype(np.float32)
    offset = rng.uniform(-3000.0, 3000.0, (P, 3)).astype(np.float32)
    return dict(features=feat.reshape(3, P, J, S2, 1), center_grid=grid, offset=offset, peak=peak, S2=S2, P=P, J=J)


def constant_case(S2, P=2, J=4, value=0.37):
    c = make_case(S2, P, J, seed=1)
    c["features"] = np.full((3, P, J, S2, 1), value, np.float32)
    return c


def soft_argmax_ref(features, center_grid, offset, beta=BETA, drop=None):
    """float64 soft-argmax of fp32 inputs: dict(pose [3,P,J,2] (offset added where given), coords
    (without it), maxprob [3,P,J], D, A [3,P,J,2], bound [3,P,J,2] (absolute, of pose),
    maxprob_rel [3,P,J]).  drop [3,P,J,S2] bool removes cells from their rows (they get no
    weight).  A row holding a NaN or +inf, or nothing but -inf, comes out NaN as in torch."""
    P, J = features.shape[1], features.shape[2]
    x = features.reshape(3, P, J, -1).astype(np.float64)
    S2 = x.shape[3]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        y = np.float64(np.float32(beta)) * x
        m = y.max(axis=3, keepdims=True)
        e = np.exp(y - m)
        if drop is not None:
            e = np.where(drop, 0.0, e)
        se = e.sum(axis=3, keepdims=True)
        p = (e / se)[..., None]
        g = center_grid.reshape(3, 1, 1, S2, 2).astype(np.float64)
        coords = (p * g).sum(axis=3)
        D = (p * np.abs(g - coords[:, :, :, None, :])).sum(axis=3)
        A = (p * np.abs(g)).sum(axis=3)
        pose = coords if offset is None else O.add_offsets(coords, offset)
        delta = U * (2.0 * np.abs(y).max(axis=3) + np.abs(m[..., 0]) + 4.0)
        n = math.ceil(S2 / 256) + 10
        bound = 2.0 * (2.0 * delta[..., None] * D + 2.0 * n * U * (A + np.abs(coords)) + 2.0 * U * np.abs(pose))
        return dict(pose=pose, coords=coords, maxprob=1.0 / se[..., 0], D=D, A=A, bound=bound,
                    maxprob_rel=(n + 4) * U + delta)


def ratios(pose, maxprob, ref):
    """(largest |pose - ref| / bound, largest relative maxprob error / its allowance) over the
    rows whose reference is finite."""
    ok = np.isfinite(ref["maxprob"])
    pr = np.abs(np.asarray(pose, np.float64) - ref["pose"])[ok] / ref["bound"][ok]
    mr = (np.abs(np.asarray(maxprob, np.float64) - ref["maxprob"])[ok] / ref["maxprob"][ok]) / ref["maxprob_rel"][ok]
    return float(pr.max()), float(mr.max())


def torch_f32_soft_argmax(features, center_grid, offset, beta=BETA):
    """The reference layer's own arithmetic in fp32 on the CPU (softmax, weighted sum, offset)."""
    import torch

    P, J = features.shape[1], features.shape[2]
    x = torch.from_numpy(np.ascontiguousarray(features)).reshape(3, P, J, -1)
    p = torch.softmax(beta * x, dim=3)
    g = torch.from_numpy(np.ascontiguousarray(center_grid)).reshape(3, 1, 1, -1, 2)
    pose = (p[..., None] * g).sum(dim=3)
    if offset is not None:
        o = torch.from_numpy(np.ascontiguousarray(offset)).reshape(1, P, 1, 3)
        pose = pose + torch.cat([o[..., [0, 1]], o[..., [0, 2]], o[..., [1, 2]]], dim=0)
    return pose.numpy(), p.max(dim=3).values.numpy()


# -- fusion ----------------------------------------------------------------------------
def fuse_ref(pose, weights, maxprob):
    """float64 fuse_pose_preds of fp32 inputs: (fused [P,J,3], its allowance 8 u max(|a|, |b|)
    of each output's two contributing coordinates, confs [P], their relative allowance)."""
    pose64 = pose.astype(np.float64)
    J = pose.shape[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        fused = O.fuse_pose_preds(pose64, weights)
    a = np.abs(pose64)
    pair = np.stack([np.maximum(a[0, :, :, 0], a[1, :, :, 0]), np.maximum(a[0, :, :, 1], a[2, :, :, 0]),
                     np.maximum(a[1, :, :, 1], a[2, :, :, 1])], axis=2)
    confs = maxprob.astype(np.float64).mean(axis=(0, 2))
    return fused, 8.0 * U * pair, confs, (3 * J + 2) * U
