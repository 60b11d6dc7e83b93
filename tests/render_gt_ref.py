"""numpy restatement of fvp_project_poses / fvp_render_poses3d (include/fvp.h), for
the 'gt' render tests: the 'gt' branch of JointsDataset.__getitem__
(lib/dataset/JointsDataset.py:221-259) with project_point_cpu
(lib/utils/cameras.py:58-84) and affine_transform (lib/utils/transforms.py:53-56),
in float64, one rounded numpy operation per operator and an exact fused
multiply-add where numpy's matmul / dot use one.  The painting is
tests/render_ref.py.  Also the poses the tests project and the fixture loader."""
import functools
import os
from fractions import Fraction

import numpy as np

import render_ref as R

CAM_STRIDE = 24
IMAGE_SIZE = (192, 128)
SIGMA = 3.0
B, P = 2, 5
# calibration fixture, original image (W, H), capture space (size, centre): fvp.workloads
CALIBRATIONS = {
    "shelf": ("calibration_shelf.json", (1032, 776), (8000.0, 8000.0, 2000.0), (450.0, -320.0, 800.0)),
    "panoptic": ("calibration_panoptic_demo.json", (1920, 1080), (8000.0, 8000.0, 2000.0), (0.0, -500.0, 800.0)),
}
# (calibration, J, heatmap (W, H), zoom of the resize transform, seed): both calibrations, both
# channel paddings, the renderer's two tile-odd shapes; the last case zooms
CASES = [("shelf", 17, (48, 32), 1.0, 2), ("panoptic", 15, (50, 37), 1.0, 3), ("shelf", 15, (50, 37), 1.0, 1),
         ("panoptic", 17, (48, 32), 1.5, 11)]


def _fma_scalar(a, b, c):
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c  # a NaN or an infinity decides the result; there is nothing to round
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # exact, then one rounding to nearest even


_fma_ufunc = np.frompyfunc(_fma_scalar, 3, 1)


def fma(a, b, c):
    """fp64 fused multiply-add, exact: the product and the sum as fractions, one rounding."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(_fma_ufunc(a, b, c), dtype=np.float64)


def project(joints3d, vis3d, cam, resize_t, ori_image_size, image_size):
    """joints3d [..., 3], vis3d [...] or None, cam fp64 [CAM_STRIDE] -> (joints2d [..., 2] fp64, vis2d
    [...] bool, detail): the contract of fvp_project_poses for one camera.  `detail` holds the
    intermediate flags the coverage tests count."""
    X = np.asarray(joints3d, np.float64)
    Rm, T = cam[0:9].reshape(3, 3), cam[9:12]
    fx, fy, cx, cy = cam[12:16]
    k0, k1, k2, p0, p1 = cam[16:21]
    t = np.asarray(resize_t, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = X - T
        xc = [fma(Rm[r, 2], d[..., 2], fma(Rm[r, 1], d[..., 1], Rm[r, 0] * d[..., 0])) for r in range(3)]
        den = xc[2] + 1e-5
        y0, y1 = xc[0] / den, xc[1] / den
        r = y0 * y0 + y1 * y1
        dd = ((1 + k0 * r) + (k1 * r) * r) + ((k2 * r) * r) * r
        u = (y0 * dd + ((2 * p0) * y0) * y1) + p1 * (r + (2 * y0) * y0)
        w = (y1 * dd + ((2 * p1) * y0) * y1) + p0 * (r + (2 * y1) * y1)
        px, py = fx * u + cx, fy * w + cy
        seen3 = np.ones(px.shape, bool) if vis3d is None else np.asarray(vis3d) > 0
        first = (px >= 0) & (px <= ori_image_size[0] - 1) & (py >= 0) & (py <= ori_image_size[1] - 1)
        qx = fma(t[0, 0], px, t[0, 1] * py) + t[0, 2]
        qy = fma(t[1, 0], px, t[1, 1] * py) + t[1, 2]
        q = np.stack([qx, qy], axis=-1)
        neg = np.min(q, axis=-1) < 0  # (np.min hands a NaN on, and NaN < 0 is false)
        second = neg | (qx >= image_size[0]) | (qy >= image_size[1])
    detail = dict(px=px, py=py, behind=xc[2] < 0, seen3=seen3, first=first, neg=neg, right=qx >= image_size[0],
                  below=qy >= image_size[1])
    return q, seen3 & first & ~second, detail


def project_batch(joints3d, vis3d, count, cams, cam_index, resize_t, ori_image_size, image_size):
    """The batched call: joints3d [B, P, J, 3], vis3d [B, P, J] or None, count [B], cams [S, V, 24],
    cam_index [B] or None -> (joints2d [B, V, P, J, 2], vis2d [B, V, P, J] uint8), rows at or beyond
    count zero (as the kernels write them)."""
    Bn, Pn, J, _ = joints3d.shape
    V = cams.shape[1]
    j2 = np.zeros((Bn, V, Pn, J, 2), np.float64)
    v2 = np.zeros((Bn, V, Pn, J), np.uint8)
    for b in range(Bn):
        n = int(count[b])
        s = 0 if cam_index is None else int(cam_index[b])
        for v in range(V):
            q, vis, _ = project(joints3d[b, :n], None if vis3d is None else vis3d[b, :n], cams[s, v], resize_t,
                                ori_image_size, image_size)
            j2[b, v, :n], v2[b, v, :n] = q, vis
    return j2, v2


def render_batch(joints2d, vis2d, count, image_size, heatmap_size, sigma):
    """The painter on the projection's outputs: count [B] holds for every view -> [B, V, J, H, W] fp32."""
    V = joints2d.shape[1]
    return R.render(joints2d, np.repeat(np.asarray(count, np.int32)[:, None], V, axis=1), vis2d, image_size,
                    heatmap_size, sigma)


# -- calibrations, transforms and the poses the tests project ----------------------------------
@functools.lru_cache(maxsize=None)
def cameras64(name):
    """fp64 [V, CAM_STRIDE] records of a committed calibration (geometry.pack_cameras64)."""
    from fvp import geometry
    from fvp.workloads import load_calibration

    cams, seq = load_calibration(CALIBRATIONS[name][0])
    out = geometry.pack_cameras64(cams, seq)
    out.setflags(write=False)
    return out


def camera_dicts(name):
    from fvp.workloads import load_calibration

    cams, seq = load_calibration(CALIBRATIONS[name][0])
    return [cams[seq][c] for c in range(len(cams[seq]))]


def resize_transform(name, zoom=1.0, image_size=IMAGE_SIZE):
    """The dataset's 2x3 float64 resize transform (geometry.resize_transform).  zoom != 1: the same
    transform with its linear part scaled by `zoom` about the image centre, which the transform
    keeps mapping the original image's centre to -- get_affine_transform with scale / zoom.  (Scaling
    the 2x2 block alone leaves the letterbox translation >= 0, so no visible joint could reach a
    negative coordinate; about the centre, joints leave the resized image on every side.)"""
    from fvp import geometry

    ori = CALIBRATIONS[name][1]
    if zoom == 1.0:
        return geometry.resize_transform(ori, image_size)
    c = np.array([ori[0] / 2.0, ori[1] / 2.0])
    return geometry.get_affine_transform(c, geometry.get_scale(ori, image_size) / zoom, 0, image_size)


def make_poses(seed, name, J):
    """(joints3d [B, P, J, 3] fp64, vis3d [B, P, J] uint8, count [B] int32): people drawn around the
    capture-space centre within +-0.6 of the space size (so that most leave some camera's image and
    some stand behind a camera), one person per frame with joints_3d_vis == 0 on a third of the
    joints, frame 1 with count < P and NaN in its padded rows."""
    rng = np.random.default_rng(seed)
    _, _, size, centre = CALIBRATIONS[name]
    joints = np.full((B, P, J, 3), np.nan)
    vis = np.ones((B, P, J), np.uint8)
    count = np.array([P, P - 2], np.int32)
    for b in range(B):
        for n in range(int(count[b])):
            c = np.asarray(centre) + rng.uniform(-0.6, 0.6, 3) * np.asarray(size)
            joints[b, n] = c + rng.normal(size=(J, 3)) * (250.0, 250.0, 450.0)
        vis[b, 1, rng.permutation(J)[:J // 3]] = 0
        vis[b, int(count[b]):] = 0
    return joints, vis, count


def coverage(joints3d, vis3d, count, cams, resize_t, ori_image_size, image_size):
    """Counts over the live joints of every view, for the coverage assertions."""
    keys = ("left", "right", "top", "bottom", "behind", "only_vis3d", "visible", "live", "second_neg", "second_right",
            "second_below")
    out = dict.fromkeys(keys, 0)
    for b in range(joints3d.shape[0]):
        n = int(count[b])
        for v in range(cams.shape[0]):
            _, vis, d = project(joints3d[b, :n], vis3d[b, :n], cams[v], resize_t, ori_image_size, image_size)
            second = d["neg"] | d["right"] | d["below"]
            out["left"] += int(np.count_nonzero(d["px"] < 0))
            out["right"] += int(np.count_nonzero(d["px"] > ori_image_size[0] - 1))
            out["top"] += int(np.count_nonzero(d["py"] < 0))
            out["bottom"] += int(np.count_nonzero(d["py"] > ori_image_size[1] - 1))
            out["behind"] += int(np.count_nonzero(d["behind"]))
            out["only_vis3d"] += int(np.count_nonzero(~d["seen3"] & d["first"] & ~second))
            out["visible"] += int(np.count_nonzero(vis))
            out["live"] += vis.size
            for key, flag in (("second_neg", d["neg"]), ("second_right", d["right"]), ("second_below", d["below"])):
                out[key] += int(np.count_nonzero(d["first"] & flag))
    return out


@functools.lru_cache(maxsize=None)
def built_case(index):
    """Case `index` of CASES, built from its seed (read-only arrays)."""
    name, J, hm, zoom, seed = CASES[index]
    joints3d, vis3d, count = make_poses(seed, name, J)
    c = dict(calibration=name, J=J, heatmap_size=hm, zoom=zoom, image_size=IMAGE_SIZE, sigma=SIGMA,
             ori_image_size=CALIBRATIONS[name][1], joints3d=joints3d, vis3d=vis3d, count=count,
             cams=cameras64(name), resize_t=resize_transform(name, zoom))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def golden_cases():
    """The cases of tests/golden/render_gt.npz (tools/gen_render_gt_golden.py): recorded inputs and the
    reference's 2-D keypoints, flags and heatmaps."""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_gt.npz"))
    cases = []
    for c in range(int(d["n_cases"])):
        case = {k: d[f"c{c}_{k}"] for k in ("joints3d", "vis3d", "count", "cams", "resize_t", "joints2d", "vis2d",
                                           "heatmaps")}
        for a in case.values():
            a.setflags(write=False)
        case.update(calibration=str(d[f"c{c}_calibration"]), zoom=float(d[f"c{c}_zoom"]),
                    J=case["joints3d"].shape[2], heatmap_size=tuple(int(x) for x in d[f"c{c}_heatmap_size"]),
                    ori_image_size=tuple(int(x) for x in d[f"c{c}_ori_image_size"]),
                    image_size=tuple(int(x) for x in d["image_size"]), sigma=float(d["sigma"]))
        cases.append(case)
    return cases
