"""numpy restatement of fvp_render_keypoints (include/fvp.h), for the render
tests: the reference's generate_input_heatmap (lib/dataset/JointsDataset.py:
368-447) with data_augmentation = False, per-joint setup in fp64 in its
operation order, per-pixel values in fp32.  Also the people the tests paint."""
import math
import os

import numpy as np

LIMIT = float(1 << 30)


def _int(v):
    """Python's int() (truncation toward zero), pinned to +-2^30 as the kernel pins it."""
    return int(min(max(float(v), -LIMIT), LIMIT))


def person_setup(q, sigma):
    """(tmp, n, c0, inv) of one person from q [J, 2] = joints / feat_stride (all J joints)."""
    ext = np.maximum(q[:, 1].max() - q[:, 1].min(), q[:, 0].max() - q[:, 0].min())
    scale = 2 * np.clip(ext * ext, 1.0 / 4 * 96 ** 2, 4 * 96 ** 2)
    cur = np.float64(sigma) * np.sqrt(scale / (96.0 * 96.0))
    tmp = cur * 3
    size = 2 * tmp + 1
    return float(tmp), _int(math.ceil(size)), _int(math.floor(size / 2)), np.float32(1.0 / (2 * (cur * cur)))


def windows(joints, count, vis, image_size, heatmap_size, sigma):
    """The window records of one frame: (v, p, j, ul, br, skipped) for every visible joint of
    every finite person below count."""
    W, H = heatmap_size
    stride = np.asarray(image_size, np.float64) / np.asarray(heatmap_size, np.float64)
    out = []
    for v in range(joints.shape[0]):
        for p in range(int(count[v])):
            q = joints[v, p].astype(np.float64) / stride
            if not np.isfinite(q).all():
                continue
            tmp, n, c0, inv = person_setup(q, sigma)
            for j in range(q.shape[0]):
                if vis is not None and vis[v, p, j] == 0:
                    continue
                mu = (_int(q[j, 0]), _int(q[j, 1]))
                ul = (_int(mu[0] - tmp), _int(mu[1] - tmp))
                br = (_int(mu[0] + tmp + 1), _int(mu[1] + tmp + 1))
                skipped = ul[0] >= W or ul[1] >= H or br[0] < 0 or br[1] < 0
                out.append((v, p, j, ul, br, skipped, n, c0, inv))
    return out


def render_frame(joints, count, vis, image_size, heatmap_size, sigma):
    """joints [V, P, J, 2], count [V], vis [V, P, J] or None -> planar heatmaps [V, J, H, W] fp32."""
    W, H = heatmap_size
    V, _, J, _ = joints.shape
    out = np.zeros((V, J, H, W), np.float32)
    for v, p, j, ul, br, skipped, n, c0, inv in windows(joints, count, vis, image_size, heatmap_size, sigma):
        if skipped:
            continue
        x0, x1 = max(0, ul[0]), min(br[0], W, ul[0] + n)
        y0, y1 = max(0, ul[1]), min(br[1], H, ul[1] + n)
        if x0 >= x1 or y0 >= y1:
            continue
        dx = (np.arange(x0, x1) - (ul[0] + c0)).astype(np.float32)
        dy = (np.arange(y0, y1) - (ul[1] + c0)).astype(np.float32)
        g = np.exp(-((dx[None, :] * dx[None, :] + dy[:, None] * dy[:, None]) * inv))
        assert g.dtype == np.float32
        out[v, j, y0:y1, x0:x1] = np.maximum(out[v, j, y0:y1, x0:x1], g)
    return out


def render(joints, count, vis, image_size, heatmap_size, sigma):
    """Batched: joints [B, V, P, J, 2], count [B, V], vis [B, V, P, J] or None -> [B, V, J, H, W] fp32."""
    return np.stack([render_frame(joints[b], count[b], None if vis is None else vis[b], image_size, heatmap_size,
                                  sigma) for b in range(joints.shape[0])])


# -- the people the tests paint ---------------------------------------------------------
IMAGE_SIZE = (192, 128)
SIGMA = 3.0
B, V, P = 2, 2, 5


def _person(rng, J, centre_hm, extent_hm, stride):
    """J joints scattered over extent_hm heatmap pixels around centre_hm, in image pixels; two
    joints pinned to the box's ends so that the extent is what was asked for."""
    q = np.asarray(centre_hm, np.float64) + rng.uniform(-0.5, 0.5, (J, 2)) * extent_hm
    q[0] = np.asarray(centre_hm) - 0.5 * extent_hm
    q[1] = np.asarray(centre_hm) + 0.5 * extent_hm
    return q * stride


def make_people(seed, J, heatmap_size, image_size=IMAGE_SIZE):
    """(joints [B, V, P, J, 2] fp64, count [B, V] int32) with, over the four frame-views: a
    person well inside, one straddling the top-left corner at negative coordinates, one
    straddling the bottom-right, one wholly outside on each of the four sides (the left one
    with br.x == 0: not skipped, paints nothing; the others skipped by each condition), a tiny
    person (scale clipped low), a huge one (clipped high), one between the clips, and two that
    overlap; padded rows hold NaN."""
    rng = np.random.default_rng(seed)
    W, H = heatmap_size
    stride = np.asarray(image_size, np.float64) / np.asarray(heatmap_size, np.float64)
    inside = (W * 0.5 + rng.uniform(-3, 3), H * 0.5 + rng.uniform(-3, 3))
    views = [
        # well inside; top-left at negative coordinates; bottom-right; two overlapping the first
        [_person(rng, J, inside, 14.0, stride), _person(rng, J, (-1.5, -2.5), 6.0, stride),
         _person(rng, J, (W - 1.5, H - 0.5), 5.0, stride),
         _person(rng, J, (inside[0] + 4, inside[1] - 3), 12.0, stride),
         _person(rng, J, (inside[0] - 2, inside[1] + 5), 30.0, stride)],
        # outside: left with br.x == 0 (mu = -7, tmp = 6.36 at sigma 3), far left (br < 0), right, top, bottom
        [_person(rng, J, (-7.5, H * 0.5), 0.6, stride), _person(rng, J, (-30.0, H * 0.3), 3.0, stride),
         _person(rng, J, (W + 12.0, H * 0.6), 4.0, stride), _person(rng, J, (W * 0.4, -25.0), 4.0, stride),
         _person(rng, J, (W * 0.7, H + 15.0), 4.0, stride)],
        # tiny (clipped low); huge (clipped high); between the clips (ext in 48 .. 192 heatmap px)
        [_person(rng, J, (W * 0.25, H * 0.7), 0.8, stride), _person(rng, J, (W * 0.5, H * 0.5), 260.0, stride),
         _person(rng, J, (W * 0.6, H * 0.4), 90.0, stride)],
        # random people, some partly off the heatmap
        [_person(rng, J, (rng.uniform(-5, W + 5), rng.uniform(-5, H + 5)), rng.uniform(5, 70), stride)
         for _ in range(4)],
    ]
    joints = np.full((B, V, P, J, 2), np.nan)
    count = np.zeros((B, V), np.int32)
    for i, view in enumerate(views):
        count[i // V, i % V] = len(view)
        joints[i // V, i % V, :len(view)] = np.stack(view)
    return joints, count


def make_vis(seed, J):
    """[B, V, P, J] uint8, about a quarter of the joints invisible."""
    rng = np.random.default_rng(seed + 1000)
    return (rng.uniform(size=(B, V, P, J)) > 0.25).astype(np.uint8)


def golden_cases():
    """The cases of tests/golden/render_kp.npz (tools/gen_render_golden.py): inputs and the reference's heatmaps."""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_kp.npz"))
    cases = []
    for c in range(int(d["n_cases"])):
        cases.append(dict(joints=d[f"c{c}_joints"], count=d[f"c{c}_count"],
                          vis=d[f"c{c}_vis"] if f"c{c}_vis" in d.files else None,
                          heatmap_size=tuple(int(x) for x in d[f"c{c}_heatmap_size"]),
                          image_size=tuple(int(x) for x in d["image_size"]), sigma=float(d["sigma"]),
                          heatmaps=d[f"c{c}_heatmaps"]))
    return cases
