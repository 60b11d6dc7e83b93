"""numpy restatement of fvp_render_keypoints_aug (include/fvp.h), for the augmented
render tests: the reference's generate_input_heatmap (lib/dataset/JointsDataset.py:
368-447) with data_augmentation = True, on top of the windows of tests/render_ref.py.
The random draws are an input (one record per joint); `draw` restates the order in
which the reference consumes Python's and numpy's streams, independently of
fvp.heatmaps.draw_augmentation, and can plant the faults the golden must catch.
Also the loader of tests/golden/render_aug.npz (tools/gen_render_aug_golden.py)."""
import functools
import os
import random

import numpy as np

import render_ref as R

# largest factor the bound of the GPU tests is derived for (tests/test_gpu_render_aug.py)
MAX_SCALE = 1.2


def identity(shape):
    """Records that change nothing: scale 1, empty rectangle."""
    return np.ones(shape, np.float32), np.zeros(tuple(shape) + (4,), np.int16)


def render_frame(joints, count, vis, scale, rect, image_size, heatmap_size, sigma, clamp=True):
    """joints [V, P, J, 2], count [V], vis [V, P, J] or None, scale [V, P, J] fp32, rect [V, P, J, 4]
    int16 (r0, r1, c0, c1 in patch coordinates) -> planar heatmaps [V, J, H, W] fp32.
    clamp=False plants the fault of a kernel without the final min(., 1)."""
    W, H = heatmap_size
    V, _, J, _ = joints.shape
    out = np.zeros((V, J, H, W), np.float32)
    for v, p, j, ul, br, skipped, n, c0, inv in R.windows(joints, count, vis, image_size, heatmap_size, sigma):
        if skipped:
            continue
        x0, x1 = max(0, ul[0]), min(br[0], W, ul[0] + n)
        y0, y1 = max(0, ul[1]), min(br[1], H, ul[1] + n)
        if x0 >= x1 or y0 >= y1:
            continue
        xs, ys = np.arange(x0, x1), np.arange(y0, y1)
        dx = (xs - (ul[0] + c0)).astype(np.float32)
        dy = (ys - (ul[1] + c0)).astype(np.float32)
        g = np.exp(-((dx[None, :] * dx[None, :] + dy[:, None] * dy[:, None]) * inv))
        assert g.dtype == np.float32
        r0, r1, q0, q1 = (max(int(x), 0) for x in rect[v, p, j])
        px, py = xs - ul[0], ys - ul[1]  # patch coordinates: all within 0 .. n-1
        cut = ((py >= r0) & (py < r1))[:, None] & ((px >= q0) & (px < q1))[None, :]
        with np.errstate(invalid="ignore"):
            val = np.where(cut, np.float32(0), g * np.float32(scale[v, p, j]))
        assert val.dtype == np.float32
        # fmax: a NaN product loses to the running maximum, which starts at 0, as a negative one does
        out[v, j, y0:y1, x0:x1] = np.fmax(out[v, j, y0:y1, x0:x1], val)
    return np.minimum(out, np.float32(1)) if clamp else out


def render(joints, count, vis, scale, rect, image_size, heatmap_size, sigma, clamp=True):
    """Batched: a leading B on every operand -> [B, V, J, H, W] fp32."""
    return np.stack([render_frame(joints[b], count[b], None if vis is None else vis[b], scale[b], rect[b], image_size,
                                  heatmap_size, sigma, clamp) for b in range(joints.shape[0])])


def draw(joints, count, vis, image_size, heatmap_size, sigma, py_rng, np_rng, fault=None):
    """The draws of one frame, views then people then joints: (scale [V, P, J] fp32, rect [V, P, J, 4]
    int16, detail) with detail a list of (v, p, j, scaled, second) per drawing joint -- `scaled`: the
    first factor was drawn, `second`: the second factor applied (1.0 if none).
    fault: None, 'swap_random' (the two random() values used in the other order) or 'draw_skipped'
    (joints skipped by vis or the off-map test draw too)."""
    W, H = heatmap_size
    V, P, J, _ = joints.shape
    scale, rect = identity((V, P, J))
    detail = []
    shown = {(v, p, j): skipped for v, p, j, _, _, skipped, _, _, _ in
             R.windows(joints, count, vis, image_size, heatmap_size, sigma)}
    finite = {(v, p) for v, p, _ in shown}
    for v in range(V):
        for p in range(int(count[v])):
            for j in range(J):
                skipped = shown.get((v, p, j), True)
                if skipped and not (fault == "draw_skipped" and (v, p) in finite):
                    continue
                a = py_rng.random()
                if fault == "swap_random":
                    b = py_rng.random()
                    a, b = b, a
                s = 0.9 + np_rng.randn(1) * 0.03 if a < 0.6 else 1.0
                scaled = a < 0.6
                if fault != "swap_random":
                    b = py_rng.random()
                second = 1.0
                if j in (7, 8):
                    second = 0.5 if b < 0.1 else 1.0
                elif j in (9, 10):
                    second = 0.2 if b < 0.1 else 1.0
                elif b < 0.05:
                    second = 0.5
                s = s * second if second != 1.0 else s
                start = [int(np_rng.uniform(0, H - 1)), int(np_rng.uniform(0, W - 1))]
                end = [int(min(start[0] + np_rng.uniform(H / 4, H * 0.75), H)),
                       int(min(start[1] + np_rng.uniform(W / 4, W * 0.75), W))]
                if skipped:
                    continue
                scale[v, p, j] = np.float32(np.asarray(s, np.float64).reshape(-1)[0])
                rect[v, p, j] = (start[0], end[0], start[1], end[1])
                detail.append((v, p, j, scaled, second))
    return scale, rect, detail


def seeded(seed):
    """(random.Random, np.random.RandomState) seeded as random.seed(seed) and np.random.seed(seed) seed the
    global streams."""
    return random.Random(seed), np.random.RandomState(seed)


def next_values(py_rng, np_rng):
    """The next value of each stream: equal to the recorded ones iff the same draws were consumed."""
    return np.array([py_rng.random(), np_rng.uniform()], np.float64)


@functools.lru_cache(maxsize=None)
def golden_cases():
    """The cases of tests/golden/render_aug.npz.  'pred' cases: joints [B, V, P, J, 2], count [B, V],
    vis or None, seeds [B, V] (one per frame-view), next [B, V, 2], heatmaps [B, V, J, H, W].  The 'gt'
    case (kind == 'gt'): joints2d / vis2d as the branch computed them, count [B] per frame, seeds [B]
    (one per frame: its views share the streams), next [B, 2]."""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_aug.npz"))
    cases = []
    for c in range(int(d["n_cases"])):
        case = dict(kind=str(d[f"c{c}_kind"]), joints=d[f"c{c}_joints"], count=d[f"c{c}_count"],
                    vis=d[f"c{c}_vis"] if f"c{c}_vis" in d.files else None, seeds=d[f"c{c}_seeds"],
                    next=d[f"c{c}_next"], heatmaps=d[f"c{c}_heatmaps"])
        for a in case.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        case.update(heatmap_size=tuple(int(x) for x in d[f"c{c}_heatmap_size"]),
                    image_size=tuple(int(x) for x in d["image_size"]), sigma=float(d["sigma"]),
                    J=case["joints"].shape[3])
        if case["kind"] == "gt":
            case.update(gt_case=int(d[f"c{c}_gt_case"]))
        cases.append(case)
    return cases


def frames(case):
    """The seeded units of a case: (index into heatmaps / next, joints [V', P, J, 2], count [V'], vis or None,
    seed) -- a frame-view (V' = 1) of a 'pred' case, a frame with all its views of the 'gt' case."""
    out = []
    Bn, V = case["joints"].shape[:2]
    for b in range(Bn):
        if case["kind"] == "gt":
            cnt = np.repeat(case["count"][b], V)
            out.append(((b,), case["joints"][b], cnt, case["vis"][b], int(case["seeds"][b])))
            continue
        for v in range(V):
            vis = None if case["vis"] is None else case["vis"][b, v:v + 1]
            out.append(((b, v), case["joints"][b, v:v + 1], case["count"][b, v:v + 1], vis, int(case["seeds"][b, v])))
    return out


@functools.lru_cache(maxsize=None)
def golden_records(index, fault=None):
    """(scale [B, V, P, J], rect [B, V, P, J, 4], next [...]) of golden case `index` drawn by `draw` with
    the recorded seeds."""
    case = golden_cases()[index]
    Bn, V, P, J, _ = case["joints"].shape
    scale, rect = identity((Bn, V, P, J))
    nxt = np.zeros(case["next"].shape, np.float64)
    for idx, joints, count, vis, seed in frames(case):
        rngs = seeded(seed)
        s, r, _ = draw(joints, count, vis, case["image_size"], case["heatmap_size"], case["sigma"], *rngs, fault=fault)
        if len(idx) == 1:
            scale[idx[0]], rect[idx[0]] = s, r
        else:
            scale[idx], rect[idx] = s[0], r[0]
        nxt[idx] = next_values(*rngs)
    for a in (scale, rect, nxt):
        a.setflags(write=False)
    return scale, rect, nxt


def case_count(case):
    """count [B, V] of a case (the 'gt' case's per-frame count holds for every view)."""
    if case["kind"] == "gt":
        return np.repeat(np.asarray(case["count"], np.int32)[:, None], case["joints"].shape[1], axis=1)
    return case["count"]
