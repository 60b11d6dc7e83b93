"""CPU tests of the augmented input heatmaps' host side: fvp.heatmaps.draw_augmentation
and the numpy restatement of the kernel (tests/render_aug_ref.py) against the
reference's recorded heatmaps and stream positions (tests/golden/render_aug.npz,
tools/gen_render_aug_golden.py), the faults the golden must catch, the new C-ABI
entries' argument checks and the Python layer's refusals and fake kernels."""
import os
import random

import numpy as np
import pytest
import torch

import render_aug_ref as A
import render_ref as R
from conftest import GOLDEN

NULL, SHAPE = 1001, 1002
TOL = 1e-6  # tests/test_gpu_render_aug.py derives it
N_CASES = 5


def _draw_case(index, global_streams=False):
    """(scale [B,V,P,J], rect [B,V,P,J,4], next) of a golden case from fvp.heatmaps.draw_augmentation."""
    from fvp.heatmaps import draw_augmentation

    c = A.golden_cases()[index]
    Bn, V, P, J, _ = c["joints"].shape
    scale, rect = A.identity((Bn, V, P, J))
    nxt = np.zeros(c["next"].shape, np.float64)
    kw = dict(image_size=c["image_size"], heatmap_size=c["heatmap_size"], sigma=c["sigma"])
    for idx, joints, count, vis, seed in A.frames(c):
        if global_streams:
            random.seed(seed)
            np.random.seed(seed)
            aug = draw_augmentation(torch.from_numpy(np.array(joints)), torch.from_numpy(np.array(count)),
                                    None if vis is None else torch.from_numpy(np.array(vis)), **kw)
            nxt[idx] = (random.random(), np.random.uniform())
        else:
            rngs = A.seeded(seed)
            aug = draw_augmentation(joints, count, vis, py_rng=rngs[0], np_rng=rngs[1], **kw)
            nxt[idx] = A.next_values(*rngs)
        assert aug.scale.dtype == torch.float32 and aug.rect.dtype == torch.int16
        assert tuple(aug.scale.shape) == joints.shape[:3] and tuple(aug.rect.shape) == joints.shape[:3] + (4,)
        if len(idx) == 1:
            scale[idx[0]], rect[idx[0]] = aug.scale.numpy(), aug.rect.numpy()
        else:
            scale[idx], rect[idx] = aug.scale.numpy()[0], aug.rect.numpy()[0]
    return scale, rect, nxt


def _mismatch(case, scale, rect, nxt, clamp=True):
    """What differs between the golden and the restatement under these records: a list of strings."""
    c = A.golden_cases()[case]
    got = A.render(c["joints"], A.case_count(c), c["vis"], scale, rect, c["image_size"], c["heatmap_size"], c["sigma"],
                   clamp=clamp)
    ref = c["heatmaps"]
    assert got.shape == ref.shape and got.dtype == np.float32 and ref.dtype == np.float32
    bad = []
    if not np.array_equal(got != 0, ref != 0):
        bad.append(f"support differs at {np.count_nonzero((got != 0) != (ref != 0))} elements")
    err = float(np.abs(got - ref).max())
    if err > TOL:
        bad.append(f"max abs error {err:.3g}")
    if not np.array_equal(nxt, c["next"]):
        bad.append("stream position differs")
    return bad, err


def test_golden_file_is_small_and_holds_the_cases():
    assert os.path.getsize(os.path.join(GOLDEN, "render_aug.npz")) < (1 << 19)
    cases = A.golden_cases()
    assert len(cases) == N_CASES and [c["kind"] for c in cases] == ["pred"] * 4 + ["gt"]
    kp = R.golden_cases()
    for c, k in zip(cases[:4], kp):  # the people of render_kp.npz, painted with augmentation
        assert np.array_equal(c["joints"], k["joints"], equal_nan=True) and np.array_equal(c["count"], k["count"])
        assert (c["vis"] is None) == (k["vis"] is None) and c["heatmap_size"] == k["heatmap_size"]
        assert c["heatmaps"].shape == k["heatmaps"].shape
        assert not np.array_equal(c["heatmaps"], k["heatmaps"])
    assert {(c["J"], c["heatmap_size"]) for c in cases} >= {(17, (48, 32)), (15, (50, 37)), (17, (50, 37)),
                                                             (15, (48, 32))}
    import render_gt_ref as G

    gt, built = cases[4], G.built_case(cases[4]["gt_case"])
    j2, v2 = G.project_batch(built["joints3d"], built["vis3d"], built["count"], built["cams"][None], None,
                             built["resize_t"], built["ori_image_size"], built["image_size"])
    n = [int(x) for x in gt["count"]]
    for b in range(G.B):  # the 'gt' case holds the keypoints the branch painted with
        assert gt["joints"][b, :, :n[b]].tobytes() == j2[b, :, :n[b]].tobytes()
    assert np.array_equal(gt["vis"], v2) and np.array_equal(gt["count"], built["count"])
    for c in cases:
        assert 0.0 <= c["heatmaps"].min() and c["heatmaps"].max() == 1.0 and c["heatmaps"].dtype == np.float32


def test_golden_covers_every_listed_condition():
    found = set()
    largest = 0.0
    for i, c in enumerate(A.golden_cases()):
        scale, rect, _ = A.golden_records(i)
        largest = max(largest, float(scale.max()))
        cnt = A.case_count(c)
        W, H = c["heatmap_size"]
        for b in range(c["joints"].shape[0]):
            vis = None if c["vis"] is None else c["vis"][b]
            wins = R.windows(c["joints"][b], cnt[b], vis, c["image_size"], c["heatmap_size"], c["sigma"])
            if vis is not None and any((vis[v, :int(cnt[b, v])] == 0).any() for v in range(vis.shape[0])):
                found.add("vis_skipped")
            for v, p, j, ul, br, skipped, n, c0, _ in wins:
                if skipped:
                    found.add("off_map_skipped")
                    assert scale[b, v, p, j] == 1 and not rect[b, v, p, j].any()  # drew nothing
                    continue
                if br[0] == 0 or br[1] == 0:
                    found.add("br_zero")
                x0, x1, y0, y1 = max(0, ul[0]), min(br[0], W, ul[0] + n), max(0, ul[1]), min(br[1], H, ul[1] + n)
                if x0 >= x1 or y0 >= y1:
                    continue
                r0, r1, q0, q1 = (int(x) for x in rect[b, v, p, j])
                cuts = max(r0, y0 - ul[1]) < min(r1, y1 - ul[1]) and max(q0, x0 - ul[0]) < min(q1, x1 - ul[0])
                found.add("rect_cuts" if cuts else "rect_misses")
                s = float(scale[b, v, p, j])
                on_map = x0 <= ul[0] + c0 < x1 and y0 <= ul[1] + c0 < y1
                if s > 1 and on_map and not (r0 <= c0 < r1 and q0 <= c0 < q1):
                    found.add("scale_above_1_on_map")
                if s == 1.0:
                    found.add("unscaled")
                if 0.35 < s < 0.55:  # 0.5 x (1 or 0.9 +- 0.03 randn)
                    found.add("half")
                if j in (9, 10) and 0.14 < s < 0.22:  # 0.2 x (1 or 0.9 +- 0.03 randn)
                    found.add("fifth")
    assert found == {"vis_skipped", "off_map_skipped", "br_zero", "rect_cuts", "rect_misses", "scale_above_1_on_map",
                     "unscaled", "half", "fifth"}, found
    assert 1.0 < largest < A.MAX_SCALE


@pytest.mark.parametrize("case", range(N_CASES))
def test_draw_then_restatement_matches_the_reference(case):
    """Same seeds -> the same draws: support identical everywhere, values within the bound, and
    both streams left where the reference left them (skipped joints drew nothing)."""
    scale, rect, nxt = _draw_case(case)
    ref_scale, ref_rect, ref_next = A.golden_records(case)  # the independent restatement of the draws
    assert np.array_equal(scale, ref_scale) and np.array_equal(rect, ref_rect) and np.array_equal(nxt, ref_next)
    bad, err = _mismatch(case, scale, rect, nxt)
    print(f"draw_augmentation + render_aug_ref vs reference, case {case}: max abs error {err:.3g}")
    assert not bad, bad


@pytest.mark.parametrize("case", [0, 4])
def test_draw_reads_the_global_streams_by_default(case):
    state = random.getstate(), np.random.get_state()
    try:
        scale, rect, nxt = _draw_case(case, global_streams=True)
    finally:
        random.setstate(state[0])
        np.random.set_state(state[1])
    ref_scale, ref_rect, _ = A.golden_records(case)
    assert np.array_equal(scale, ref_scale) and np.array_equal(rect, ref_rect)
    assert np.array_equal(nxt, A.golden_cases()[case]["next"])


def _fails_somewhere(records_of, clamp=True):
    hits = []
    for case in range(N_CASES):
        bad, _ = _mismatch(case, *records_of(case), clamp=clamp)
        if bad:
            hits.append((case, bad))
    return hits


def test_planted_faults_fail_against_the_golden():
    assert not _fails_somewhere(A.golden_records)  # (the sound restatement passes: the faults below are the cause)
    no_clamp = _fails_somewhere(A.golden_records, clamp=False)
    assert no_clamp and all("max abs error" in " ".join(b) for _, b in no_clamp), no_clamp

    def transposed(case):
        scale, rect, nxt = A.golden_records(case)
        return scale, rect[..., [2, 3, 0, 1]], nxt

    assert len(_fails_somewhere(transposed)) == N_CASES
    swapped = _fails_somewhere(lambda case: A.golden_records(case, "swap_random"))
    assert len(swapped) == N_CASES
    skipped = _fails_somewhere(lambda case: A.golden_records(case, "draw_skipped"))
    assert len(skipped) == N_CASES and all("stream position differs" in b for _, b in skipped), skipped


def test_skipped_joints_get_the_identity_record():
    from fvp.heatmaps import draw_augmentation

    c = A.golden_cases()[2]  # with vis
    kw = dict(image_size=c["image_size"], heatmap_size=c["heatmap_size"], sigma=c["sigma"])
    joints, count, vis = np.array(c["joints"][0]), np.array(c["count"][0]), np.array(c["vis"][0])
    aug = draw_augmentation(joints, count, vis, py_rng=random.Random(1), np_rng=np.random.RandomState(1), **kw)
    s, r = aug.scale.numpy(), aug.rect.numpy()
    hidden = vis == 0
    assert hidden.any() and (s[hidden] == 1).all() and not r[hidden].any()
    for v in range(joints.shape[0]):  # rows at or beyond count
        assert (s[v, int(count[v]):] == 1).all() and not r[v, int(count[v]):].any()
    drawn = (r[..., 1] > r[..., 0]) & (r[..., 3] > r[..., 2])
    assert drawn.any() and (s[drawn] > 0).all() and (s != 1).any()
    H, W = c["heatmap_size"][1], c["heatmap_size"][0]
    assert r[drawn][:, 1].max() <= H and r[drawn][:, 3].max() <= W and r.min() >= 0
    # a person with a non-finite coordinate draws nothing; the people after it draw what they drew without it
    bad = joints.copy()
    bad[0, 0, 3, 1] = np.nan
    less, cnt = joints.copy(), count.copy()
    less[0, :-1], cnt[0] = joints[0, 1:], count[0] - 1
    vless = vis.copy()
    vless[0, :-1] = vis[0, 1:]
    a = draw_augmentation(bad, count, vis, py_rng=random.Random(2), np_rng=np.random.RandomState(2), **kw)
    b = draw_augmentation(less, cnt, vless, py_rng=random.Random(2), np_rng=np.random.RandomState(2), **kw)
    assert (a.scale[0, 0] == 1).all() and not a.rect[0, 0].any()
    n = int(count[0])
    assert torch.equal(a.scale[0, 1:n], b.scale[0, :n - 1]) and torch.equal(a.rect[0, 1:n], b.rect[0, :n - 1])
    assert torch.equal(a.scale[1], b.scale[1]) and torch.equal(a.rect[1], b.rect[1])
    # the default collate's stack
    from torch.utils.data import default_collate

    batch = default_collate([aug, a])
    assert type(batch).__name__ == "Augmentation" and tuple(batch.scale.shape) == (2,) + s.shape
    assert tuple(batch.rect.shape) == (2,) + r.shape and batch.rect.dtype == torch.int16
    from fvp import _lib

    for wrong in (lambda: draw_augmentation(joints[0], count, None, **kw),
                  lambda: draw_augmentation(joints, count[:1], None, **kw),
                  lambda: draw_augmentation(joints, count, vis[:, :2], **kw)):
        with pytest.raises(_lib.FvpError):
            wrong()


# -- the C entry points' host refusals ----------------------------------------------------------
def _keypoints_aug(**kw):
    from fvp import _lib

    a = dict(joints=1, joints_f64=1, count=1, vis=None, aug_scale=1, aug_rect=1, B=2, V=2, P=5, J=17, H=32, W=48,
             image_w=192.0, image_h=128.0, sigma=3.0, Cp=32, out=16, out_half=0)
    assert set(kw) <= set(a)
    a.update(kw)
    return _lib.load().fvp_render_keypoints_aug(*a.values(), None)


def _poses_aug(**kw):
    from fvp import _lib

    a = dict(joints3d=1, vis3d=None, count=1, B=2, P=5, J=17, cams64=1, cam_index=None, S=1, V=5, resize_t64=1,
             ori_w=1032.0, ori_h=776.0, image_w=192.0, image_h=128.0, aug_scale=1, aug_rect=1, H=32, W=48, sigma=3.0,
             Cp=32, out=16, out_half=0, joints2d=None, vis2d=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return _lib.load().fvp_render_poses3d_aug(*a.values(), None)


def test_aug_entries_reject_bad_arguments_on_the_host():
    """Every refusal returns before anything is launched (the pointers are not device pointers)."""
    for key in ("joints", "count", "out", "aug_scale", "aug_rect"):
        assert _keypoints_aug(**{key: None}) == NULL, key
    for key in ("joints3d", "count", "cams64", "resize_t64", "out", "aug_scale", "aug_rect"):
        assert _poses_aug(**{key: None}) == NULL, key
    shapes = (dict(J=0), dict(J=33, Cp=48), dict(P=0), dict(P=33), dict(V=0), dict(B=0), dict(Cp=8), dict(Cp=16),
              dict(Cp=24), dict(Cp=48), dict(H=0), dict(W=0), dict(W=-3), dict(sigma=0.0), dict(sigma=float("nan")),
              dict(image_w=0.0), dict(image_h=float("nan")), dict(image_w=float("inf")))  # Cp = 16 < J = 17
    for call in (_keypoints_aug, _poses_aug):
        for bad in shapes:
            assert call(**bad) == SHAPE, (call.__name__, bad)
        assert call(out=8, out_half=1) == SHAPE  # 16-B stores
    for bad in (dict(V=256), dict(S=0), dict(ori_w=0.0), dict(ori_h=-1.0)):
        assert _poses_aug(**bad) == SHAPE, bad


def test_abi_version_is_unchanged():
    from fvp import _lib

    assert _lib.load().fvp_abi_version() == 22 and _lib.ABI_VERSION == 22
    assert {"fvp_render_keypoints_aug", "fvp_render_poses3d_aug"} <= set(_lib.SIGNATURES)


# -- the Python layer --------------------------------------------------------------------------
def test_augment_refusals_on_the_host():
    from fvp import _lib
    from fvp.heatmaps import Augmentation, render_keypoints, render_poses3d

    kw = dict(image_size=R.IMAGE_SIZE, heatmap_size=(48, 32), sigma=R.SIGMA)
    joints = torch.zeros((2, 2, 5, 17, 2), dtype=torch.float64)
    count = torch.ones((2, 2), dtype=torch.int32)
    scale, rect = (torch.from_numpy(a) for a in A.identity((2, 2, 5, 17)))
    with pytest.raises(_lib.FvpError, match="HIP device"):  # the operands' own check comes first
        render_keypoints(joints, count, augment=Augmentation(scale, rect), **kw)
    j3 = torch.zeros((2, 5, 17, 3), dtype=torch.float64)
    with pytest.raises(_lib.FvpError, match="HIP device"):
        render_poses3d(j3, None, torch.ones((2,), dtype=torch.int32), torch.zeros((5, 24), dtype=torch.float64),
                       torch.zeros((2, 3), dtype=torch.float64), ori_image_size=(1032, 776),
                       augment=Augmentation(scale, rect), **kw)
    from fvp.heatmaps import _augment_records

    dev = torch.device("cpu")
    assert [tuple(t.shape) for t in _augment_records("x", (scale, rect), (2, 2, 5, 17), dev)] == [(2, 2, 5, 17),
                                                                                                 (2, 2, 5, 17, 4)]
    for bad in ((scale, rect[..., :3]), (scale[:1], rect), (scale.double(), rect), (scale, rect.int()), (scale,),
                scale, (scale.numpy(), rect.numpy()), (rect, scale)):
        with pytest.raises(_lib.FvpError, match="augment"):
            _augment_records("x", bad, (2, 2, 5, 17), dev)


def test_aug_ops_fake_shapes():
    from fvp import ops  # noqa: F401  (registers torch.ops.fvp.*)

    for J, cp in ((15, 16), (17, 32)):
        joints = torch.empty((2, 3, 5, J, 2), dtype=torch.float64, device="meta")
        count = torch.empty((2, 3), dtype=torch.int32, device="meta")
        scale = torch.empty((2, 3, 5, J), dtype=torch.float32, device="meta")
        rect = torch.empty((2, 3, 5, J, 4), dtype=torch.int16, device="meta")
        for half, dtype in ((False, torch.float32), (True, torch.float16)):
            out = torch.ops.fvp.render_keypoints_aug(joints, count, None, scale, rect, 192.0, 128.0, 37, 50, 3.0, half)
            assert tuple(out.shape) == (2, 3, 37, 50, cp) and out.dtype == dtype and out.device.type == "meta"
            j3 = torch.empty((2, 5, J, 3), dtype=torch.float64, device="meta")
            cams = torch.empty((1, 3, 24), dtype=torch.float64, device="meta")
            t = torch.empty((2, 3), dtype=torch.float64, device="meta")
            c1 = torch.empty((2,), dtype=torch.int32, device="meta")
            out, k2, f2 = torch.ops.fvp.render_poses3d_aug(j3, None, c1, cams, None, t, scale, rect, 1032.0, 776.0,
                                                           192.0, 128.0, 37, 50, 3.0, True, half)
            assert tuple(out.shape) == (2, 3, 37, 50, cp) and out.dtype == dtype
            assert tuple(k2.shape) == (2, 3, 5, J, 2) and tuple(f2.shape) == (2, 3, 5, J)
