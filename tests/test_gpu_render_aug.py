"""GPU tests of fvp_render_keypoints_aug / fvp_render_poses3d_aug
(fvp.heatmaps.render_keypoints(augment=), render_poses3d(augment=)): input heatmaps
with the reference's data_augmentation = True painted in one launch from recorded
draws, against the reference's own heatmaps (tests/golden/render_aug.npz) and the
numpy restatement (tests/render_aug_ref.py).

Tolerance 1e-6 absolute, support (the non-zero set) identical.  Derivation: the
plain painter's fp32 value is within 1.9e-7 of the exact one; the
factor is at most MAX_SCALE = 1.2 (asserted on the golden's records): 2.3e-7; the
fp32 product and the fp32 rounding of the factor add 2 * 2^-24 = 1.2e-7 on values
<= 1.2; the reference's fp64 -> fp32 store adds 2^-25 = 3e-8.  Sum < 4.4e-7."""
import functools

import numpy as np
import pytest
import torch

import render_aug_ref as A
import render_gt_ref as G
import render_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-6
KW = dict(image_size=R.IMAGE_SIZE, sigma=R.SIGMA)


def _dev(dev, a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.array(a))  # (a copy: the shared cases are read-only)
    return (t if dtype is None else t.to(dtype)).to(dev)


def _render(dev, joints, count, vis, scale, rect, hm, dtype=None, image_size=R.IMAGE_SIZE, sigma=R.SIGMA):
    from fvp.heatmaps import Augmentation, render_keypoints

    aug = None if scale is None else Augmentation(_dev(dev, scale), _dev(dev, rect))
    return render_keypoints(_dev(dev, joints), _dev(dev, count), _dev(dev, vis), image_size=image_size,
                            heatmap_size=hm, sigma=sigma, dtype=dtype, augment=aug)


def _planar(cl):
    """The J joint planes [B, V, J, H, W] of a channels-last result, after checking its padding."""
    t = cl.t.float().cpu()
    assert t.shape[4] == 16 * ((cl.J + 15) // 16)
    assert not t[..., cl.J:].any(), "padding channels must be exactly zero"
    return t[..., :cl.J].permute(0, 1, 4, 2, 3).contiguous().numpy()


def _assert_close(got, ref, what, tol=TOL):
    assert got.shape == ref.shape
    diff = np.count_nonzero((got != 0) != (ref != 0))
    assert diff == 0, f"{what}: support differs at {diff} elements"
    err = float(np.abs(got - ref).max())
    print(f"{what}: max abs error {err:.3g} over {np.count_nonzero(ref)} painted values")
    assert err <= tol, f"{what}: max abs error {err}"


@functools.lru_cache(maxsize=None)
def _case(seed, J, with_vis):
    """People of tests/render_ref.py with drawn records and the restatement's heatmaps (read-only)."""
    hm = [(48, 32), (50, 37)][seed % 2]
    joints, count = R.make_people(seed, J, hm)
    vis = R.make_vis(seed, J) if with_vis else None
    scale, rect = A.identity((R.B, R.V, R.P, J))
    rngs = A.seeded(seed)
    for b in range(R.B):
        scale[b], rect[b], _ = A.draw(joints[b], count[b], None if vis is None else vis[b], R.IMAGE_SIZE, hm, R.SIGMA,
                                      *rngs)
    ref = A.render(joints, count, vis, scale, rect, R.IMAGE_SIZE, hm, R.SIGMA)
    for a in (joints, count, scale, rect, ref):
        a.setflags(write=False)
    return hm, joints, count, vis, scale, rect, ref


@pytest.mark.parametrize("case", range(5))
def test_golden_parity(gpu_device, case):
    """The reference's painter under recorded seeds == the draw helper's records through the kernel."""
    c = A.golden_cases()[case]
    scale, rect, _ = A.golden_records(case)
    assert float(scale.max()) < A.MAX_SCALE  # the bound's premise
    if c["kind"] == "gt":
        from fvp.heatmaps import Augmentation, render_poses3d

        b = G.built_case(c["gt_case"])
        cl = render_poses3d(_dev(gpu_device, b["joints3d"]), _dev(gpu_device, b["vis3d"]), _dev(gpu_device, b["count"]),
                            _dev(gpu_device, b["cams"]), _dev(gpu_device, b["resize_t"]),
                            ori_image_size=b["ori_image_size"], image_size=c["image_size"],
                            heatmap_size=c["heatmap_size"], sigma=c["sigma"],
                            augment=Augmentation(torch.from_numpy(np.array(scale)), torch.from_numpy(np.array(rect))))
    else:
        cl = _render(gpu_device, c["joints"], c["count"], c["vis"], scale, rect, c["heatmap_size"],
                     image_size=c["image_size"], sigma=c["sigma"])
    got = _planar(cl)
    _assert_close(got, c["heatmaps"], f"golden case {case} vs the reference")
    ref = A.render(c["joints"], A.case_count(c), c["vis"], scale, rect, c["image_size"], c["heatmap_size"], c["sigma"])
    _assert_close(got, ref, f"golden case {case} vs render_aug_ref")
    assert got.max() == 1.0


@pytest.mark.parametrize("J, with_vis, seed", [(15, False, 11), (17, True, 12), (17, False, 13), (15, True, 14)])
def test_random_parity_and_half(gpu_device, J, with_vis, seed):
    hm, joints, count, vis, scale, rect, ref = _case(seed, J, with_vis)
    f32 = _render(gpu_device, joints, count, vis, scale, rect, hm)
    assert f32.cp == (16 if J == 15 else 32) and f32.t.dtype == torch.float32
    _assert_close(_planar(f32), ref, f"J={J} vis={with_vis} seed={seed}")
    f16 = _render(gpu_device, joints, count, vis, scale, rect, hm, dtype=torch.float16)
    assert f16.t.dtype == torch.float16 and torch.equal(f16.t, f32.t.half())  # one rounding per channel
    # fp32 keypoints are widened on load
    j32 = joints.astype(np.float32)
    a = _render(gpu_device, j32, count, vis, scale, rect, hm)
    b = _render(gpu_device, j32.astype(np.float64), count, vis, scale, rect, hm)
    assert torch.equal(a.t, b.t)


@pytest.mark.parametrize("J, with_vis, seed", [(15, True, 11), (17, False, 12)])
def test_identity_records_change_nothing(gpu_device, J, with_vis, seed):
    hm, joints, count, vis, _, _, _ = _case(seed, J, with_vis)
    scale, rect = A.identity((R.B, R.V, R.P, J))
    for dtype in (None, torch.float16):
        plain = _render(gpu_device, joints, count, vis, None, None, hm, dtype=dtype)
        same = _render(gpu_device, joints, count, vis, scale, rect, hm, dtype=dtype)
        assert plain.t.any() and torch.equal(plain.t, same.t)


def test_poses3d_equals_the_two_step_route(gpu_device):
    from fvp.heatmaps import Augmentation, draw_augmentation, project_poses, render_keypoints, render_poses3d

    for index in (1, 3):  # Panoptic: 15 joints at 50 x 37; 17 joints at 48 x 32 under the zoomed transform
        b = G.built_case(index)
        ops = [_dev(gpu_device, b[k]) for k in ("joints3d", "vis3d", "count", "cams", "resize_t")]
        kw = dict(ori_image_size=b["ori_image_size"], image_size=b["image_size"])
        j2, v2 = project_poses(*ops, **kw)
        V = j2.shape[1]
        cnt = ops[2][:, None].expand(G.B, V).contiguous()
        rkw = dict(image_size=b["image_size"], heatmap_size=b["heatmap_size"], sigma=b["sigma"])
        rngs = A.seeded(index)
        augs = [draw_augmentation(j2[f].cpu(), cnt[f].cpu(), v2[f].cpu(), py_rng=rngs[0], np_rng=rngs[1], **rkw)
                for f in range(G.B)]
        aug = Augmentation(torch.stack([a.scale for a in augs]), torch.stack([a.rect for a in augs]))
        assert (aug.scale != 1).any()
        for dtype in (None, torch.float16):
            one, k2, f2 = render_poses3d(*ops, heatmap_size=b["heatmap_size"], sigma=b["sigma"], dtype=dtype,
                                         augment=aug, return_keypoints=True, **kw)
            two = render_keypoints(j2, cnt, v2, dtype=dtype, augment=aug, **rkw)
            assert one.t.any() and torch.equal(one.t, two.t)
            assert torch.equal(k2, j2) and torch.equal(f2, v2)
        plain = render_poses3d(*ops, heatmap_size=b["heatmap_size"], sigma=b["sigma"], dtype=torch.float16, **kw)
        assert not torch.equal(plain.t, one.t)  # (the augmentation did something)


def test_largest_view(gpu_device):
    """P = 32 people of J = 32 joints: the largest record table a block builds; the augmentation
    records live in it, so the block's LDS is the plain painter's."""
    rng = np.random.default_rng(7)
    hm = (50, 37)
    stride = np.asarray(R.IMAGE_SIZE, np.float64) / np.asarray(hm, np.float64)
    joints = np.stack([R._person(rng, 32, (rng.uniform(-4, 54), rng.uniform(-4, 41)), rng.uniform(2, 60), stride)
                       for _ in range(32)])[None, None]
    count = np.array([[32]], np.int32)
    vis = (rng.uniform(size=(1, 1, 32, 32)) > 0.5).astype(np.uint8)
    scale, rect, _ = A.draw(joints[0], count[0], vis[0], R.IMAGE_SIZE, hm, R.SIGMA, *A.seeded(7))
    ref = A.render(joints, count, vis, scale[None], rect[None], R.IMAGE_SIZE, hm, R.SIGMA)
    f32 = _render(gpu_device, joints, count, vis, scale[None], rect[None], hm)
    _assert_close(_planar(f32), ref, "P = J = 32")
    f16 = _render(gpu_device, joints, count, vis, scale[None], rect[None], hm, dtype=torch.float16)
    assert torch.equal(f16.t, f32.t.half())


def test_order_of_people_does_not_matter(gpu_device):
    hm, joints, count, vis, scale, rect, _ = _case(13, 17, True)
    first = _render(gpu_device, joints, count, vis, scale, rect, hm).t
    rng = np.random.default_rng(3)
    for _ in range(2):
        pj, pv, ps, pr = joints.copy(), vis.copy(), scale.copy(), rect.copy()
        for b in range(R.B):
            for v in range(R.V):
                n = int(count[b, v])
                perm = rng.permutation(n)
                pj[b, v, :n], pv[b, v, :n] = joints[b, v, perm], vis[b, v, perm]
                ps[b, v, :n], pr[b, v, :n] = scale[b, v, perm], rect[b, v, perm]
        assert torch.equal(_render(gpu_device, pj, count, pv, ps, pr, hm).t, first)


def test_guarded_output_is_fully_overwritten_and_nothing_else(gpu_device):
    from fvp import ops

    for J, dtype in ((15, torch.float32), (17, torch.float16)):
        hm, joints, count, vis, scale, rect, _ = _case(11, J, True)
        want = _render(gpu_device, joints, count, vis, scale, rect, hm, dtype=dtype).t
        guard = 4096
        buf = torch.full((want.numel() + 2 * guard,), float("nan"), dtype=dtype, device=gpu_device)
        out = buf[guard:guard + want.numel()].view(want.shape)
        ops.render_keypoints_aug_into(_dev(gpu_device, joints), _dev(gpu_device, count), _dev(gpu_device, vis),
                                      _dev(gpu_device, scale), _dev(gpu_device, rect), R.IMAGE_SIZE[0],
                                      R.IMAGE_SIZE[1], R.SIGMA, out)
        assert torch.equal(out, want) and not torch.isnan(out).any()
        assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + want.numel():]).all()


def test_hand_made_records(gpu_device):
    """Each held to render_aug_ref with identical support."""
    hm, joints, count, vis, _, _, _ = _case(12, 17, True)
    shape = (R.B, R.V, R.P, 17)
    plain = R.render(joints, count, vis, R.IMAGE_SIZE, hm, R.SIGMA)
    assert plain.any()

    def run(scale_value, rect_value, tol=TOL):
        scale = np.full(shape, scale_value, np.float32)
        rect = np.zeros(shape + (4,), np.int16)
        rect[...] = rect_value
        got = _planar(_render(gpu_device, joints, count, vis, scale, rect, hm))
        ref = A.render(joints, count, vis, scale, rect, R.IMAGE_SIZE, hm, R.SIGMA)
        _assert_close(got, ref, f"scale {scale_value} rect {rect_value}", tol)
        return got, ref

    # empty rectangles (r0 >= r1, c0 >= c1, negative ends pinned to 0): the scale alone
    for rc in ((5, 5, 0, 100), (0, 100, 7, 3), (9, 2, 9, 2), (-5, -1, 0, 100), (0, 100, -32768, 0)):
        got, ref = run(0.75, rc)
        assert np.array_equal(ref, (plain * np.float32(0.75)).astype(np.float32)) and got.any()
    # the whole patch (and more; a negative start is pinned to 0): nothing is painted
    for rc in ((0, 32767, 0, 32767), (-7, 200, -1, 200)):
        got, _ = run(0.9, rc)
        assert not got.any()
    # beyond the patch (the largest patch here is under 60 pixels): the scale alone
    got, ref = run(0.9, (100, 300, 0, 300))
    assert np.array_equal(ref != 0, plain != 0)
    got, ref = run(0.9, (0, 300, 100, 32767))
    assert np.array_equal(ref != 0, plain != 0)
    # the first rows of every patch: some of the support goes, not all
    got, ref = run(1.0, (0, 6, 0, 32767))
    assert 0 < np.count_nonzero(got) < np.count_nonzero(plain)
    # factors that paint nothing
    for s in (0.0, -0.0, -1.5, float("nan"), float("-inf")):
        got, _ = run(s, (0, 0, 0, 0))
        assert not got.any() and not np.isnan(got).any()
    # a factor of 50 clamps to exactly 1.0.  Below the clamp the value is 50 x the plain painter's, whose
    # fp32 error is <= 1.9e-7: 9.5e-6, plus one product rounding of 2^-24 on values <= 1
    got, ref = run(50.0, (0, 0, 0, 0), tol=9.6e-6)
    assert got.max() == 1.0 and np.count_nonzero(got == 1.0) > np.count_nonzero(plain == 1.0)
    sure = plain * np.float32(50.0) >= 1.0 + 1e-5
    assert sure.any() and (got[sure] == 1.0).all()
    got, _ = run(float("inf"), (0, 0, 0, 0))
    assert np.array_equal(got != 0, plain != 0) and (got[got != 0] == 1.0).all()


def test_guards(gpu_device):
    from fvp import _lib
    from fvp.heatmaps import Augmentation, render_keypoints

    kw = dict(image_size=R.IMAGE_SIZE, heatmap_size=(48, 32), sigma=R.SIGMA)
    joints = torch.zeros((1, 2, 3, 17, 2), dtype=torch.float64, device=gpu_device)
    count = torch.ones((1, 2), dtype=torch.int32, device=gpu_device)
    scale, rect = (torch.from_numpy(a) for a in A.identity((1, 2, 3, 17)))
    assert render_keypoints(joints, count, augment=Augmentation(scale, rect), **kw).shape == (1, 2, 17, 32, 48)
    assert render_keypoints(joints, count, augment=(scale.to(gpu_device), rect.to(gpu_device)), **kw).t.dtype \
        == torch.float32
    for bad in ((scale[..., :16], rect), (scale, rect[..., :2]), (scale.half(), rect), (scale, rect.int()), scale):
        with pytest.raises(_lib.FvpError, match="augment"):
            render_keypoints(joints, count, augment=bad, **kw)
    with pytest.raises(_lib.FvpError, match="requires grad"):
        render_keypoints(joints.clone().requires_grad_(True), count, augment=(scale, rect), **kw)
