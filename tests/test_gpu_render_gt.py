"""GPU tests of the 'gt' heatmap source (fvp.heatmaps.render_poses3d / project_poses;
fvp_render_poses3d, fvp_render_poses3d_f16, fvp_project_poses): 3-D poses ->
2-D keypoints, visibility flags and channels-last input heatmaps in one launch,
against the reference's recorded values (tests/golden/render_gt.npz) and the
numpy restatement (tests/render_gt_ref.py).

The 2-D keypoints are float64 and compared bit for bit; the flags are compared
exactly.  Heatmaps: support identical and values within 1e-6, the bound of
tests/test_gpu_render.py for its stated reason (<= 3 fp32 roundings of the
exponent's argument plus 1-2 ulp of expf on values in [0, 1])."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import render_gt_ref as G

pytestmark = pytest.mark.gpu
TOL = 1e-6
SHAPES = [(48, 32), (50, 37)]  # heatmap (W, H): the renderer's two tile-odd shapes


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)  # (copies: the shared cases are read-only)


def _operands(dev, c, cams=None, cam_index=None):
    cams = c["cams"] if cams is None else cams
    return (_dev(c["joints3d"], dev), _dev(c["vis3d"], dev), _dev(c["count"], dev), _dev(cams, dev),
            _dev(c["resize_t"], dev)), dict(ori_image_size=c["ori_image_size"], image_size=c["image_size"],
                                           cam_index=cam_index)


def _render(dev, c, dtype=None, return_keypoints=False, **kw):
    from fvp.heatmaps import render_poses3d

    args, sizes = _operands(dev, c, **kw)
    return render_poses3d(*args, heatmap_size=c["heatmap_size"], sigma=c["sigma"], dtype=dtype,
                          return_keypoints=return_keypoints, **sizes)


def _project(dev, c, **kw):
    from fvp.heatmaps import project_poses

    args, sizes = _operands(dev, c, **kw)
    return project_poses(*args, **sizes)


def _planar(cl):
    """The J joint planes [B, V, J, H, W] of a channels-last result, after checking its padding."""
    t = cl.t.float().cpu()
    assert t.shape[4] == 16 * ((cl.J + 15) // 16)
    assert not t[..., cl.J:].any(), "padding channels must be exactly zero"
    return t[..., :cl.J].permute(0, 1, 4, 2, 3).contiguous().numpy()


def _assert_close(got, ref, what):
    assert got.shape == ref.shape
    diff = np.count_nonzero((got != 0) != (ref != 0))
    assert diff == 0, f"{what}: support differs at {diff} elements"
    err = float(np.abs(got - ref).max())
    print(f"{what}: max abs error {err:.3g} over {np.count_nonzero(ref)} painted values")
    assert err <= TOL, f"{what}: max abs error {err}"


def _assert_keypoints(j2, v2, ref_j2, ref_v2, count, what):
    """Bit for bit below count; zeros at and beyond it (what the kernels write there)."""
    j2, v2 = j2.cpu().numpy(), v2.cpu().numpy()
    assert j2.dtype == np.float64 and v2.dtype == np.uint8 and j2.shape == ref_j2.shape
    for b in range(j2.shape[0]):
        n = int(count[b])
        want = np.ascontiguousarray(ref_j2[b, :, :n])
        differ = np.count_nonzero(np.ascontiguousarray(j2[b, :, :n]).view(np.uint64) != want.view(np.uint64))
        assert differ == 0, f"{what}: {differ} coordinates of frame {b} differ in their bits"
        assert np.array_equal(v2[b, :, :n], ref_v2[b, :, :n]), f"{what}: flags of frame {b}"
        assert not j2[b, :, n:].any() and not v2[b, :, n:].any(), f"{what}: rows at or beyond count"


def _with_reference(c):
    c["ref_j2"], c["ref_v2"] = G.project_batch(c["joints3d"], c["vis3d"], c["count"], c["cams"][None], None,
                                               c["resize_t"], c["ori_image_size"], c["image_size"])
    c["ref"] = G.render_batch(c["ref_j2"], c["ref_v2"], c["count"], c["image_size"], c["heatmap_size"], c["sigma"])
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _case(seed, name, J):
    """A random case and its restatement, computed once and shared read-only; odd seeds zoom, so that the
    resized-image test fires too."""
    joints3d, vis3d, count = G.make_poses(seed, name, J)
    zoom = 1.5 if seed % 2 else 1.0
    return _with_reference(dict(J=J, joints3d=joints3d, vis3d=vis3d, count=count, cams=np.array(G.cameras64(name)),
                                resize_t=G.resize_transform(name, zoom), ori_image_size=G.CALIBRATIONS[name][1],
                                image_size=G.IMAGE_SIZE, heatmap_size=SHAPES[seed % 2], sigma=G.SIGMA))


@pytest.mark.parametrize("case", range(4))
def test_golden_parity(gpu_device, case):
    c = G.golden_cases()[case]
    cl, j2, v2 = _render(gpu_device, c, return_keypoints=True)
    assert cl.shape == c["heatmaps"].shape
    _assert_keypoints(j2, v2, c["joints2d"], c["vis2d"], c["count"], f"golden case {case}")
    _assert_close(_planar(cl), c["heatmaps"], f"golden case {case}")
    pj2, pv2 = _project(gpu_device, c)
    assert torch.equal(pj2, j2) and torch.equal(pv2, v2)


@pytest.mark.parametrize("seed", [21, 22])
@pytest.mark.parametrize("name", ["shelf", "panoptic"])
@pytest.mark.parametrize("J", [15, 17])
def test_random_parity_and_one_launch_equals_two(gpu_device, J, name, seed):
    from fvp.heatmaps import render_keypoints

    c = _case(seed, name, J)
    what = f"J={J} {name} seed={seed}"
    j2, v2 = _project(gpu_device, c)
    _assert_keypoints(j2, v2, c["ref_j2"], c["ref_v2"], c["count"], what)
    assert 0 < int(v2.sum()) < v2.numel()
    count_bv = _dev(c["count"], gpu_device)[:, None].expand(-1, j2.shape[1]).contiguous()
    kw = dict(image_size=c["image_size"], heatmap_size=c["heatmap_size"], sigma=c["sigma"])
    for dtype in (torch.float32, torch.float16):
        cl, rj2, rv2 = _render(gpu_device, c, dtype=dtype, return_keypoints=True)
        assert cl.dtype == dtype and cl.cp == (16 if J == 15 else 32)
        assert torch.equal(rj2, j2) and torch.equal(rv2, v2)
        two = render_keypoints(j2, count_bv, v2, dtype=dtype, **kw)
        assert torch.equal(cl.t, two.t), f"{what} {dtype}: one launch differs from project + render"
        assert torch.equal(_render(gpu_device, c, dtype=dtype).t, cl.t)  # without the keypoint outputs
    f32 = _render(gpu_device, c)
    assert torch.equal(_render(gpu_device, c, dtype=torch.float16).t, f32.t.half())
    _assert_close(_planar(f32), c["ref"], what)


def test_largest_frame(gpu_device):
    """P = 32 people of J = 32 joints through the 5 Shelf cameras: the largest record table a block builds."""
    rng = np.random.default_rng(7)
    _, ori, size, centre = G.CALIBRATIONS["shelf"]
    joints3d = (np.asarray(centre) + rng.uniform(-0.3, 0.3, (1, 32, 1, 3)) * np.asarray(size)
                + rng.normal(size=(1, 32, 32, 3)) * (250.0, 250.0, 450.0))
    c = _with_reference(dict(J=32, joints3d=joints3d, vis3d=(rng.uniform(size=(1, 32, 32)) > 0.3).astype(np.uint8),
                             count=np.array([32], np.int32), cams=np.array(G.cameras64("shelf")),
                             resize_t=G.resize_transform("shelf"), ori_image_size=ori, image_size=G.IMAGE_SIZE,
                             heatmap_size=(50, 37), sigma=G.SIGMA))
    cl, j2, v2 = _render(gpu_device, c, return_keypoints=True)
    _assert_keypoints(j2, v2, c["ref_j2"], c["ref_v2"], c["count"], "P = J = 32")
    assert int(v2.sum()) > 500
    _assert_close(_planar(cl), c["ref"], "P = J = 32")


def test_cam_index_mixes_sequences(gpu_device):
    """Frames of two calibrations in one batch equal the two single-sequence calls."""
    c = dict(_case(22, "shelf", 17))
    sets = np.stack([G.cameras64("shelf"), G.cameras64("panoptic")])
    one = {name: _render(gpu_device, c, cams=np.array(G.cameras64(name)), return_keypoints=True)
           for name in ("shelf", "panoptic")}
    assert not torch.equal(one["shelf"][0].t, one["panoptic"][0].t)
    for index in ([0, 1], [1, 0], [1, 1]):
        for cam_index in (index, torch.tensor(index, dtype=torch.int32),
                          torch.tensor(index, dtype=torch.int32, device=gpu_device)):  # list, host and device tensor
            cl, j2, v2 = _render(gpu_device, c, cams=sets, cam_index=cam_index, return_keypoints=True)
            for b, s in enumerate(index):
                want = one[("shelf", "panoptic")[s]]
                assert torch.equal(cl.t[b], want[0].t[b]) and torch.equal(j2[b], want[1][b])
                assert torch.equal(v2[b], want[2][b])
    pj2, pv2 = _project(gpu_device, c, cams=sets, cam_index=[1, 0])
    assert torch.equal(pj2[0], one["panoptic"][1][0]) and torch.equal(pv2[1], one["shelf"][2][1])


def test_empty_frame_and_padded_rows(gpu_device):
    c = dict(_case(21, "panoptic", 15))
    full = _render(gpu_device, c).t
    assert full[0].any() and full[1].any()
    c["count"] = np.array([0, int(c["count"][1])], np.int32)
    cl, j2, v2 = _render(gpu_device, c, return_keypoints=True)
    assert not cl.t[0].any() and not j2[0].any() and not v2[0].any()  # a frame of zeros
    assert torch.equal(cl.t[1], full[1])
    # count < P: NaN in the padded rows (as make_poses leaves them) changes nothing
    c = dict(_case(21, "panoptic", 15))
    assert np.isnan(c["joints3d"][1]).any()
    padded = np.isnan(c["joints3d"][..., 0])
    clean = dict(c, joints3d=np.nan_to_num(c["joints3d"], nan=77.0),
                 vis3d=np.where(padded, 1, c["vis3d"]).astype(np.uint8))  # (the padded rows' flags set, too)
    a, aj, av = _render(gpu_device, c, return_keypoints=True)
    b, bj, bv = _render(gpu_device, clean, return_keypoints=True)
    assert torch.equal(a.t, b.t) and torch.equal(aj, bj) and torch.equal(av, bv)


def test_person_with_non_finite_joint_is_skipped(gpu_device):
    c = dict(_case(22, "shelf", 15))
    bad = np.array(c["joints3d"])
    bad[0, 1, 3, 0] = np.nan
    bad[1, 0, 0, 2] = np.inf
    got = _render(gpu_device, dict(c, joints3d=bad))
    # the same frames without those people (moved out by shortening the lists)
    less, vis, cnt = np.array(c["joints3d"]), np.array(c["vis3d"]), np.array(c["count"])
    less[0, 1:4], vis[0, 1:4] = c["joints3d"][0, 2:5], c["vis3d"][0, 2:5]
    less[1, 0:2], vis[1, 0:2] = c["joints3d"][1, 1:3], c["vis3d"][1, 1:3]
    cnt -= 1
    want = _render(gpu_device, dict(c, joints3d=less, vis3d=vis, count=cnt))
    assert torch.equal(got.t, want.t)
    assert c["ref_v2"][0, :, 1].any() and c["ref_v2"][1, :, 0].any()  # (both skipped people would have painted)


def test_order_of_people_does_not_matter(gpu_device):
    c = dict(_case(21, "shelf", 17))
    first = _render(gpu_device, c).t
    rng = np.random.default_rng(3)
    for _ in range(2):
        pj, pv = np.array(c["joints3d"]), np.array(c["vis3d"])
        for b in range(G.B):
            n = int(c["count"][b])
            perm = rng.permutation(n)
            pj[b, :n], pv[b, :n] = c["joints3d"][b, perm], c["vis3d"][b, perm]
        assert torch.equal(_render(gpu_device, dict(c, joints3d=pj, vis3d=pv)).t, first)


def _guarded(shape, dtype, fill, dev, guard=64):
    """A tensor of `shape` inside a buffer pre-filled with `fill`, `guard` elements on both sides."""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * guard,), fill, dtype=dtype, device=dev)
    return flat, flat[guard:guard + n].view(shape)


def _guards_intact(flat, fill, guard=64):
    ends = torch.cat([flat[:guard], flat[-guard:]])
    return bool(torch.isnan(ends).all()) if fill != fill else bool((ends == fill).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_prefilled_guarded_outputs_are_fully_overwritten(gpu_device, dtype):
    """Through render_poses3d_into and the C entry points: every element inside is overwritten --
    rows at or beyond count with 0, which is what the kernels write there -- and no guard word is touched."""
    from fvp import _lib, ops

    c = _case(21, "shelf", 17)
    nan = float("nan")
    want, wj2, wv2 = _render(gpu_device, c, dtype=dtype, return_keypoints=True)
    assert int(c["count"][1]) < G.P  # frame 1 has rows at and beyond count
    (j3, v3, cnt, cams, t), _ = _operands(gpu_device, c)
    cams = cams.unsqueeze(0)
    ori, img = c["ori_image_size"], c["image_size"]

    def buffers():
        return (_guarded(want.t.shape, dtype, nan, gpu_device), _guarded(wj2.shape, torch.float64, nan, gpu_device),
                _guarded(wv2.shape, torch.uint8, 0xFF, gpu_device))

    def check(*written):
        for (flat, view), fill, ref in zip(written, (nan, nan, 0xFF), (want.t, wj2, wv2)):
            assert _guards_intact(flat, fill) and torch.equal(view, ref)

    out, j2, v2 = buffers()
    ops.render_poses3d_into(j3, v3, cnt, cams, None, t, ori[0], ori[1], img[0], img[1], c["sigma"], out[1], j2[1],
                            v2[1])
    check(out, j2, v2)
    assert not torch.isnan(out[1]).any() and not torch.isnan(j2[1]).any() and not (v2[1] == 0xFF).any()
    assert not j2[1][1, :, int(c["count"][1]):].any() and not v2[1][1, :, int(c["count"][1]):].any()

    out, j2, v2 = buffers()  # the optional outputs left out: they stay untouched
    ops.render_poses3d_into(j3, v3, cnt, cams, None, t, ori[0], ori[1], img[0], img[1], c["sigma"], out[1])
    check(out)
    assert torch.isnan(j2[0]).all() and (v2[0] == 0xFF).all()

    out, j2, v2 = buffers()  # the C entry points
    B, P, J = j3.shape[:3]
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    name = "fvp_render_poses3d_f16" if dtype == torch.float16 else "fvp_render_poses3d"
    _lib.call(name, j3.data_ptr(), v3.data_ptr(), cnt.data_ptr(), B, P, J, cams.data_ptr(), None, 1, cams.shape[1],
              t.data_ptr(), float(ori[0]), float(ori[1]), float(img[0]), float(img[1]), want.t.shape[2],
              want.t.shape[3], c["sigma"], want.t.shape[4], out[1].data_ptr(), j2[1].data_ptr(), v2[1].data_ptr(),
              stream)
    check(out, j2, v2)
    out, j2, v2 = buffers()
    _lib.call("fvp_project_poses", j3.data_ptr(), v3.data_ptr(), cnt.data_ptr(), B, P, J, cams.data_ptr(), None, 1,
              cams.shape[1], t.data_ptr(), float(ori[0]), float(ori[1]), float(img[0]), float(img[1]),
              j2[1].data_ptr(), v2[1].data_ptr(), stream)
    for (flat, view), fill, ref in ((j2, nan, wj2), (v2, 0xFF, wv2)):
        assert _guards_intact(flat, fill) and torch.equal(view, ref)
    assert torch.isnan(out[0]).all()


def test_consumer_reads_the_render_in_place(gpu_device):
    """ProjectLayer.forward_fused fed the ChannelsLastHeatmaps == fed the same values as a plain planar tensor."""
    from fvp import geometry
    from fvp.heatmaps import channels_last_of, render_poses3d
    from fvp.project_whole import ProjectLayer
    from fvp.workloads import WORKLOADS

    w = dataclasses.replace(WORKLOADS["shelf_native"], heatmap_size=(50, 37), voxels_per_axis=(24, 16, 5),
                            space_size=(2000.0, 2000.0, 2000.0))
    rng = np.random.default_rng(21)
    B = 2
    joints3d = (np.asarray(w.space_center) + rng.uniform(-0.3, 0.3, (B, 3, 1, 3)) * np.asarray(w.space_size)
                + rng.normal(size=(B, 3, w.num_joints, 3)) * 200.0)
    cams, seq = w.cameras()
    rt = geometry.resize_transform(w.ori_image_size, w.image_size)
    cl = render_poses3d(_dev(joints3d, gpu_device), None, torch.full((B,), 3, dtype=torch.int32, device=gpu_device),
                        _dev(geometry.pack_cameras64(cams, seq), gpu_device), _dev(rt, gpu_device),
                        ori_image_size=w.ori_image_size, image_size=w.image_size, heatmap_size=w.heatmap_size,
                        sigma=G.SIGMA)
    planar = cl.planar()
    assert channels_last_of(planar) is cl and planar.any()
    plain = planar.clone()
    assert channels_last_of(plain) is None
    layer = ProjectLayer(w.cfg(str(gpu_device)))
    layer.verbose = False
    meta, rt32 = {"seq": [seq] * B}, torch.as_tensor(rt, dtype=torch.float).to(gpu_device)
    cube_ref, xy_ref = layer.forward_fused(plain, meta, cams, rt32)
    assert cube_ref.any()
    cube, xy = layer.forward_fused(cl, meta, cams, rt32)
    assert torch.equal(cube, cube_ref) and torch.equal(xy, xy_ref)


def test_guards(gpu_device):
    from fvp import _lib
    from fvp.heatmaps import project_poses, render_poses3d

    kw = dict(ori_image_size=(1032, 776), image_size=G.IMAGE_SIZE)
    rkw = dict(heatmap_size=(48, 32), sigma=G.SIGMA, **kw)
    j = torch.zeros((2, 3, 17, 3), dtype=torch.float64, device=gpu_device)
    v = torch.ones((2, 3, 17), dtype=torch.bool, device=gpu_device)
    c = torch.ones((2,), dtype=torch.int32, device=gpu_device)
    cams = _dev(G.cameras64("shelf"), gpu_device)
    t = _dev(G.resize_transform("shelf"), gpu_device)
    with pytest.raises(_lib.FvpError, match="requires grad"):
        render_poses3d(j.clone().requires_grad_(True), v, c, cams, t, **rkw)
    with pytest.raises(_lib.FvpError, match="requires grad"):
        project_poses(j.clone().requires_grad_(True), v, c, cams, t, **kw)
    with pytest.raises(_lib.FvpError, match="HIP device"):
        render_poses3d(j.cpu(), v.cpu(), c.cpu(), cams.cpu(), t.cpu(), **rkw)
    with pytest.raises(_lib.FvpError, match="HIP device"):
        render_poses3d(j, v, c.cpu(), cams, t, **rkw)
    with pytest.raises(_lib.FvpError, match="HIP device"):
        project_poses(j, v, c, cams.cpu(), t, **kw)
    with pytest.raises(_lib.FvpError, match="contiguous"):
        render_poses3d(torch.zeros((2, 3, 17, 4), dtype=torch.float64, device=gpu_device)[..., :3], v, c, cams, t,
                       **rkw)
    with pytest.raises(_lib.FvpError, match="contiguous"):
        project_poses(j, v, c, torch.cat([cams, cams], dim=1)[:, :24], t, **kw)
    for index in ([0, 1], [-1, 0], torch.tensor([0, 5], dtype=torch.int32)):
        with pytest.raises(_lib.FvpError, match="cam_index"):
            render_poses3d(j, v, c, cams, t, cam_index=index, **rkw)
    cl, j2, v2 = render_poses3d(j, v, c, cams, t, return_keypoints=True, **rkw)  # bool flags are taken as they are
    assert cl.shape == (2, 5, 17, 32, 48) and tuple(j2.shape) == (2, 5, 3, 17, 2) and tuple(v2.shape) == (2, 5, 3, 17)
    out = torch.ops.fvp.render_poses3d(j.to("meta"), None, c.to("meta"), cams.unsqueeze(0).to("meta"), None,
                                       t.to("meta"), 1032.0, 776.0, 192.0, 128.0, 32, 48, 3.0, False)
    assert tuple(out[0].shape) == (2, 5, 32, 48, 32) and out[0].dtype == torch.float32
