"""GPU tests of fvp_render_keypoints (fvp.heatmaps.render_keypoints): 2-D
keypoints -> channels-last input heatmaps in one launch, against the
reference's recorded heatmaps (tests/golden/render_kp.npz) and the numpy
restatement (tests/render_ref.py).

Tolerance 1e-6 absolute on values in [0, 1], support (the non-zero set)
identical: the argument a = d^2 * inv carries at most ~3 fp32 roundings, so
|delta e^-a| <= a e^-a * 3 * 2^-24 <= 0.37 * 1.8e-7, plus 1-2 ulp of expf near 1
(<= 1.2e-7); the smallest painted value is ~1e-5, so nothing underflows."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import render_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-6
SHAPES = [(48, 32), (50, 37)]  # heatmap (W, H): neither is a multiple of the 32 x 16 tile in both axes


def _render(dev, joints, count, vis, heatmap_size, dtype=torch.float64, image_size=R.IMAGE_SIZE, sigma=R.SIGMA):
    from fvp.heatmaps import render_keypoints

    j = torch.from_numpy(np.array(joints)).to(dtype).to(dev)  # (copies: the shared cases are read-only)
    c = torch.from_numpy(np.array(count)).to(dev)
    v = None if vis is None else torch.from_numpy(np.array(vis)).to(dev)
    return render_keypoints(j, c, v, image_size=image_size, heatmap_size=heatmap_size, sigma=sigma)


def _planar(cl):
    """The J joint planes [B, V, J, H, W] of a channels-last result, after checking its padding."""
    t = cl.t.cpu()
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


@functools.lru_cache(maxsize=None)
def _case(seed, J, with_vis, f32):
    hm = SHAPES[seed % 2]
    joints, count = R.make_people(seed, J, hm)
    if f32:
        joints = joints.astype(np.float32).astype(np.float64)  # what the kernel widens
    vis = R.make_vis(seed, J) if with_vis else None
    ref = R.render(joints, count, vis, R.IMAGE_SIZE, hm, R.SIGMA)
    for a in (joints, count, ref):
        a.setflags(write=False)
    return hm, joints, count, vis, ref


@pytest.mark.parametrize("case", range(4))
def test_golden_parity(gpu_device, case):
    c = R.golden_cases()[case]
    cl = _render(gpu_device, c["joints"], c["count"], c["vis"], c["heatmap_size"], torch.float64, c["image_size"],
                 c["sigma"])
    assert cl.shape == c["heatmaps"].shape
    _assert_close(_planar(cl), c["heatmaps"], f"golden case {case}")


@pytest.mark.parametrize("seed", [11, 12, 13])
@pytest.mark.parametrize("with_vis", [False, True], ids=["all-visible", "vis"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("J", [15, 17])
def test_random_parity(gpu_device, J, f32, with_vis, seed):
    hm, joints, count, vis, ref = _case(seed, J, with_vis, f32)
    cl = _render(gpu_device, joints, count, vis, hm, torch.float32 if f32 else torch.float64)
    assert cl.cp == (16 if J == 15 else 32)
    _assert_close(_planar(cl), ref, f"J={J} f32={f32} vis={with_vis} seed={seed}")


def test_largest_view(gpu_device):
    """P = 32 people of J = 32 joints: the largest record table a block builds."""
    rng = np.random.default_rng(7)
    hm = (50, 37)
    stride = np.asarray(R.IMAGE_SIZE, np.float64) / np.asarray(hm, np.float64)
    joints = np.stack([R._person(rng, 32, (rng.uniform(-4, 54), rng.uniform(-4, 41)), rng.uniform(2, 60), stride)
                       for _ in range(32)])[None, None]
    count = np.array([[32]], np.int32)
    vis = (rng.uniform(size=(1, 1, 32, 32)) > 0.5).astype(np.uint8)
    ref = R.render(joints, count, vis, R.IMAGE_SIZE, hm, R.SIGMA)
    _assert_close(_planar(_render(gpu_device, joints, count, vis, hm)), ref, "P = J = 32")


def test_empty_view_and_padded_rows(gpu_device):
    hm, joints, count, _, ref = _case(11, 17, False, False)
    count0 = count.copy()
    count0[1, 0] = 0
    got = _planar(_render(gpu_device, joints, count0, None, hm))
    assert not got[1, 0].any()
    for b, v in ((0, 0), (0, 1), (1, 1)):
        assert np.array_equal(got[b, v] != 0, ref[b, v] != 0)
    # count < P: NaN in the padded rows (as make_people leaves them) changes nothing
    assert np.isnan(joints[1]).any()
    clean = np.nan_to_num(joints, nan=77.0)
    a = _render(gpu_device, joints, count, None, hm).t
    b = _render(gpu_device, clean, count, None, hm).t
    assert torch.equal(a, b)


def test_person_with_nan_joint_is_skipped(gpu_device):
    hm, joints, count, _, _ = _case(12, 15, False, False)
    bad = joints.copy()
    bad[0, 0, 1, 3, 0] = np.nan
    bad[0, 1, 2, 0, 1] = np.inf
    got = _planar(_render(gpu_device, bad, count, None, hm))
    # the same views without those people (moved out by shortening the lists)
    less = joints.copy()
    cnt = count.copy()
    less[0, 0, 1:4] = joints[0, 0, 2:5]
    less[0, 1, 2:4] = joints[0, 1, 3:5]
    cnt[0, 0] -= 1
    cnt[0, 1] -= 1
    ref = R.render(less, cnt, None, R.IMAGE_SIZE, hm, R.SIGMA)
    assert np.array_equal(R.render(bad, count, None, R.IMAGE_SIZE, hm, R.SIGMA), ref)
    _assert_close(got, ref, "non-finite people skipped")
    assert np.array_equal(got, _planar(_render(gpu_device, less, cnt, None, hm)))


def test_order_of_people_does_not_matter(gpu_device):
    hm, joints, count, vis, _ = _case(13, 17, True, False)
    first = _render(gpu_device, joints, count, vis, hm).t
    rng = np.random.default_rng(3)
    for _ in range(2):
        pj, pv = joints.copy(), vis.copy()
        for b in range(R.B):
            for v in range(R.V):
                n = int(count[b, v])
                perm = rng.permutation(n)
                pj[b, v, :n], pv[b, v, :n] = joints[b, v, perm], vis[b, v, perm]
        assert torch.equal(_render(gpu_device, pj, count, pv, hm).t, first)


def test_prefilled_output_is_fully_overwritten(gpu_device):
    from fvp import ops

    hm, joints, count, _, _ = _case(11, 15, False, False)
    want = _render(gpu_device, joints, count, None, hm).t
    j = torch.from_numpy(np.array(joints)).to(gpu_device)
    c = torch.from_numpy(np.array(count)).to(gpu_device)
    for fill in (float("nan"), 3.5):
        out = torch.full_like(want, fill)
        ops.render_keypoints_into(j, c, None, R.IMAGE_SIZE[0], R.IMAGE_SIZE[1], R.SIGMA, out)
        assert torch.equal(out, want)


def _shelf_people(w, B, P, seed):
    rng = np.random.default_rng(seed)
    W, H = w.heatmap_size
    stride = np.asarray(w.image_size, np.float64) / np.asarray(w.heatmap_size, np.float64)
    V = len(w.cameras()[0][w.cameras()[1]])
    joints = np.stack([R._person(rng, w.num_joints, (rng.uniform(0, W), rng.uniform(0, H)), rng.uniform(4, 40), stride)
                       for _ in range(B * V * P)]).reshape(B, V, P, w.num_joints, 2)
    count = rng.integers(1, P + 1, size=(B, V)).astype(np.int32)
    return joints, count


def test_consumers_read_the_render_in_place(gpu_device):
    """ProjectLayer (whole space and per person) fed the ChannelsLastHeatmaps == fed the same
    values as a plain planar tensor (which goes through the layout pass), bit for bit."""
    from fvp import geometry
    from fvp.heatmaps import channels_last_of
    from fvp.project_individual import ProjectLayer as PersonLayer
    from fvp.project_whole import ProjectLayer
    from fvp.workloads import WORKLOADS

    w = dataclasses.replace(WORKLOADS["shelf_native"], heatmap_size=(50, 37), voxels_per_axis=(24, 16, 5),
                            space_size=(2000.0, 2000.0, 2000.0), ind_space_size=(2000.0, 2000.0, 2000.0),
                            ind_voxels_per_axis=(16, 16, 16))
    B = 2
    joints, count = _shelf_people(w, B, 3, 21)
    cl = _render(gpu_device, joints, count, None, w.heatmap_size, image_size=w.image_size)
    ref = R.render(joints, count, None, w.image_size, w.heatmap_size, R.SIGMA)
    planar = cl.planar()
    assert channels_last_of(planar) is cl  # the mark travels through tensor-typed interfaces
    _assert_close(planar.cpu().numpy(), ref, "cl.planar()")
    plain = planar.clone()
    assert channels_last_of(plain) is None

    cams, seq = w.cameras()
    rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float).to(gpu_device)
    meta = {"seq": [seq] * B}
    layer = ProjectLayer(w.cfg(str(gpu_device)))
    layer.verbose = False
    cube_ref, xy_ref = layer.forward_fused(plain, meta, cams, rt)
    assert cube_ref.any()
    for src in (cl, planar):
        cube, xy = layer.forward_fused(src, meta, cams, rt)
        assert torch.equal(cube, cube_ref) and torch.equal(xy, xy_ref)

    person = PersonLayer(w.cfg(str(gpu_device)))
    person.verbose = False
    c = w.space_center
    props = torch.tensor([[c[0], c[1], c[2], 0, 0.9, 0.5, 0.5], [c[0] + 300, c[1] - 200, c[2] - 100, 0, 0.8, 0.2, 0.9]],
                         dtype=torch.float32, device=gpu_device)
    cubes_ref, off_ref = person(plain, 1, meta, props, cams, rt)
    for src in (cl, planar):
        cubes, off = person(src, 1, meta, props, cams, rt)
        assert torch.equal(cubes, cubes_ref) and torch.equal(off, off_ref)


def test_guards(gpu_device):
    from fvp import _lib
    from fvp.heatmaps import render_keypoints

    kw = dict(image_size=R.IMAGE_SIZE, heatmap_size=(48, 32), sigma=R.SIGMA)
    joints = torch.zeros((1, 2, 3, 17, 2), dtype=torch.float64, device=gpu_device)
    count = torch.ones((1, 2), dtype=torch.int32, device=gpu_device)
    with pytest.raises(_lib.FvpError, match="requires grad"):
        render_keypoints(joints.clone().requires_grad_(True), count, **kw)
    with pytest.raises(_lib.FvpError, match="HIP device"):
        render_keypoints(joints.cpu(), count.cpu(), **kw)
    with pytest.raises(_lib.FvpError, match="HIP device"):
        render_keypoints(joints, count.cpu(), **kw)
    with pytest.raises(_lib.FvpError, match="contiguous"):
        render_keypoints(torch.zeros((1, 2, 3, 17, 4), dtype=torch.float64, device=gpu_device)[..., :2], count, **kw)
    out = torch.ops.fvp.render_keypoints(joints.to("meta"), count.to("meta"), None, 192.0, 128.0, 32, 48, 3.0)
    assert tuple(out.shape) == (1, 2, 32, 48, 32) and out.dtype == torch.float32
    assert render_keypoints(joints, count, **kw).shape == (1, 2, 17, 32, 48)
