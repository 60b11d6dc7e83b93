"""CPU tests of the 'gt' heatmap source's host side: the numpy restatement
(tests/render_gt_ref.py) against the reference's recorded 2-D keypoints, flags
and heatmaps (tests/golden/render_gt.npz, tools/gen_render_gt_golden.py), the
coverage of the cases, the new C-ABI entries' argument checks, pack_poses3d,
pack_cameras64 and the ops' fake kernels."""
import os

import numpy as np
import pytest
import torch

import render_gt_ref as G
from conftest import GOLDEN

NULL, SHAPE = 1001, 1002


def test_golden_file_is_small_and_holds_the_cases():
    assert os.path.getsize(os.path.join(GOLDEN, "render_gt.npz")) < (1 << 20)
    cases = G.golden_cases()
    assert [(c["calibration"], c["J"], c["heatmap_size"], c["zoom"]) for c in cases] == [x[:4] for x in G.CASES]
    assert {c["ori_image_size"] for c in cases} == {(1032, 776), (1920, 1080)}
    for i, c in enumerate(cases):
        built = G.built_case(i)  # the fixture holds what the case builders build
        for key in ("joints3d", "vis3d", "count", "cams", "resize_t"):
            assert np.array_equal(c[key], built[key], equal_nan=True), key
        assert c["joints3d"].shape == (G.B, G.P, c["J"], 3) and c["cams"].shape == (5, G.CAM_STRIDE)
        assert c["count"].tolist() == [G.P, G.P - 2] and np.isnan(c["joints3d"][1, G.P - 2:]).all()  # padded rows
        assert c["image_size"] == G.IMAGE_SIZE and c["sigma"] == G.SIGMA
    assert not cases[0]["cams"][:, 16:21].any() and cases[1]["cams"][:, 16:21].all()  # no distortion / k and p


@pytest.mark.parametrize("case", range(4))
def test_cases_cover_every_visibility_outcome(case):
    c = G.golden_cases()[case]
    cov = G.coverage(c["joints3d"], c["vis3d"], c["count"], c["cams"], c["resize_t"], c["ori_image_size"],
                     c["image_size"])
    print(f"case {case}: {cov}")
    for side in ("left", "right", "top", "bottom"):  # each side of the original-image test
        assert cov[side] >= 1, side
    assert cov["behind"] >= 1 and cov["only_vis3d"] >= 1
    assert 0.2 <= cov["visible"] / cov["live"] <= 0.8
    second = [cov["second_neg"], cov["second_right"], cov["second_below"]]
    if c["zoom"] == 1.0:  # the letterbox transform keeps what the first test passed
        assert second == [0, 0, 0]
    else:
        assert min(second) >= 1
    for b in range(G.B):  # a live person with joints_3d_vis == 0 on some joints, not on all
        n = int(c["count"][b])
        assert any(0 < np.count_nonzero(c["vis3d"][b, p] == 0) < c["J"] for p in range(n))


@pytest.mark.parametrize("case", range(4))
def test_projection_restatement_equals_the_reference_bit_for_bit(case):
    """The fma chain of the 3x3 matmul and the 2x3 dot is the order numpy's BLAS used on the
    machine that wrote the fixture: any other order shows here, as differing bytes."""
    c = G.golden_cases()[case]
    j2, v2 = G.project_batch(c["joints3d"], c["vis3d"], c["count"], c["cams"][None], None, c["resize_t"],
                             c["ori_image_size"], c["image_size"])
    assert j2.dtype == np.float64 and c["joints2d"].dtype == np.float64
    for b in range(G.B):
        n = int(c["count"][b])
        assert np.isfinite(c["joints2d"][b, :, :n]).all()
        assert j2[b, :, :n].tobytes() == c["joints2d"][b, :, :n].tobytes()
        assert not j2[b, :, n:].any() and not v2[b, :, n:].any()
    assert np.array_equal(v2, c["vis2d"])


@pytest.mark.parametrize("case", range(4))
def test_painted_restatement_matches_the_reference(case):
    """Support identical, values within 1e-6 (fp32 argument and expf against the reference's fp64:
    the bound of test_render_golden.py)."""
    c = G.golden_cases()[case]
    j2, v2 = G.project_batch(c["joints3d"], c["vis3d"], c["count"], c["cams"][None], None, c["resize_t"],
                             c["ori_image_size"], c["image_size"])
    got = G.render_batch(j2, v2, c["count"], c["image_size"], c["heatmap_size"], c["sigma"])
    ref = c["heatmaps"]
    assert got.shape == ref.shape and got.dtype == np.float32 and ref.any()
    assert np.array_equal(got != 0, ref != 0)
    err = float(np.abs(got - ref).max())
    print(f"render_gt_ref vs reference, case {case}: max abs error {err:.3g}")
    assert err <= 1e-6


def test_fma_is_exact():
    a, b = np.float64(1 + 2.0 ** -30), np.float64(1 - 2.0 ** -30)
    assert a * b == 1.0 and G.fma(a, b, -1.0) == -(2.0 ** -60)  # the product's low part survives
    assert G.fma(0.1, 10.0, -1.0) == 2.0 ** -54
    assert np.isnan(G.fma(np.nan, 1.0, 1.0)) and G.fma(np.inf, 1.0, 1.0) == np.inf


# -- the C entry points' host refusals ----------------------------------------------------------
def _project_args(**kw):
    a = dict(joints3d=1, vis3d=None, count=1, B=2, P=5, J=17, cams64=1, cam_index=None, S=1, V=5, resize_t64=1,
             ori_w=1032.0, ori_h=776.0, image_w=192.0, image_h=128.0)
    a.update(kw)
    return a


def _call(name, **kw):
    from fvp import _lib

    a = _project_args(**{k: v for k, v in kw.items() if k in _project_args()})
    tail = dict(H=32, W=48, sigma=3.0, Cp=32, out=16, joints2d=1, vis2d=1)
    tail.update({k: v for k, v in kw.items() if k in tail})
    head = list(a.values())
    if name == "fvp_project_poses":
        return getattr(_lib.load(), name)(*head, tail["joints2d"], tail["vis2d"], None)
    return getattr(_lib.load(), name)(*head, tail["H"], tail["W"], tail["sigma"], tail["Cp"], tail["out"],
                                      tail["joints2d"], tail["vis2d"], None)


ENTRIES = ["fvp_project_poses", "fvp_render_poses3d", "fvp_render_poses3d_f16"]


@pytest.mark.parametrize("name", ENTRIES)
def test_pose_entries_reject_bad_arguments_on_the_host(name):
    """Every refusal returns before anything is launched (the pointers are not device pointers)."""
    for key in ("joints3d", "count", "cams64", "resize_t64"):
        assert _call(name, **{key: None}) == NULL, key
    for bad in (dict(J=0), dict(J=33, Cp=48), dict(P=0), dict(P=33), dict(V=0), dict(V=256), dict(S=0), dict(B=0),
                dict(ori_w=0.0), dict(ori_h=-1.0), dict(image_w=0.0), dict(image_h=float("nan")),
                dict(image_w=float("inf"))):
        assert _call(name, **bad) == SHAPE, bad
    if name == "fvp_project_poses":
        assert _call(name, joints2d=None) == NULL and _call(name, vis2d=None) == NULL
        return
    assert _call(name, out=None) == NULL
    for bad in (dict(Cp=8), dict(Cp=16), dict(Cp=24), dict(Cp=48), dict(H=0), dict(W=0), dict(W=-3), dict(sigma=0.0),
                dict(sigma=float("nan"))):  # Cp = 16 < J = 17
        assert _call(name, **bad) == SHAPE, bad
    if name.endswith("_f16"):
        assert _call(name, out=8) == SHAPE  # 16-B stores


def test_abi_version_is_unchanged():
    from fvp import _lib

    assert _lib.load().fvp_abi_version() == 22 and _lib.ABI_VERSION == 22


# -- the Python layer --------------------------------------------------------------------------
def test_pack_poses3d_round_trip_and_refusals():
    from fvp import _lib
    from fvp.heatmaps import pack_poses3d

    rng = np.random.default_rng(5)
    people = [rng.normal(size=(17, 4)) for _ in range(3)]  # x, y, z and a column that is ignored
    flags = [rng.integers(-1, 3, size=17).astype(np.float64) for _ in range(3)]
    joints, vis, count = pack_poses3d(people, flags)
    assert joints.dtype == torch.float64 and tuple(joints.shape) == (3, 17, 3)
    assert vis.dtype == torch.uint8 and tuple(vis.shape) == (3, 17)
    assert count.dtype == torch.int32 and count.dim() == 0 and int(count) == 3
    for n in range(3):
        assert np.array_equal(joints[n].numpy(), people[n][:, :3])
        assert np.array_equal(vis[n].numpy(), (flags[n] > 0).astype(np.uint8))  # > 0, as the reference reads them
    j5, v5, c5 = pack_poses3d(people, flags, max_people=5)
    assert tuple(j5.shape) == (5, 17, 3) and torch.equal(j5[:3], joints) and torch.equal(v5[:3], vis) and int(c5) == 3
    assert not j5[3:].any() and not v5[3:].any()
    # Panoptic's [J, 3] flags: column 0 is read
    flags3 = [np.stack([f, np.ones(17), np.zeros(17)], axis=1) for f in flags]
    assert torch.equal(pack_poses3d(people, flags3)[1], vis)
    # no flags: all visible;  meta's arrays (padded with all-zero people) pass as they are
    assert pack_poses3d(people)[1].all()
    ja, va, ca = pack_poses3d(j5.numpy(), v5.numpy().astype(np.float64))
    assert torch.equal(ja, j5) and torch.equal(va, v5) and int(ca) == 5
    # the default collate's stack
    batch = [pack_poses3d(people[:k], flags[:k], max_people=4) for k in (1, 3)]
    assert torch.stack([b[2] for b in batch]).tolist() == [1, 3] and torch.stack([b[0] for b in batch]).shape[0] == 2
    j0, v0, c0 = pack_poses3d(np.zeros((0, 17, 3)), [], max_people=2)  # an empty frame of a known J
    assert tuple(j0.shape) == (2, 17, 3) and int(c0) == 0 and not v0.any()
    for bad in (lambda: pack_poses3d(people, flags, max_people=2), lambda: pack_poses3d([]),
                lambda: pack_poses3d([np.zeros((17, 3)), np.zeros((15, 3))]), lambda: pack_poses3d([np.zeros((17, 2))]),
                lambda: pack_poses3d(people, flags[:2]), lambda: pack_poses3d(people, [np.zeros(15)] * 3),
                lambda: pack_poses3d(people, [np.zeros((17, 2))] * 3)):
        with pytest.raises(_lib.FvpError):
            bad()


def test_pack_cameras64_keeps_float64_values():
    from fvp import geometry
    from fvp.workloads import load_calibration

    for name in ("calibration_shelf.json", "calibration_panoptic_demo.json"):
        cams, seq = load_calibration(name)
        got = geometry.pack_cameras64(cams, seq)
        assert got.dtype == np.float64 and got.shape == (5, geometry.CAM_STRIDE)
        f32 = geometry.pack_cameras(cams, seq)
        assert np.array_equal(got.astype(np.float32), f32)  # the same fields in the same places
        assert (got != f32.astype(np.float64)).any()  # not rounded through fp32
        for v, cam in enumerate(geometry.camera_list(cams, seq)):
            assert np.array_equal(got[v, 0:9], np.asarray(cam["R"]).reshape(9))
            assert np.array_equal(got[v, 9:12], np.asarray(cam["T"]).reshape(3))
            assert got[v, 12:16].tolist() == [float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"])]
            assert np.array_equal(got[v, 16:19], np.asarray(cam["k"]).reshape(3))
            assert np.array_equal(got[v, 19:21], np.asarray(cam["p"]).reshape(2)) and not got[v, 21:].any()


def _operands(J=17):
    return (torch.zeros((2, 5, J, 3), dtype=torch.float64), torch.ones((2, 5, J), dtype=torch.uint8),
            torch.ones((2,), dtype=torch.int32), torch.zeros((5, 24), dtype=torch.float64),
            torch.zeros((2, 3), dtype=torch.float64))


def test_pose_functions_refuse_cpu_tensors_and_bad_operands():
    from fvp import _lib
    from fvp.heatmaps import project_poses, render_poses3d

    kw = dict(ori_image_size=(1032, 776), image_size=(192, 128))
    rkw = dict(heatmap_size=(48, 32), sigma=3.0, **kw)
    j, v, c, cams, t = _operands()
    with pytest.raises(_lib.FvpError, match="HIP device"):
        render_poses3d(j, v, c, cams, t, **rkw)
    with pytest.raises(_lib.FvpError, match="HIP device"):
        project_poses(j, v, c, cams, t, **kw)
    for bad in (lambda: render_poses3d(j.float(), v, c, cams, t, **rkw),
                lambda: render_poses3d(j, v.to(torch.int32), c, cams, t, **rkw),
                lambda: render_poses3d(j, v[:, :4], c, cams, t, **rkw),
                lambda: render_poses3d(j, v, c.to(torch.int64), cams, t, **rkw),
                lambda: render_poses3d(j, v, c[:1], cams, t, **rkw),
                lambda: render_poses3d(j, v, c, cams.float(), t, **rkw),
                lambda: render_poses3d(j, v, c, cams[:, :21], t, **rkw),
                lambda: render_poses3d(j, v, c, cams, t.float(), **rkw),
                lambda: render_poses3d(j, v, c, cams, torch.zeros((3, 3), dtype=torch.float64), **rkw),
                lambda: render_poses3d(torch.zeros((2, 5, 33, 3), dtype=torch.float64), None, c, cams, t, **rkw),
                lambda: render_poses3d(torch.zeros((2, 33, 17, 3), dtype=torch.float64), None, c, cams, t, **rkw),
                lambda: render_poses3d(j, v, c, cams, t, dtype=torch.bfloat16, **rkw),
                lambda: render_poses3d(j, v, c, cams, t, cam_index=[0, 1], **rkw),  # one camera set
                lambda: render_poses3d(j, v, c, cams, t, cam_index=[0, -1], **rkw),
                lambda: render_poses3d(j, v, c, cams, t, cam_index=[0], **rkw),
                lambda: project_poses(j[0], v, c, cams, t, **kw)):
        with pytest.raises(_lib.FvpError):
            bad()


def test_pose_ops_fake_shapes():
    from fvp import ops  # noqa: F401  (registers torch.ops.fvp.*)

    for J, cp in ((15, 16), (17, 32)):
        j, v, c, cams, t = (x.to("meta") for x in _operands(J))
        cams = cams.unsqueeze(0)
        j2, v2 = torch.ops.fvp.project_poses(j, v, c, cams, None, t, 1032.0, 776.0, 192.0, 128.0)
        assert tuple(j2.shape) == (2, 5, 5, J, 2) and j2.dtype == torch.float64 and j2.device.type == "meta"
        assert tuple(v2.shape) == (2, 5, 5, J) and v2.dtype == torch.uint8
        for op, dtype in ((torch.ops.fvp.render_poses3d, torch.float32),
                          (torch.ops.fvp.render_poses3d_f16, torch.float16)):
            out, k2, f2 = op(j, v, c, cams, None, t, 1032.0, 776.0, 192.0, 128.0, 37, 50, 3.0, True)
            assert tuple(out.shape) == (2, 5, 37, 50, cp) and out.dtype == dtype and out.device.type == "meta"
            assert tuple(k2.shape) == (2, 5, 5, J, 2) and k2.dtype == torch.float64
            assert tuple(f2.shape) == (2, 5, 5, J) and f2.dtype == torch.uint8
            out, k2, f2 = op(j, None, c, cams, None, t, 1032.0, 776.0, 192.0, 128.0, 37, 50, 3.0, False)
            assert tuple(out.shape) == (2, 5, 37, 50, cp) and k2.numel() == 0 and f2.numel() == 0
