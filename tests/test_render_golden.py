"""CPU tests of the keypoint renderer's host side: the numpy restatement
(tests/render_ref.py) against the reference's recorded heatmaps
(tests/golden/render_kp.npz, tools/gen_render_golden.py), the new C-ABI
entry's argument checks, and pack_keypoints."""
import os

import numpy as np
import pytest
import torch

import render_ref as R
from conftest import GOLDEN
from render_ref import golden_cases


def test_golden_file_is_small_and_covers_the_quirks():
    assert os.path.getsize(os.path.join(GOLDEN, "render_kp.npz")) < (1 << 20)
    cases = golden_cases()
    assert {(c["joints"].shape[3], c["heatmap_size"], c["vis"] is not None) for c in cases} == {
        (17, (48, 32), False), (15, (50, 37), False), (17, (50, 37), True), (15, (48, 32), True)}
    for c in cases:
        W, H = c["heatmap_size"]
        recs = [r for b in range(R.B)
                for r in R.windows(c["joints"][b], c["count"][b], None, c["image_size"], c["heatmap_size"], c["sigma"])]
        ul = np.array([r[3] for r in recs])
        br = np.array([r[4] for r in recs])
        skipped = np.array([r[5] for r in recs])
        # every skip condition, the br == 0 window that is not skipped, negative ul that paints
        assert (ul[:, 0] >= W).any() and (ul[:, 1] >= H).any() and (br[:, 0] < 0).any() and (br[:, 1] < 0).any()
        assert ((br[:, 0] == 0) & ~skipped).any()
        assert ((ul[:, 0] < 0) & (ul[:, 1] < 0) & (br[:, 0] > 0) & (br[:, 1] > 0)).any()
        assert ((br[:, 0] > W) & (br[:, 1] > H) & (ul[:, 0] < W) & (ul[:, 1] < H)).any()
        sizes = {r[6] for r in recs}
        assert min(sizes) == 14 and max(sizes) == 52 and len(sizes) >= 3  # clipped low, high, between
        assert np.isnan(c["joints"]).any()  # padded rows


@pytest.mark.parametrize("case", range(4))
def test_render_ref_matches_the_reference(case):
    """Support identical, values within 1e-6 (fp32 argument and expf against the reference's fp64)."""
    c = golden_cases()[case]
    got = R.render(c["joints"], c["count"], c["vis"], c["image_size"], c["heatmap_size"], c["sigma"])
    ref = c["heatmaps"]
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.array_equal(got != 0, ref != 0)
    err = float(np.abs(got - ref).max())
    print(f"render_ref vs reference, case {case}: max abs error {err:.3g}")
    assert err <= 1e-6


def test_render_entry_rejects_bad_arguments_on_the_host():
    from fvp import _lib

    f = _lib.load().fvp_render_keypoints
    #        joints f64 count vis   B  V  P  J   H   W   img_w  img_h  sigma Cp out stream
    assert f(None, 1, 1, None, 2, 2, 5, 17, 32, 48, 192.0, 128.0, 3.0, 32, 1, None) == 1001
    assert f(1, 1, None, None, 2, 2, 5, 17, 32, 48, 192.0, 128.0, 3.0, 32, 1, None) == 1001
    assert f(1, 1, 1, None, 2, 2, 5, 17, 32, 48, 192.0, 128.0, 3.0, 32, None, None) == 1001
    assert f(1, 1, 1, None, 2, 2, 5, 33, 32, 48, 192.0, 128.0, 3.0, 48, 1, None) == 1002  # J = 33
    assert f(1, 1, 1, None, 2, 2, 33, 17, 32, 48, 192.0, 128.0, 3.0, 32, 1, None) == 1002  # P = 33
    assert f(1, 1, 1, None, 2, 2, 5, 7, 32, 48, 192.0, 128.0, 3.0, 8, 1, None) == 1002  # Cp = 8
    assert f(1, 1, 1, None, 0, 2, 5, 17, 32, 48, 192.0, 128.0, 3.0, 32, 1, None) == 1002  # B = 0
    assert f(1, 1, 1, None, 2, 2, 5, 17, 32, 48, 192.0, 128.0, 3.0, 16, 1, None) == 1002  # Cp < J
    assert f(1, 1, 1, None, 2, 2, 5, 17, 32, 0, 192.0, 128.0, 3.0, 32, 1, None) == 1002  # W = 0
    assert f(1, 1, 1, None, 2, 2, 5, 17, 32, 48, 192.0, 128.0, 0.0, 32, 1, None) == 1002  # sigma = 0


def test_pack_keypoints_round_trip():
    from fvp import _lib
    from fvp.heatmaps import pack_keypoints

    rng = np.random.default_rng(5)
    views = [[rng.normal(size=(17, 3)) for _ in range(n)] for n in (2, 0, 3, 1)]  # x, y, score
    joints, count = pack_keypoints(views)
    assert joints.dtype == torch.float64 and tuple(joints.shape) == (4, 3, 17, 2)
    assert count.dtype == torch.int32 and count.tolist() == [2, 0, 3, 1]
    for v, view in enumerate(views):
        for n, p in enumerate(view):
            assert np.array_equal(joints[v, n].numpy(), p[:, :2])
        assert not joints[v, len(view):].any()
    joints5, count5 = pack_keypoints(views, max_people=5)
    assert tuple(joints5.shape) == (4, 5, 17, 2) and torch.equal(joints5[:, :3], joints) and torch.equal(count5, count)
    with pytest.raises(_lib.FvpError):
        pack_keypoints(views, max_people=2)
    with pytest.raises(_lib.FvpError):
        pack_keypoints([[np.zeros((17, 2)), np.zeros((15, 2))]])


def test_render_keypoints_refuses_cpu_tensors_and_bad_operands():
    from fvp import _lib
    from fvp.heatmaps import render_keypoints

    kw = dict(image_size=(192, 128), heatmap_size=(48, 32), sigma=3.0)
    joints, count = torch.zeros((1, 2, 3, 17, 2), dtype=torch.float64), torch.ones((1, 2), dtype=torch.int32)
    with pytest.raises(_lib.FvpError, match="HIP device"):
        render_keypoints(joints, count, **kw)
    with pytest.raises(_lib.FvpError):
        render_keypoints(joints.to(torch.float16), count, **kw)
    with pytest.raises(_lib.FvpError):
        render_keypoints(joints, count.to(torch.int64), **kw)
    with pytest.raises(_lib.FvpError):
        render_keypoints(torch.zeros((1, 2, 3, 33, 2)), count, **kw)


def test_render_op_fake_shape():
    from fvp import ops  # noqa: F401  (registers torch.ops.fvp.*)

    for J, cp in ((15, 16), (17, 32)):
        joints = torch.empty((2, 3, 4, J, 2), dtype=torch.float64, device="meta")
        out = torch.ops.fvp.render_keypoints(joints, torch.empty((2, 3), dtype=torch.int32, device="meta"), None,
                                             192.0, 128.0, 37, 50, 3.0)
        assert tuple(out.shape) == (2, 3, 37, 50, cp) and out.dtype == torch.float32 and out.device.type == "meta"
