"""Host-side checks of the sync-free JLN route (no GPU): the dead row's empty window under the
oracle's restatement of project_individual.py:255-275, the two new C entry points' exports and
refusals, and FvpOptions.sync_free.

Every library call below returns from its host checks: none reaches a launch (the fake pointer
16 is only ever passed together with a size or a NULL that is refused first).
"""
import dataclasses
import types

import numpy as np
import pytest

from oracle import fvp_oracle as O

NULL, SHAPE = 1001, 1002
DEAD = (0.0, 0.0, 0.0, 0.0, 0.0, -3.0, -3.0)
P16 = 16  # a non-NULL pointer that is never dereferenced


def _specs():
    from fvp.workloads import WORKLOADS

    out = [(name, w) for name, w in WORKLOADS.items()]
    for s in (2, 8, 33, 64, 65):
        out.append((f"2m_{s}", dataclasses.replace(WORKLOADS["c3"], space_size=(2000.0,) * 3,
                                                   ind_space_size=(2000.0,) * 3, ind_voxels_per_axis=(s, s, s))))
    return out


@pytest.mark.parametrize("name,w", _specs(), ids=[n for n, _ in _specs()])
def test_dead_row_window_is_empty(name, w):
    """(0, 0, 0, 0, 0, -3, -3), and the same row with its centre at +-1e6, gives start >= end on
    x AND y (so the skip holds whichever axis a kernel tests first), for every workload's person
    spec and for 2 .. 65 person voxels per axis on a 2 m space."""
    ind = O.Individual(w.space_size, w.space_center, w.ind_space_size, w.ind_voxels_per_axis)
    rows = np.array([DEAD,
                     (1e6, 1e6, 1e6) + DEAD[3:], (-1e6, -1e6, -1e6) + DEAD[3:],
                     (1e6, -1e6, 0.0) + DEAD[3:], (-1e6, 1e6, 0.0) + DEAD[3:]], np.float32)
    _, offset, start, end = ind.windows(rows)
    assert (start[:, 0] >= end[:, 0]).all() and (start[:, 1] >= end[:, 1]).all(), (name, start, end)
    assert np.isfinite(offset[0]).all()
    # the margin itself: int((1 - (-3)) / 2 * (bins - 1)) = 2 * (bins - 1), exact in fp32
    bins = np.asarray(w.ind_voxels_per_axis[:2])
    margin = ((np.float32(1) - np.float32(-3)) / np.float32(2) * (bins - 1).astype(np.float32)).astype(np.int32)
    assert (margin == 2 * (bins - 1)).all() and (2 * margin >= bins).all()


def test_a_live_row_is_not_skipped():
    """The check above can fail: an ordinary proposal at the space centre has a non-empty window."""
    from fvp.workloads import WORKLOADS

    w = WORKLOADS["c3"]
    ind = O.Individual(w.space_size, w.space_center, w.ind_space_size, w.ind_voxels_per_axis)
    row = np.array([tuple(w.space_center) + (0.0, 0.9, 0.5, 0.5)], np.float32)
    _, _, start, end = ind.windows(row)
    assert (start < end).all()


def test_symbols_and_abi_version():
    from fvp import _lib

    lib = _lib.load()
    assert lib.fvp_abi_version() == 22 and _lib.ABI_VERSION == 22
    for name in ("fvp_pad_proposals", "fvp_fuse_scatter_poses"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_pad_proposals_refusals():
    from fvp import _lib

    f = _lib.load().fvp_pad_proposals
    # (mask, B, K, rows, rs0, rs1, out, frame_of, stream)
    assert f(None, 2, 3, P16, 21, 7, P16, None, None) == NULL
    assert f(P16, 2, 3, None, 21, 7, P16, None, None) == NULL
    assert f(P16, 2, 3, P16, 21, 7, None, P16, None) == NULL
    assert f(P16, -1, 3, P16, 21, 7, P16, None, None) == SHAPE
    assert f(P16, 2, -3, P16, 21, 7, P16, None, None) == SHAPE
    assert f(P16, 0, 3, P16, 21, 7, P16, None, None) == 0
    assert f(P16, 2, 0, P16, 21, 7, P16, P16, None) == 0
    assert f(None, 0, 0, None, 0, 0, None, None, None) == 0


def test_fuse_scatter_poses_refusals():
    from fvp import _lib

    f = _lib.load().fvp_fuse_scatter_poses
    # (mask, pose, weights, maxprob, P, J, all_fused, all_pose, centers, cs, conf_col, stream)
    ok = [P16, P16, P16, P16, 4, 15, P16, P16, None, 7, 4, None]
    for i in (0, 1, 2, 6, 7):
        a = list(ok)
        a[i] = None
        assert f(*a) == NULL, i
    a = list(ok)
    a[3], a[8] = None, P16  # centers asked for without maxprob
    assert f(*a) == NULL
    a = [P16, P16, P16, P16, -4, 15, P16, P16, None, 7, 4, None]
    assert f(*a) == SHAPE
    a = [P16, P16, P16, P16, 4, -1, P16, P16, None, 7, 4, None]
    assert f(*a) == SHAPE
    a = [None, None, None, None, 0, 15, None, None, None, 0, 4, None]
    assert f(*a) == 0


def test_options_default_and_round_trip():
    from fvp import integration

    assert integration.FvpOptions().sync_free is None
    assert integration.DEFAULT_OPTIONS.sync_free is None
    obj = types.SimpleNamespace()
    assert integration.set_options(obj, sync_free=True).sync_free is True
    assert integration.options_of(obj).sync_free is True
    assert integration.set_options(obj, sync_free=False).sync_free is False
    assert integration.set_options(obj, sync_free=None).sync_free is None
    assert integration.options_of(obj) == integration.FvpOptions()


def test_install_passes_sync_free_through():
    from fvp import integration

    class JointLocalizationNet:
        def forward(self):
            pass

    mods = {"models.joint_localization_net": types.SimpleNamespace(JointLocalizationNet=JointLocalizationNet)}
    integration.install(modules=mods)
    assert JointLocalizationNet.fvp_options == integration.FvpOptions()
    integration.install(modules=mods, sync_free=True)
    assert JointLocalizationNet.fvp_options.sync_free is True


def test_sync_free_false_under_capture_raises(monkeypatch):
    """sync_free=False while the stream is being captured: FvpError before anything touches the
    inputs (they are placeholders here: the refusal must not depend on them)."""
    import torch

    from fvp import integration, jln
    from fvp._lib import FvpError

    net = types.SimpleNamespace(training=False)
    integration.set_options(net, sync_free=False)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    hm = torch.zeros((1, 1, 1, 2, 2))
    with pytest.raises(FvpError, match="sync_free"):
        jln.fused_jln_forward(net, {"seq": ["s"]}, hm, None, None, None, None)


@pytest.mark.parametrize("mask", [None, [[True]]], ids=["none", "list"])
def test_a_mask_that_is_no_tensor_raises_fvp_error(mask):
    import torch

    from fvp import integration, jln
    from fvp._lib import FvpError

    net = types.SimpleNamespace(training=False)
    integration.set_options(net, sync_free=True)
    with pytest.raises(FvpError, match="2-D bool device mask"):
        jln.fused_jln_forward(net, {"seq": ["s"]}, torch.zeros((1, 1, 1, 2, 2)), torch.zeros((1, 1, 7)), mask, None,
                              None)
