"""GPU tests of the sync-free JLN route: fvp_pad_proposals and fvp_fuse_scatter_poses bit for
bit against torch.where and fuse_poses + scatter_poses, the route against the synced one with no
CNN in between (per-slot arithmetic: any difference is a bug), against the golden with the real
nets, and a whole heatmaps -> poses forward captured into one graph and replayed.

Order matters on the device: the kernels and the eager route (tests 1-4) run before the capture
(test 5), which records only code that has already run.
"""
import dataclasses
import types

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

HM = (45, 31)  # heatmap_size (W, H) of the small person cases, as tests/test_gpu_cl_half.py
DEAD = (0.0, 0.0, 0.0, 0.0, 0.0, -3.0, -3.0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """Equal bit for bit (NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _masks(B, K):
    n = B * K
    flat = torch.arange(n)
    frame_dead = torch.ones((B, K), dtype=torch.bool)
    frame_dead[0] = False
    return {"none": torch.zeros((B, K), dtype=torch.bool), "all": torch.ones((B, K), dtype=torch.bool),
            "first": (flat == 0).view(B, K), "last": (flat == n - 1).view(B, K),
            "alternating": (flat % 2 == 0).view(B, K), "frame0_dead": frame_dead}


def _poison(t, dead):
    """NaN / +Inf / -Inf / 3e38 in the dead rows of t [..., n, w] (dead [n] bool), cycling."""
    bad = torch.tensor([float("nan"), float("inf"), float("-inf"), 3e38])
    n, w = t.shape[-2], t.shape[-1]
    fill = bad[(torch.arange(n)[:, None] + torch.arange(w)[None, :]) % 4]
    return torch.where(dead[:, None], fill, t)


# -- 1. pad_proposals -----------------------------------------------------------------------------
@pytest.mark.parametrize("B,K", [(1, 1), (1, 10), (3, 5), (2, 16), (5, 300)])
def test_pad_proposals_equals_torch_where(gpu_device, B, K):
    """Every mask pattern; rows a strided [B, K, 7] slice of a wider tensor with NaN / Inf /
    3e38 in the dead slots and a NaN and a -0.0 in live ones (copied bit for bit)."""
    from fvp import ops

    g = torch.Generator().manual_seed(100 * B + K)
    for name, mask in _masks(B, K).items():
        wide = torch.randn((B, K, 11), generator=g) * 1000.0
        wide[..., 2:9] = _poison(wide[..., 2:9].reshape(B * K, 7), ~mask.reshape(-1)).view(B, K, 7)
        live = mask.nonzero()
        if live.shape[0]:
            b0, k0 = live[0].tolist()
            wide[b0, k0, 4], wide[b0, k0, 5] = float("nan"), -0.0
        wide_d = wide.to(gpu_device)
        rows = wide_d[..., 2:9]
        assert rows.stride() == (K * 11, 11, 1)
        props, frame_of = ops.pad_proposals(mask.to(gpu_device), rows)
        want = torch.where(mask[..., None], wide[..., 2:9], torch.tensor(DEAD)).reshape(B * K, 7)
        assert props.dtype == torch.float32 and _same(props.cpu(), want), (name, B, K)
        assert frame_of.dtype == torch.int32
        assert torch.equal(frame_of.cpu(), torch.arange(B, dtype=torch.int32).repeat_interleave(K)), name
        assert _same(wide_d.cpu(), wide), "the input was written"


def test_pad_proposals_rejects_bad_operands(gpu_device):
    from fvp import ops
    from fvp._lib import FvpError

    mask = torch.ones((2, 3), dtype=torch.bool, device=gpu_device)
    rows = torch.zeros((2, 3, 7), device=gpu_device)
    for m, r in ((mask.to(torch.uint8), rows), (mask[0], rows), (mask.cpu(), rows.cpu()), (mask, rows.double()),
                 (mask, rows[:, :2]), (mask, rows[..., :6]), (mask, torch.zeros((2, 3, 14), device=gpu_device)[..., ::2])):
        with pytest.raises(FvpError):
            ops.pad_proposals(m, r)
    p, f = ops.pad_proposals(mask[:0], rows[:0])
    assert tuple(p.shape) == (0, 7) and tuple(f.shape) == (0,)


# -- 2. fuse_scatter_poses ------------------------------------------------------------------------
@pytest.mark.parametrize("J", [1, 15, 65])
@pytest.mark.parametrize("B,K", [(1, 1), (3, 5), (2, 65)])
def test_fuse_scatter_poses_equals_fuse_then_scatter(gpu_device, B, K, J):
    """Live slots == ops.fuse_poses + ops.scatter_poses on the selected slots, bit for bit; dead
    slots +0.0 by their bits although every dead input is NaN / Inf; the dead slots' centres
    column untouched; outputs pre-filled with NaN are fully overwritten."""
    from fvp import _lib, ops
    from fvp.ops import _ptr, _stream

    P = B * K
    g = torch.Generator().manual_seed(1000 * P + J)
    for name, mask in _masks(B, K).items():
        dead = ~mask.reshape(-1)
        pose = _poison((torch.randn((3, P, J * 2), generator=g) * 500.0), dead).view(3, P, J, 2).to(gpu_device)
        weights = _poison(torch.rand((3, P, J), generator=g) * 0.9 + 0.05, dead).reshape(3 * P, J, 1).to(gpu_device)
        maxprob = _poison(torch.rand((3, P, J), generator=g), dead).to(gpu_device)
        mask_d = mask.to(gpu_device)
        idx = mask_d.nonzero()
        live = idx[:, 0] * K + idx[:, 1]
        fused_l, confs_l = ops.fuse_poses(pose[:, live].contiguous(),
                                          weights.view(3, P, J)[:, live].reshape(-1, J, 1).contiguous(),
                                          maxprob[:, live].contiguous())
        for conf_col in (4, 0):
            wide = torch.randn((B, K, 9), generator=g)
            wide[0, 0, 8] = float("nan")
            want_c = wide.to(gpu_device)
            got_c = want_c.clone()
            want_f = torch.zeros((B, K, J, 3), device=gpu_device)
            want_p = torch.zeros((3, B, K, J, 2), device=gpu_device)
            ops.scatter_poses(idx, fused_l, pose[:, live].contiguous(), confs_l, want_f, want_p, want_c[..., 1:8],
                              conf_col)
            got_f, got_p = ops.fuse_scatter_poses(mask_d, pose, weights, maxprob, got_c[..., 1:8], conf_col)
            assert tuple(got_f.shape) == (B, K, J, 3) and tuple(got_p.shape) == (3, B, K, J, 2)
            assert _same(got_f, want_f), (name, conf_col)
            assert _same(got_p, want_p), (name, conf_col)
            assert _same(got_c, want_c), (name, conf_col)
            dead_d = dead.to(gpu_device)
            assert not bool((_bits(got_f).view(P, -1)[dead_d] != 0).any())
            assert not bool((_bits(got_p).view(3, P, -1)[:, dead_d] != 0).any())
        # the entry point itself on NaN-filled outputs: every element is written
        raw_f = torch.full((B, K, J, 3), float("nan"), device=gpu_device)
        raw_p = torch.full((3, B, K, J, 2), float("nan"), device=gpu_device)
        m8 = mask_d.contiguous()
        _lib.call("fvp_fuse_scatter_poses", _ptr(m8), _ptr(pose), _ptr(weights), _ptr(maxprob), P, J, _ptr(raw_f),
                  _ptr(raw_p), None, 0, 4, _stream(pose))
        assert _same(raw_f, want_f) and _same(raw_p, want_p), name
        none_f, none_p = ops.fuse_scatter_poses(mask_d, pose, weights, maxprob, None)
        assert _same(none_f, want_f) and _same(none_p, want_p), name


def test_fuse_scatter_poses_rejects_bad_operands(gpu_device):
    from fvp import ops
    from fvp._lib import FvpError

    B, K, J = 2, 3, 4
    mask = torch.ones((B, K), dtype=torch.bool, device=gpu_device)
    pose = torch.zeros((3, B * K, J, 2), device=gpu_device)
    w = torch.ones((3 * B * K, J, 1), device=gpu_device)
    mp = torch.zeros((3, B * K, J), device=gpu_device)
    c = torch.zeros((B, K, 7), device=gpu_device)
    ops.fuse_scatter_poses(mask, pose, w, mp, c)
    uneven = torch.zeros((B, K + 1, 7), device=gpu_device)[:, :K]  # frames not K slots apart
    for args in ((mask.to(torch.uint8), pose, w, mp, c), (mask, pose[:, :5], w, mp, c), (mask, pose, w[:5], mp, c),
                 (mask, pose, w, mp.double(), c), (mask, pose, w, mp, c.double()), (mask, pose, w, mp, c[:1]),
                 (mask, pose, w, mp, uneven), (mask, pose, w, mp, c, 7), (mask, pose.cpu(), w, mp, c)):
        with pytest.raises(FvpError):
            ops.fuse_scatter_poses(*args)


# -- 3. the route against the synced one, no CNN in between ------------------------------------------
def _person_case(dev, J, S, frames):
    """The person layer of tests/test_gpu_cl_half.py's _person_case: a 2 m space, S^3 person voxels."""
    from fvp import geometry, synthetic
    from fvp.project_individual import ProjectLayer
    from fvp.workloads import WORKLOADS

    space = 2000.0
    w = dataclasses.replace(WORKLOADS["c3"], num_joints=J, space_size=(space,) * 3, ind_space_size=(space,) * 3,
                            ind_voxels_per_axis=(S, S, S), heatmap_size=HM)
    layer = ProjectLayer(w.cfg(str(dev)))
    layer.verbose = False
    layer.on_the_fly = False
    cams, seq = w.cameras()
    cams = dict(cams)
    cams["other"] = list(reversed(list(cams[seq])))
    rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float).to(dev)
    hm = synthetic.uniform_heatmaps(w, frames, seed=J + S).half()
    return w, layer, cams, seq, rt, hm


def _heatmaps(kind, hm16, dev):
    from fvp.heatmaps import ChannelsLastHeatmaps

    B, V, J, H, W = hm16.shape
    if kind in ("planar", "otf"):
        return hm16.float().to(dev)
    cp = 16 * ((J + 15) // 16)
    cl = torch.zeros((B, V, H, W, cp), dtype=torch.float32 if kind == "cl_f32" else torch.float16)
    cl[..., :J] = hm16.permute(0, 1, 3, 4, 2).to(cl.dtype)
    return ChannelsLastHeatmaps(cl.to(dev), J)


@pytest.mark.parametrize("kind", ["planar", "cl_f32", "cl_f16", "otf"])
@pytest.mark.parametrize("S,J", [(8, 15), (16, 17)])
def test_sync_free_equals_synced_route(gpu_device, S, J, kind):
    """fused_jln_forward with sync_free=True and =False on clones of the same centres: conv_net is
    the identity and weight_net a fixed per-slot table, so every step is per-slot arithmetic and
    all_fused, all_pose and the centres afterwards are equal bit for bit, for every mask pattern
    (an all-dead mask gives all zeros); dead centres hold NaN / Inf / 3e38.  planar / channels-last
    fp32 / fp16 heatmaps on the cached fine grid, and the on-the-fly projection."""
    from fvp import integration, jln
    from fvp._lib import FvpError

    B, K = 3, 5
    w, layer, cams, seq, rt, hm16 = _person_case(gpu_device, J, S, B)
    layer.on_the_fly = kind == "otf"
    g = torch.Generator().manual_seed(S + J)
    table = (torch.rand((3, B * K, J), generator=g) * 0.9 + 0.05).to(gpu_device)
    state = {}

    def weight_net(f):  # [3, P, J, S, S]: all slots (sync-free) or the live ones in mask order (synced)
        t = table if f.shape[1] == B * K else table[:, state["live"]]
        return t.reshape(-1, J, 1).contiguous()

    net = types.SimpleNamespace(training=False, project_layer=layer, conv_net=torch.nn.Identity(),
                                weight_net=weight_net, soft_argmax_layer=types.SimpleNamespace(beta=100.0))
    meta = {"seq": [seq] * B}
    heat = _heatmaps(kind, hm16, gpu_device)
    c = torch.tensor(w.space_center)
    for name, mask in _masks(B, K).items():
        pc = torch.zeros((B, K, 7))
        pc[..., :3] = c + (torch.rand((B, K, 3), generator=g) - 0.5) * 1600.0
        pc[..., 4] = 0.5
        pc[..., 5:] = torch.rand((B, K, 2), generator=g) * 1.3 - 0.2
        pc = _poison(pc.view(B * K, 7), ~mask.reshape(-1)).view(B, K, 7).to(gpu_device)
        mask_d = mask.to(gpu_device)
        state["live"] = mask_d.reshape(-1).nonzero()[:, 0]
        out = {}
        for sf in (True, False):
            integration.set_options(net, sync_free=sf)
            centers = pc.clone()
            with torch.no_grad():
                fused, poses = jln.fused_jln_forward(net, meta, heat, centers, mask_d, cams, rt)
            out[sf] = (fused, poses, centers)
        for a, b, what in zip(out[True], out[False], ("all_fused", "all_pose", "centres")):
            assert _same(a, b), (name, what)
        fused, poses, centers = out[True]
        assert tuple(fused.shape) == (B, K, J, 3) and tuple(poses.shape) == (3, B, K, J, 2)
        assert not bool((_bits(fused)[~mask_d] != 0).any()) and not bool((_bits(poses)[:, ~mask_d] != 0).any())
        if name == "all":
            assert torch.isfinite(fused).all() and float(fused.abs().max()) > 0
            assert not _same(centers[..., 4], pc[..., 4])  # the confidences were written
        if name == "none":
            assert _same(centers, pc)
    integration.set_options(net, sync_free=True)
    with pytest.raises(FvpError, match="sequence"):
        jln.fused_jln_forward(net, {"seq": [seq, "other", seq]}, heat, pc.clone(), mask_d, cams, rt)
    with pytest.raises(FvpError, match="mask"):
        jln.fused_jln_forward(net, meta, heat, pc.clone(), mask_d.to(torch.uint8), cams, rt)
    with pytest.raises(FvpError, match="centres"):
        jln.fused_jln_forward(net, meta, heat, pc.double(), mask_d, cams, rt)


def test_forward_all_refuses_one_bin_and_two_rigs(gpu_device):
    from fvp._lib import FvpError

    w, layer, cams, seq, rt, hm16 = _person_case(gpu_device, 15, 8, 2)
    hm = hm16.float().to(gpu_device)
    pc = torch.zeros((2, 3, 7), device=gpu_device)
    mask = torch.ones((2, 3), dtype=torch.bool, device=gpu_device)
    with pytest.raises(FvpError, match="one sequence"):
        layer.forward_all(hm, {"seq": [seq, "other"]}, pc, mask, cams, rt)
    layer._const = dict(layer._const, ind_bins=np.array([1, 8, 8]))
    with pytest.raises(FvpError, match="person voxels"):
        layer.forward_all(hm, {"seq": [seq, seq]}, pc, mask, cams, rt)


# -- 4. the real nets -------------------------------------------------------------------------------
def _jln_net(w, dev):
    """The seeded JLN of tests/test_gpu_fullsize.py::test_fused_jln_forward_matches_reference_jln."""
    import cnn_arch

    from fvp import jln, synthetic
    from fvp.config import AttrDict
    from fvp.project_individual import ProjectLayer

    J = w.num_joints
    net = types.SimpleNamespace(training=False)
    net.project_layer = ProjectLayer(w.cfg(str(dev)))
    net.project_layer.verbose = False
    net.conv_net = cnn_arch.P2PNet(J, J).eval()
    net.conv_net.load_state_dict(synthetic.seeded_state_dict(net.conv_net, 11))
    net.conv_net = net.conv_net.to(dev)
    net.weight_net = cnn_arch.WeightNet(J).eval()
    net.weight_net.load_state_dict(synthetic.seeded_state_dict(net.weight_net, 15))
    net.weight_net = net.weight_net.to(dev)
    net.soft_argmax_layer = jln.SoftArgmaxLayer(AttrDict.wrap({"NETWORK": {"BETA": 100}}))
    return net


def _hdn_net(w, dev):
    """The seeded HDN of tests/test_gpu_fullsize.py (_hdn)."""
    import cnn_arch

    from fvp import synthetic
    from fvp.project_whole import ProjectLayer
    from fvp.proposal import ProposalLayer

    net = types.SimpleNamespace()
    cfg = w.cfg(str(dev))
    net.project_layer = ProjectLayer(cfg)
    net.project_layer.verbose = False
    net.center_net = cnn_arch.CenterNet(w.num_joints, 1).eval()
    net.center_net.load_state_dict(synthetic.seeded_state_dict(net.center_net, 12))
    with torch.no_grad():
        net.center_net.output_hm[2].bias += float(golden("e2e_c3.npz")["hm_bias_shift"])
    net.center_net = net.center_net.to(dev)
    net.c2c_net = cnn_arch.C2CNet(w.num_joints, 1).eval()
    net.c2c_net.load_state_dict(synthetic.seeded_state_dict(net.c2c_net, 14))
    net.c2c_net = net.c2c_net.to(dev)
    net.proposal_layer = ProposalLayer(cfg).eval()
    net.max_people = w.max_people
    return net


def test_sync_free_matches_reference_jln(gpu_device):
    """The sync-free route with the real P2PNet / WeightNet on the fvp convolutions against the
    reference's own JointLocalizationNet.forward (e2e_c3.npz), with the tolerances of
    test_fused_jln_forward_matches_reference_jln: poses and fused within 0.2 mm, centres within
    1e-4, zeros where ~mask."""
    from fvp import geometry, integration, jln
    from fvp.workloads import WORKLOADS

    d = golden("e2e_c3.npz")
    w = WORKLOADS["c3"]
    cams, seq = w.cameras()
    net = _jln_net(w, gpu_device)
    hm = torch.from_numpy(golden("whole_c3.npz")["heatmaps"]).to(gpu_device)
    rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float).to(gpu_device)
    mask = torch.from_numpy(d["mask"]).to(gpu_device)
    meta = {"seq": [seq] * 2}
    out = {}
    for sf in (False, True):
        integration.set_options(net, cnn=True, sync_free=sf)
        pc = torch.from_numpy(d["centers"]).to(gpu_device)
        with torch.no_grad():
            fused, poses = jln.fused_jln_forward(net, meta, hm, pc, mask, cams, rt)
        torch.cuda.synchronize()
        out[sf] = [t.cpu().numpy() for t in (fused, poses, pc)]
    fused, poses, pc = out[True]
    print(f"sync-free JLN: {int(d['mask'].sum())} live of {d['mask'].size} slots; max |diff| from the synced route: "
          f"fused {np.abs(fused - out[False][0]).max():.3g} mm, poses {np.abs(poses - out[False][1]).max():.3g} mm, "
          f"centres {np.abs(pc - out[False][2]).max():.3g}; from the reference: fused "
          f"{np.abs(fused - d['fused']).max():.3g} mm, poses {np.abs(poses - d['poses']).max():.3g} mm, "
          f"confs {np.abs(pc[..., 4] - d['centers_after'][..., 4]).max():.3g}")
    np.testing.assert_allclose(poses, d["poses"], atol=0.2, rtol=0)
    np.testing.assert_allclose(fused, d["fused"], atol=0.2, rtol=0)
    np.testing.assert_allclose(pc, d["centers_after"], atol=1e-4, rtol=0)
    assert not np.any(fused[~d["mask"]]) and not np.any(poses[:, ~d["mask"]])


# -- 5. capture -------------------------------------------------------------------------------------
def _close(got, ref):
    """Test 4's tolerances, for outputs whose eager runs themselves differ from run to run."""
    fused, centers = got[0].cpu().numpy(), got[2].cpu().numpy()
    np.testing.assert_allclose(fused[..., :3], ref[0].cpu().numpy()[..., :3], atol=0.2, rtol=0)
    np.testing.assert_allclose(got[1].cpu().numpy(), ref[1].cpu().numpy(), atol=0.2, rtol=0)
    np.testing.assert_allclose(centers, ref[2].cpu().numpy(), atol=1e-4, rtol=0)
    np.testing.assert_allclose(fused[..., 3:], ref[0].cpu().numpy()[..., 3:], atol=1e-4, rtol=0)


def test_whole_forward_captures_and_replays(gpu_device):
    """heatmaps -> poses (fused_hdn_forward -> mask -> fused_jln_forward -> the cat of the
    confidence columns, faster_voxelpose.py:85-100) records into ONE graph with sync_free left at
    None -- the capture itself proves that nothing reads the device -- and each replay equals an
    eager sync_free=True forward on the same values: the golden frames, other frames with other
    live slots, and all zeros.  (With the seeded heatmap head an all-zero input still scores
    6 of 20 slots above the threshold -- the head's bias alone.)  The batch with no live slot --
    the empty scene -- is a second capture of the same forward with a threshold above every
    score, replayed on the same three inputs: equal to eager bit for bit, poses +0.0 by their
    bits, the centres exactly as the HDN left them.  Every replay after the first is the one
    that counts: a graph whose replays depend on what the previous one left in its buffers
    passes the first and fails the rest (the person planes' pre-zeroing as a memset node did)."""
    from fvp import geometry, integration, jln
    from fvp.graphs import CapturedStep
    from fvp.workloads import WORKLOADS

    w = WORKLOADS["c3"]
    J = w.num_joints
    cams, seq = w.cameras()
    hdn, jl = _hdn_net(w, gpu_device), _jln_net(w, gpu_device)
    # the seeded HDN scores every slot above the config's threshold on any input; the median of the
    # reference's own confidences on the golden frames (e2e_c3.npz) as the threshold splits them
    hdn.proposal_layer.min_score = float(np.median(golden("e2e_c3.npz")["centers"][..., 4]))
    for net in (hdn, jl):
        integration.set_options(net, cnn=True)
    a = torch.from_numpy(golden("whole_c3.npz")["heatmaps"]).to(gpu_device)
    B = a.shape[0]
    assert B == 2
    rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float).to(gpu_device)
    meta = {"seq": [seq] * B}
    static = a.clone()

    def model(hm, hdn=hdn):
        _, _, centers, _ = integration.fused_hdn_forward(hdn, hm, meta, cams, rt)
        mask = centers[:, :, 3] >= 0
        fused, poses = jln.fused_jln_forward(jl, meta, hm, centers, mask, cams, rt)
        fused = torch.cat((fused, centers[:, :, 3:5].reshape(B, -1, 1, 2).repeat(1, 1, J, 1)), dim=3)
        return fused, poses, centers

    def eager(hm, hdn=hdn):
        integration.set_options(jl, sync_free=True)
        try:
            with torch.no_grad():
                out = model(hm, hdn)
            torch.cuda.synchronize()
            return out
        finally:
            integration.set_options(jl, sync_free=None)

    inputs = {"golden": a, "flipped": (a.flip(0) * 0.75).contiguous(), "zeros": torch.zeros_like(a)}
    refs = {k: eager(v.clone()) for k, v in inputs.items()}  # (also: every shape of the route has run eagerly)
    live = {k: int((r[2][:, :, 3] >= 0).sum()) for k, r in refs.items()}
    print(f"live slots of {B * w.max_people}: {live}")
    assert 0 < live["golden"] < B * w.max_people
    assert not torch.equal(refs["golden"][2][:, :, 3] >= 0, refs["flipped"][2][:, :, 3] >= 0)

    # nothing in the eager sync-free forward synchronises (where this build can tell)
    try:
        torch.cuda.set_sync_debug_mode("error")
        debug = torch.cuda.get_sync_debug_mode() == 2
    except Exception:  # noqa: BLE001 -- an unsupported build: the capture below is the proof
        debug = False
    try:
        if debug:
            integration.set_options(jl, sync_free=True)
            with torch.no_grad():
                model(static)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        integration.set_options(jl, sync_free=None)
    torch.cuda.synchronize()

    assert integration.options_of(jl).sync_free is None
    with torch.no_grad():
        cap = CapturedStep(lambda: model(static))
    for name, x in inputs.items():
        static.copy_(x)
        got = [t.clone() for t in cap.replay()]
        torch.cuda.synchronize()
        ref = refs[name]
        if all(_same(g, r) for g, r in zip(got, ref)):
            continue
        # only a difference that eager-vs-eager also shows may be compared within tolerances
        again = eager(x.clone())
        diff = [float((g.double() - r.double()).abs().nan_to_num(0).max()) for g, r in zip(got, ref)]
        assert not all(_same(p, q) for p, q in zip(again, ref)), \
            f"{name}: the replay differs from eager (max |diff| {diff}) although eager repeats bit for bit"
        print(f"{name}: eager differs from eager; replay max |diff| {diff}")
        _close(got, ref)

    # the empty scene: the same forward with a threshold above every score, so that no slot is
    # live -- the real P2PNet, soft-argmax and WeightNet on all-zero planes and the device-side
    # mask, inside a replayed graph, on each of the three inputs
    empty = _hdn_net(w, gpu_device)
    empty.proposal_layer.min_score = 1e30
    integration.set_options(empty, cnn=True)
    with torch.no_grad():
        hdn_only = {k: integration.fused_hdn_forward(empty, v.clone(), meta, cams, rt)[2].clone()
                    for k, v in inputs.items()}
    dead_refs = {k: eager(v.clone(), empty) for k, v in inputs.items()}
    with torch.no_grad():
        cap_dead = CapturedStep(lambda: model(static, empty))
    for name, x in inputs.items():
        static.copy_(x)
        fused, poses, centers = (t.clone() for t in cap_dead.replay())
        torch.cuda.synchronize()
        assert not bool((centers[:, :, 3] >= 0).any()), name
        for g, r, what in zip((fused, poses, centers), dead_refs[name], ("fused", "poses", "centres")):
            assert _same(g, r), (name, what)
        assert not bool((_bits(fused[..., :3]) != 0).any()) and not bool((_bits(poses) != 0).any()), name
        assert _same(centers[..., 4], hdn_only[name][..., 4]), f"{name}: a dead slot's confidence was written"
        assert _same(centers, hdn_only[name]), name
