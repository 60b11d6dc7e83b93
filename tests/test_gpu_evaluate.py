"""fvp_match_poses / fvp_match_actors and fvp.evaluate on the device, against
tests/eval_ref.py: the golden cases of the reference's own evaluate methods and a
seeded sweep over the shapes at which the kernels take another path (K * G past
the block of 128, one frame per block across N = 2,049).

Discrete outputs (gt_index, pred_index, parts, valid_count) and the score bits are
equal exactly; mpjpe is NaN exactly where the reference's is and otherwise within
(2n + 8) * 2^-53 relative, n the joints averaged: both sides round each distance
(three squares, two sums, a square root: about 3.5 ulp), the n-term sum and the
division, the reference pairwise and the kernel in index order.
"""
import types

import numpy as np
import pytest
import torch

import eval_cases as EC
import eval_ref as E

pytestmark = pytest.mark.gpu

GUARD = 3                                  # rows after each output that a launch must leave alone
FILL64 = 0x7FF8DEAD0000BEEF                # a NaN no computation produces
FILL32 = 0x7FC0BEEF                        # the same for fp32; as int32 / uint32 it is a value no output takes


def _filled(shape, dtype, dev):
    if dtype == torch.float64:
        return torch.full(shape, FILL64, dtype=torch.int64, device=dev).view(torch.float64)
    t = torch.full(shape, FILL32, dtype=torch.int32, device=dev)
    return t.view(dtype) if dtype != torch.int32 else t


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _check_written(out, rows, fill):
    got = _bits(out.cpu().numpy())
    assert not (got[:rows] == fill).any(), "an output element was not written"
    assert (got[rows:] == fill).all(), "a guard row was written"


def _close(got, want, n):
    """NaN exactly where the reference has NaN; elsewhere within (2n + 8) * 2^-53 relative."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    bound = (2.0 * np.broadcast_to(n, want.shape)[ok] + 8.0) * 2.0 ** -53 * np.abs(want[ok])
    err = np.abs(got[ok] - want[ok])
    assert (err <= bound).all(), f"worst {np.max(err / np.maximum(bound, 1e-300)):.3f} of the bound"


def launch_poses(dev, preds, joints, vis, count):
    from fvp import _lib

    N, K, J, C = preds.shape
    G = joints.shape[1]
    p = torch.from_numpy(preds).to(dev)
    gt = torch.from_numpy(np.ascontiguousarray(joints, np.float64)).to(dev)
    gv = torch.from_numpy((vis > 0.1).astype(np.uint8)).to(dev)
    cnt = torch.from_numpy(count.astype(np.int32)).to(dev)
    mpjpe = _filled((N + GUARD, K), torch.float64, dev)
    idx = _filled((N + GUARD, K), torch.int32, dev)
    score = _filled((N + GUARD, K), torch.float32, dev)
    _lib.call("fvp_match_poses", p.data_ptr(), N, K, J, C, gt.data_ptr(), gv.data_ptr(), cnt.data_ptr(), G,
              mpjpe.data_ptr(), idx.data_ptr(), score.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    for out, fill in ((mpjpe, FILL64), (idx, FILL32), (score, FILL32)):
        _check_written(out, N, fill)
    return {"mpjpe": mpjpe[:N].cpu().numpy(), "gt_index": idx[:N].cpu().numpy(), "score": score[:N].cpu().numpy()}


def check_poses(dev, preds, joints, vis, count, want=None):
    got = launch_poses(dev, preds, joints, vis, count)
    if want is None:
        want = E.panoptic(preds, joints, vis, count)[3]
    assert np.array_equal(got["gt_index"], want["gt_index"])
    assert np.array_equal(_bits(got["score"]), _bits(np.ascontiguousarray(preds[:, :, 0, 4])))
    matched = np.maximum(want["gt_index"], 0)
    n = (vis > 0.1).sum(axis=2)[np.arange(len(preds))[:, None], matched]  # visible joints of the matched person
    _close(got["mpjpe"], want["mpjpe"], n)
    return got


def launch_actors(dev, preds, gt, present, convert):
    from fvp import _lib

    N, K, _, C = preds.shape
    A = gt.shape[1]
    p = torch.from_numpy(preds).to(dev)
    g = torch.from_numpy(np.ascontiguousarray(gt, np.float64)).to(dev)
    pr = torch.from_numpy(present.astype(np.uint8)).to(dev)
    mpjpe = _filled((N + GUARD, A), torch.float64, dev)
    idx = _filled((N + GUARD, A), torch.int32, dev)
    parts = _filled((N + GUARD, A), torch.int32, dev)
    valid = _filled((N + GUARD,), torch.int32, dev)
    _lib.call("fvp_match_actors", p.data_ptr(), N, K, C, g.data_ptr(), pr.data_ptr(), A, convert, mpjpe.data_ptr(),
              idx.data_ptr(), parts.data_ptr(), valid.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    for out, fill in ((mpjpe, FILL64), (idx, FILL32), (parts, FILL32), (valid, FILL32)):
        _check_written(out, N, fill)
    return {"mpjpe": mpjpe[:N].cpu().numpy(), "pred_index": idx[:N].cpu().numpy(),
            "parts": parts[:N].cpu().numpy().view(np.uint32), "valid_count": valid[:N].cpu().numpy()}


def check_actors(dev, preds, gt, present, convert, want=None):
    got = launch_actors(dev, preds, gt, present, convert)
    if want is None:
        want = E.match_actors(preds, gt, present, convert)[0]
    for k in ("pred_index", "parts", "valid_count"):
        assert np.array_equal(got[k], want[k]), k
    _close(got["mpjpe"], want["mpjpe"], 14)
    return got


# -- the kernels -------------------------------------------------------------------------

@pytest.mark.parametrize("name", EC.PANOPTIC_CASES)
def test_match_poses_on_the_golden(gpu_device, name):
    check_poses(gpu_device, *EC.panoptic_golden(name), want=EC.records(name, ("mpjpe", "gt_index", "score")))


@pytest.mark.parametrize("K,G,J", EC.PANOPTIC_SWEEP, ids=[f"K{k}-G{g}-J{j}" for k, g, j in EC.PANOPTIC_SWEEP])
def test_match_poses_sweep(gpu_device, K, G, J):
    check_poses(gpu_device, *EC.random_panoptic(100 * K + 10 * G + J, 3, K, G, J))


def test_match_poses_across_2049_frames(gpu_device):
    preds, joints, vis, count = EC.random_panoptic(7, 2049, 4, 3, 5, C=5)
    check_poses(gpu_device, preds, joints, vis, count)


@pytest.mark.parametrize("name", EC.ACTOR_CASES)
def test_match_actors_on_the_golden(gpu_device, name):
    check_actors(gpu_device, *EC.actor_golden(name),
                 want=EC.records(name, ("mpjpe", "pred_index", "parts", "valid_count")))


@pytest.mark.parametrize("K,A,convert", EC.ACTOR_SWEEP,
                         ids=[f"K{k}-A{a}-{'campus' if c else 'shelf'}" for k, a, c in EC.ACTOR_SWEEP])
def test_match_actors_sweep(gpu_device, K, A, convert):
    check_actors(gpu_device, *EC.random_actors(100 * K + 10 * A + convert, 4, K, A, convert), convert)


def test_no_frames_is_success_without_a_launch(gpu_device):
    from fvp import evaluate as V

    rec = V.match_actors(torch.empty((0, 3, 17, 5), device=gpu_device),
                         V.ActorGroundTruth(torch.empty((0, 4, 14, 3), dtype=torch.float64, device=gpu_device),
                                            torch.empty((0, 4), dtype=torch.uint8, device=gpu_device)), V.CAMPUS)
    assert rec["mpjpe"].shape == (0, 4) and rec["valid_count"].shape == (0,)


# -- the caller's stream -----------------------------------------------------------------

def _side_stream(dev, cycles):
    """A stream seen to run beside the default one (HIP maps streams onto a few hardware
    queues; one that shares the default stream's queue could not tell a misplaced launch)."""
    ones = torch.ones(64, device=dev)
    for _ in range(8):
        side, buf = torch.cuda.Stream(dev), torch.zeros(64, device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            torch.cuda._sleep(cycles)
            buf.copy_(ones)
        seen = float((buf + 0.0).sum())
        side.synchronize()
        if seen == 0.0:
            return side
    pytest.fail("no torch.cuda.Stream() runs beside the default stream: the stream test cannot tell")


def test_launches_land_on_the_current_stream(gpu_device):
    """On a side stream: a sleep, then new predictions copied into the buffer, then the call.
    A launch that went to the default stream runs during the sleep and reads the old ones."""
    from fvp import evaluate as V

    dev, cycles = gpu_device, 20_000_000  # several ms of sleep against microseconds of kernel
    side = _side_stream(dev, cycles)
    old, joints, vis, count = EC.random_panoptic(1, 3, 10, 4, 15)
    new = EC.random_panoptic(2, 3, 10, 4, 15)[0]
    gt = V.PanopticGroundTruth.from_db(EC.db_of(joints, vis, count)).to(dev)
    a_old, gt_a, present = EC.random_actors(3, 4, 10, 4, E.CAMPUS)
    a_new = EC.random_actors(4, 4, 10, 4, E.CAMPUS)[0]
    agt = V.ActorGroundTruth(torch.from_numpy(gt_a).to(dev), torch.from_numpy(present.astype(np.uint8)).to(dev))
    buf, abuf = torch.from_numpy(old).to(dev), torch.from_numpy(a_old).to(dev)
    src, asrc = torch.from_numpy(new).to(dev), torch.from_numpy(a_new).to(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        buf.copy_(src)
        abuf.copy_(asrc)
        rec = V.match_poses(buf, gt)
        arec = V.match_actors(abuf, agt, V.CAMPUS)
    side.synchronize()
    want = E.panoptic(new, joints, vis, count)[3]
    stale = E.panoptic(old, joints, vis, count)[3]
    assert not np.array_equal(want["gt_index"], stale["gt_index"])
    assert np.array_equal(rec["gt_index"], want["gt_index"])
    assert np.array_equal(_bits(rec["score"]), _bits(want["score"]))
    awant = E.match_actors(a_new, gt_a, present, E.CAMPUS)[0]
    assert not np.array_equal(awant["pred_index"], E.match_actors(a_old, gt_a, present, E.CAMPUS)[0]["pred_index"])
    assert np.array_equal(arec["pred_index"], awant["pred_index"]) and np.array_equal(arec["parts"], awant["parts"])


# -- the public functions and the drop-in ------------------------------------------------

def _want(name):
    g = EC.golden()
    return float(g[f"{name}_metric"]), str(g[f"{name}_msg"])


@pytest.mark.parametrize("name", EC.PANOPTIC_CASES)
def test_panoptic_returns_the_reference_result(gpu_device, name):
    from fvp import evaluate as V

    preds, joints, vis, count = EC.panoptic_golden(name)
    gt = V.PanopticGroundTruth.from_db(EC.db_of(joints, vis, count)).to(gpu_device)
    for p in (torch.from_numpy(preds).to(gpu_device), list(torch.from_numpy(preds).to(gpu_device)),
              torch.from_numpy(preds).to(gpu_device).requires_grad_()):
        metric, msg = V.panoptic(p, gt)
        assert (float(metric), msg) == _want(name)


@pytest.mark.parametrize("name", EC.ACTOR_CASES)
def test_pcp_returns_the_reference_result(gpu_device, name):
    from fvp import evaluate as V

    preds, _, _, convert = EC.actor_golden(name)
    gt = V.ActorGroundTruth.from_actor3d(EC.actor3d_of(name), EC.golden()[f"{name}_frame_range"]).to(gpu_device)
    metric, msg = V.pcp(torch.from_numpy(preds).to(gpu_device), gt, convert)
    assert (float(metric), msg) == _want(name)


def test_cpu_predictions_raise(gpu_device):
    from fvp import _lib
    from fvp import evaluate as V

    preds, joints, vis, count = EC.panoptic_golden("panoptic")
    gt = V.PanopticGroundTruth.from_db(EC.db_of(joints, vis, count)).to(gpu_device)
    with pytest.raises(_lib.FvpError, match="HIP device"):
        V.panoptic(torch.from_numpy(preds), gt)
    with pytest.raises(_lib.FvpError, match="HIP device"):  # ground truth left on the host
        V.panoptic(torch.from_numpy(preds).to(gpu_device), V.PanopticGroundTruth.from_db(EC.db_of(joints, vis, count)))


def test_shelf_raises_on_a_frame_without_a_valid_prediction(gpu_device):
    from fvp import evaluate as V

    preds = EC.actor_golden("campus")[0]
    gt = V.ActorGroundTruth.from_actor3d(EC.actor3d_of("campus"), EC.golden()["campus_frame_range"]).to(gpu_device)
    frame = int(np.nonzero(EC.records("campus", ("valid_count",))["valid_count"] == 0)[0][0])
    with pytest.raises(ValueError, match=f"frame {frame}"):
        V.pcp(torch.from_numpy(preds).to(gpu_device), gt, V.SHELF)


def test_patched_datasets_return_the_reference_result(gpu_device, tmp_path):
    from fvp import integration

    def original(self, preds, recall_threshold=500):
        raise AssertionError("device predictions went to the original method")

    classes = {n: type(n, (), {"evaluate": original}) for n in ("Panoptic", "Shelf", "Campus")}
    mods = {f"dataset.{n.lower()}": types.SimpleNamespace(**{n: c}) for n, c in classes.items()}
    assert len(integration.install(modules=mods, evaluate=True)) == 3
    preds, joints, vis, count = EC.panoptic_golden("panoptic")
    ds = classes["Panoptic"]()
    ds.db, ds.db_size = EC.db_of(joints, vis, count), len(count)
    dev_preds = torch.from_numpy(preds).to(gpu_device)
    for _ in range(2):  # the second call takes the ground truth cached on the dataset object
        metric, msg = ds.evaluate(dev_preds)
        assert (float(metric), msg) == _want("panoptic")
    assert dev_preds.device in ds._fvp_evaluate_gt
    for name, cls in (("shelf", "Shelf"), ("campus", "Campus")):
        d = tmp_path / name
        d.mkdir()
        EC.write_actors_mat(str(d / "actorsGT.mat"), EC.actor3d_of(name))
        ds = classes[cls]()
        ds.dataset_dir, ds.frame_range = str(d), [int(f) for f in EC.golden()[f"{name}_frame_range"]]
        metric, msg = ds.evaluate(torch.from_numpy(EC.actor_golden(name)[0]).to(gpu_device))
        assert (float(metric), msg) == _want(name)
