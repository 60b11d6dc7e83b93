"""CPU tests of the scoring path (fvp.evaluate, csrc/fvp_eval.hip's host checks):
tests/eval_ref.py against the reference's recorded results, the vectorised host
scoring against the same, argument validation without a device, and the
install(evaluate=True) drop-in on stand-in dataset classes."""
import types

import numpy as np
import pytest
import torch

import eval_cases as EC
import eval_ref as E


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", EC.PANOPTIC_CASES)
def test_eval_ref_reproduces_the_reference_on_panoptic(name):
    g = EC.golden()
    metric, msg, items, rec = E.panoptic(*EC.panoptic_golden(name))
    assert (float(metric), msg) == (float(g[f"{name}_metric"]), str(g[f"{name}_msg"]))
    assert _same(np.array(items, np.float64).reshape(-1, 3), g[f"{name}_eval_list"])
    for k, v in EC.records(name, ("mpjpe", "gt_index", "score")).items():
        assert rec[k].dtype == v.dtype and _same(rec[k], v), k


@pytest.mark.parametrize("name", EC.ACTOR_CASES)
def test_eval_ref_reproduces_the_reference_on_actors(name):
    g = EC.golden()
    metric, msg, rec = E.pcp(*EC.actor_golden(name))
    assert (float(metric), msg) == (float(g[f"{name}_metric"]), str(g[f"{name}_msg"]))
    for k, v in EC.records(name, ("mpjpe", "pred_index", "parts", "valid_count")).items():
        assert rec[k].dtype == v.dtype and _same(rec[k], v), k


def test_golden_holds_the_cases_the_kernels_can_get_wrong():
    preds, joints, vis, count = EC.panoptic_golden("panoptic")
    rec = EC.records("panoptic", ("mpjpe", "gt_index", "score"))
    valid = preds[:, :, 0, 3] >= 0
    assert count[0] == 0 and valid[0].any() and (rec["gt_index"][0] == -1).all()       # no people: ignored
    assert count[1] > 0 and not valid[1].any()                                           # people, nothing valid
    assert (vis[2, 1] <= 0.1).all() and np.isnan(rec["mpjpe"][2][valid[2]]).all()        # a hidden person: NaN wins
    assert _same(joints[3, 0], joints[3, 1]) and (rec["gt_index"][3, :2] == 0).all()     # a tie: the first
    assert len(np.unique(rec["score"][4])) == 1 and rec["score"][5, 0] == rec["score"][4, 0]  # equal scores
    assert np.isnan(preds[5, 2, :, :3]).any() and np.isnan(rec["mpjpe"][5, 2])           # a NaN coordinate
    assert np.isnan(preds[6, 1, 0, 3]) and rec["gt_index"][6, 1] == -1                   # a NaN flag: not valid
    assert len(EC.golden()["panoptic_empty_eval_list"]) == 0 and EC.golden()["panoptic_empty_num_person"].sum() > 0
    for name in ("shelf", "campus"):
        p, gt, present, convert = EC.actor_golden(name)
        r = EC.records(name, ("mpjpe", "pred_index", "parts", "valid_count"))
        assert p.shape[:2] == (5, 5) and gt.shape[1] == 4 and not present.all() and present.any()
        assert _same(p[1, 0], p[1, 2]) and 2 not in r["pred_index"][1]                   # identical: the first
        assert np.isnan(p[2, 1, :, :3]).any() and np.isnan(r["mpjpe"][2][present[2]]).all()
        assert ((r["valid_count"] == 0).any()) == (name == "campus")
    masks = {int(EC.records(f"shelf_limbs{n}", ("parts",))["parts"][0, 0]) for n in range(4)}
    assert len(masks) == 4 and 0x3FF in masks                                            # distinct limb decisions


@pytest.mark.parametrize("name", EC.PANOPTIC_CASES)
def test_host_scoring_of_panoptic_records_is_the_reference(name):
    from fvp import evaluate as V

    g = EC.golden()
    _, _, _, count = EC.panoptic_golden(name)
    gt = V.PanopticGroundTruth.from_db(EC.db_of(*EC.panoptic_golden(name)[1:]))
    assert gt.total_gt == int(count.sum()) and np.array_equal(gt.prefix, np.cumsum(count) - count)
    assert gt.joints.dtype == torch.float64 and gt.vis.dtype == torch.uint8 and gt.num_person.dtype == torch.int32
    rec = EC.records(name, ("mpjpe", "gt_index", "score"))
    metric, msg = V.score_panoptic(rec["mpjpe"], rec["gt_index"], rec["score"], gt.prefix, gt.total_gt)
    want = str(g[f"{name}_msg"])
    assert msg == want                                   # every AP, the recall and the MPJPE as printed
    assert float(metric) == float(g[f"{name}_metric"])   # the mean AP exactly
    # mpjpe@500mm itself: within len * 2^-53 relative of the reference's mean
    items = [tuple(r) for r in g[f"{name}_eval_list"]]
    ref_mean = E.matched_mpjpe(items)
    if np.isfinite(ref_mean):
        order = np.argsort(-rec["score"][rec["gt_index"] >= 0].astype(np.float64), kind="stable")
        m = rec["mpjpe"][rec["gt_index"] >= 0][order]
        gid = (gt.prefix[:, None] + rec["gt_index"])[rec["gt_index"] >= 0][order]
        kept = m[V._first_hits(m < 500, gid)]
        assert abs(np.mean(kept) - ref_mean) <= len(kept) * 2.0 ** -53 * ref_mean
    else:
        assert msg.endswith("mpjpe@500mm: inf")


def test_host_scoring_keeps_equal_scores_in_frame_slot_order():
    """Two records of one person with equal scores: the earlier (frame, slot) one is the true positive."""
    from fvp import evaluate as V

    mpjpe = np.array([[140.0, 30.0]])
    for scores in ([0.5, 0.5], [0.5, 0.6]):
        items = [(140.0, scores[0], 0), (30.0, scores[1], 0)]
        want = E.score_items(items, 1)
        got = V.score_panoptic(mpjpe, np.zeros((1, 2), np.int32), np.array([scores], np.float32), np.zeros(1), 1)
        assert (float(got[0]), got[1]) == (float(want[0]), want[1])
        # nothing is under 25 mm; at 150 mm whichever record sorts first is the person's one true positive
        assert "ap@25: 0.0000" in got[1] and "ap@150: 1.0000" in got[1]


@pytest.mark.parametrize("name", EC.ACTOR_CASES)
def test_host_scoring_of_actor_records_is_the_reference(name):
    from fvp import evaluate as V

    g = EC.golden()
    rec = EC.records(name, ("mpjpe", "pred_index", "parts", "valid_count"))
    metric, msg = V.score_pcp(rec["mpjpe"], rec["pred_index"], rec["parts"], rec["valid_count"],
                              int(g[f"{name}_convert"]))
    assert (float(metric), msg) == (float(g[f"{name}_metric"]), str(g[f"{name}_msg"]))


def test_shelf_scoring_raises_on_a_frame_without_a_valid_prediction():
    from fvp import evaluate as V

    rec = EC.records("campus", ("mpjpe", "pred_index", "parts", "valid_count"))
    frame = int(np.nonzero(rec["valid_count"] == 0)[0][0])
    with pytest.raises(ValueError, match=f"frame {frame}"):
        V.score_pcp(rec["mpjpe"], rec["pred_index"], rec["parts"], rec["valid_count"], V.SHELF)
    with pytest.raises(ValueError, match=f"frame {frame}"):
        E.pcp(*EC.actor_golden("campus")[:3], E.SHELF)


def test_actor_ground_truth_from_the_mat_cells():
    from fvp import evaluate as V

    g = EC.golden()
    gt = V.ActorGroundTruth.from_actor3d(EC.actor3d_of("shelf"), g["shelf_frame_range"])
    assert gt.joints.dtype == torch.float64 and gt.present.dtype == torch.uint8
    assert np.array_equal(gt.present.numpy(), g["shelf_present"])
    assert np.array_equal(gt.joints.numpy()[g["shelf_present"] > 0], g["shelf_gt"][g["shelf_present"] > 0])


def test_load_actor3d_unwraps_the_mat(tmp_path):
    from fvp.integration import load_actor3d

    cells = EC.actor3d_of("campus")
    EC.write_actors_mat(str(tmp_path / "actorsGT.mat"), cells)
    got = load_actor3d(str(tmp_path / "actorsGT.mat"))
    assert got.shape == cells.shape
    for a in range(cells.shape[0]):
        for f in range(cells.shape[1]):
            assert len(got[a, f][0]) == len(cells[a, f][0])
            assert np.array_equal(np.asarray(got[a, f], np.float64).reshape(cells[a, f].shape), cells[a, f])


def test_entry_points_check_their_arguments_without_a_device():
    from fvp import _lib

    lib = _lib.load()
    mp, ma = lib.fvp_match_poses, lib.fvp_match_actors
    # (preds, N, K, J, C, gt, gt_vis, num_person, G, mpjpe, gt_index, score, stream)
    good = [8, 2, 3, 15, 5, 8, 8, 8, 4, 8, 8, 8, None]
    for at in (0, 5, 6, 7, 9, 10, 11):
        args = list(good)
        args[at] = None
        assert mp(*args) == 1001, at
    for at, bad in ((1, -1), (2, 0), (2, -3), (3, 0), (3, 1025), (4, 4), (4, 0), (4, 65), (8, 0), (8, -1)):
        args = list(good)
        args[at] = bad
        assert mp(*args) == 1002, (at, bad)
    assert mp(8, 2, 65, 15, 5, 8, 8, 8, 64, 8, 8, 8, None) == 1002   # K * G over FVP_EVAL_MAX_PAIRS
    assert mp(8, 0, 64, 1024, 64, 8, 8, 8, 64, 8, 8, 8, None) == 0   # the caps themselves are inside (no frames)
    assert mp(8, 0, 3, 15, 5, 8, 8, 8, 4, 8, 8, 8, None) == 0        # no frames: success, no launch
    assert mp(None, 0, 3, 15, 5, 8, 8, 8, 4, 8, 8, 8, None) == 1001  # ... after the pointer check
    # (preds, N, K, C, gt, present, A, convert, mpjpe, pred_index, parts, valid_count, stream)
    good = [8, 2, 3, 5, 8, 8, 4, 0, 8, 8, 8, 8, None]
    for at in (0, 4, 5, 8, 9, 10, 11):
        args = list(good)
        args[at] = None
        assert ma(*args) == 1001, at
    for at, bad in ((1, -1), (2, 0), (2, 65), (3, 4), (3, 65), (6, 0), (6, 33), (7, -1), (7, 2)):
        args = list(good)
        args[at] = bad
        assert ma(*args) == 1002, (at, bad)
    assert ma(8, 0, 64, 5, 8, 8, 32, 1, 8, 8, 8, 8, None) == 0       # the caps themselves are inside


def test_cpu_predictions_are_refused():
    from fvp import _lib
    from fvp import evaluate as V

    gt = V.PanopticGroundTruth.from_db(EC.db_of(*EC.panoptic_golden("panoptic")[1:]))
    with pytest.raises(_lib.FvpError, match="HIP device"):
        V.panoptic(torch.from_numpy(EC.panoptic_golden("panoptic")[0]), gt)
    agt = V.ActorGroundTruth.from_actor3d(EC.actor3d_of("shelf"), EC.golden()["shelf_frame_range"])
    with pytest.raises(_lib.FvpError, match="HIP device"):
        V.pcp(list(torch.from_numpy(EC.actor_golden("shelf")[0])), agt, V.SHELF)


def _stand_ins():
    calls = []

    def make(name, with_threshold):
        if with_threshold:
            def evaluate(self, preds, recall_threshold=500):
                calls.append((name, recall_threshold))
                return 0.0, f"original {name}"
        else:
            def evaluate(self, preds):
                calls.append((name, None))
                return 0.0, f"original {name}"
        return type(name, (), {"evaluate": evaluate})

    classes = {"Panoptic": make("Panoptic", False), "Shelf": make("Shelf", True), "Campus": make("Campus", True)}
    mods = {f"dataset.{n.lower()}": types.SimpleNamespace(**{n: c}) for n, c in classes.items()}
    return classes, mods, calls


def test_install_patches_the_three_evaluate_methods_only_when_asked():
    from fvp import integration

    classes, mods, calls = _stand_ins()
    originals = {n: c.evaluate for n, c in classes.items()}
    assert integration.install(modules=mods) == {}                 # the default: nothing of these is touched
    assert all(c.evaluate is originals[n] and not hasattr(c, "_fvp_original_evaluate") for n, c in classes.items())
    patched = integration.install(modules=mods, evaluate=True)
    assert sorted(patched) == ["dataset.campus.Campus.evaluate", "dataset.panoptic.Panoptic.evaluate",
                               "dataset.shelf.Shelf.evaluate"]
    for n, c in classes.items():
        assert c._fvp_original_evaluate is originals[n] and c.evaluate is patched[f"dataset.{n.lower()}.{n}.evaluate"]
    integration.install(modules=mods, evaluate=True)               # again: the original stays the original
    assert all(c._fvp_original_evaluate is originals[n] for n, c in classes.items())
    # a CPU preds goes to the original method, arguments and all
    cpu = torch.zeros((2, 3, 15, 5))
    assert classes["Panoptic"]().evaluate(cpu) == (0.0, "original Panoptic")
    assert classes["Shelf"]().evaluate(cpu, 400) == (0.0, "original Shelf")
    assert classes["Campus"]().evaluate(list(cpu)) == (0.0, "original Campus")
    assert calls == [("Panoptic", None), ("Shelf", 400), ("Campus", 500)]
    # only the importable modules are patched and listed
    classes, mods, _ = _stand_ins()
    del mods["dataset.shelf"]
    assert sorted(integration.install(modules=mods, evaluate=True)) == [
        "dataset.campus.Campus.evaluate", "dataset.panoptic.Panoptic.evaluate"]


def test_registered_op_set_is_unchanged():
    import op_cases as OC

    registered = OC.registered_ops()
    assert len(registered) == 26
    assert not [n for n in registered if "match" in n or "eval" in n]
