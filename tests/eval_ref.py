"""numpy restatement of the reference's three dataset.evaluate() methods
(lib/dataset/panoptic.py:214-312, shelf.py:162-256, campus.py:138-230), frame
loop and all: the tests' reference for fvp.evaluate and the baseline of
tools/bench_evaluate.py.  Written from the methods' behaviour; their results
on tests/golden/evaluate.npz pin it (tools/gen_evaluate_golden.py).

Besides (metric, msg) each function returns what the kernels of
csrc/fvp_eval.hip produce: per-slot records for Panoptic, per-(frame, actor)
records for Shelf / Campus, with the kernels' fill values (index -1, mpjpe
NaN, parts 0) where the reference computes nothing.

`preds` is a sequence of N frames [K, J, C]: a numpy array or a torch tensor
on any device; a tensor is brought over one frame at a time, as the reference
does (one synchronisation and one small copy per frame).
"""
import numpy as np

AP_THRESHOLDS = (25, 50, 75, 100, 125, 150)
COCO_TO_14 = (16, 14, 12, 11, 13, 15, 10, 8, 6, 5, 7, 9)
LIMBS = ((0, 1), (1, 2), (3, 4), (4, 5), (6, 7), (7, 8), (9, 10), (10, 11), (12, 13))
SHELF, CAMPUS = 0, 1

PANOPTIC_MSG = ("Evaluation results on Panoptic dataset:\nap@25: {:.4f}\tap@50: {:.4f}\tap@75: {:.4f}\t"
                "ap@100: {:.4f}\tap@125: {:.4f}\tap@150: {:.4f}\trecall@500mm: {:.4f}\tmpjpe@500mm: {:.3f}")
PCP_MSG = ("     | Actor 1 | Actor 2 | Actor 3 | Average | \n PCP |  {:.2f}  |  {:.2f}  |  {:.2f}  |  {:.2f}  |"
           "\t Recall@500mm: {:.4f}")


def _host(frame):
    return frame.detach().cpu().numpy() if hasattr(frame, "detach") else np.asarray(frame)


# -- Panoptic ------------------------------------------------------------------------

def _first_hits(items, threshold):
    """Flags, in `items` order, of the first item under `threshold` of each gt_id."""
    seen, flags = set(), []
    for mpjpe, _, gt_id in items:
        hit = mpjpe < threshold and gt_id not in seen
        if hit:
            seen.add(gt_id)
        flags.append(hit)
    return flags


def _by_score(items):
    return sorted(items, key=lambda it: it[1], reverse=True)  # stable: ties keep (frame, slot) order


def ap_recall(items, total_gt, threshold):
    items = _by_score(items)
    hit = np.array(_first_hits(items, threshold), dtype=bool)
    tp = np.cumsum(np.where(hit, 1.0, 0.0))
    fp = np.cumsum(np.where(hit, 0.0, 1.0))
    recall = tp / (total_gt + 1e-5)
    precision = tp / (tp + fp + 1e-5)
    for n in range(len(items) - 2, -1, -1):
        precision[n] = max(precision[n], precision[n + 1])
    precision = np.concatenate(([0], precision, [0]))
    recall = np.concatenate(([0], recall, [1]))
    step = np.where(recall[1:] != recall[:-1])[0]
    return np.sum((recall[step + 1] - recall[step]) * precision[step + 1]), recall[-2]


def matched_mpjpe(items, threshold=500):
    items = _by_score(items)
    kept = [it[0] for it, hit in zip(items, _first_hits(items, threshold)) if hit]
    return np.mean(kept) if kept else np.inf


def recall_at(items, total_gt, threshold=500):
    return len(np.unique([it[2] for it in items if it[0] < threshold])) / total_gt


def score_items(items, total_gt):
    """(metric, msg) of Panoptic.evaluate from its (mpjpe, score, gt_id) items in (frame, slot) order."""
    aps, recs = [], []
    for t in AP_THRESHOLDS:
        ap, rec = ap_recall(items, total_gt, t)
        aps.append(ap)
        recs.append(rec)
    msg = PANOPTIC_MSG.format(*aps, recall_at(items, total_gt), matched_mpjpe(items))
    return np.mean(aps), msg


def panoptic(preds, joints_3d, joints_3d_vis, num_person):
    """joints_3d [N, G, J, 3] fp64, joints_3d_vis [N, G, J], num_person [N].
    Returns (metric, msg, items, records): items = the (mpjpe, score, gt_id) list
    in (frame, slot) order; records = dict of mpjpe / gt_index / score [N, K]."""
    N = len(preds)
    assert N == len(num_person), "number mismatch"
    K = preds[0].shape[0] if N else 0
    rec = {"mpjpe": np.full((N, K), np.nan), "gt_index": np.full((N, K), -1, np.int32),
           "score": np.zeros((N, K), np.float32)}
    items, total_gt = [], 0
    with np.errstate(invalid="ignore"), _quiet():
        for i in range(N):
            pred = _host(preds[i])
            rec["score"][i] = pred[:, 0, 4]
            n = int(num_person[i])
            if n == 0:
                continue
            for k in np.nonzero(pred[:, 0, 3] >= 0)[0]:
                pose = pred[k]
                per_gt = []
                for g in range(n):
                    vis = joints_3d_vis[i][g] > 0.1
                    d = pose[vis, 0:3] - joints_3d[i][g][vis]
                    per_gt.append(np.sqrt((d * d).sum(axis=-1)).mean())
                best = int(np.argmin(per_gt))
                rec["mpjpe"][i, k], rec["gt_index"][i, k] = per_gt[best], best
                items.append((float(np.min(per_gt)), float(pose[0, 4]), total_gt + best))
            total_gt += n
        metric, msg = score_items(items, total_gt)
    return metric, msg, items, rec


class _quiet:
    """np.mean of an empty selection warns (and gives the NaN the reference gets)."""

    def __enter__(self):
        import warnings

        self._cm = warnings.catch_warnings()
        self._cm.__enter__()
        warnings.simplefilter("ignore", RuntimeWarning)

    def __exit__(self, *exc):
        return self._cm.__exit__(*exc)


# -- Shelf / Campus ------------------------------------------------------------------

def convert_pose(coco, convert):
    """[17, 3] (float32 from the model) -> [14, 3] float64 in the reference's mixed precision:
    the head points are expressions of the input's own dtype, the rest float64."""
    out = np.zeros((14, 3))
    out[:12] = coco[list(COCO_TO_14)]
    shoulders = (coco[5] + coco[6]) / 2
    ears = (coco[3] + coco[4]) / 2
    head_bottom = (shoulders + ears) / 2
    head_top = head_bottom + (ears - head_bottom) * 2
    if convert == CAMPUS:
        out[12], out[13] = head_bottom, head_top
        return out
    neck = (out[8] + out[9]) / 2
    top = neck + (coco[0] - neck) * np.array([0.75, 0.75, 1.5])
    neck = neck + (coco[0] - neck) * 0.5
    out[13] = top * 0.75 + head_top * 0.25
    out[12] = neck * 0.75 + head_bottom * 0.25
    return out


def part_sides(pose, gt):
    """The ten (left, right) sides of the PCP tests `left <= right` for one matched pose."""
    sides = []
    for s, e in LIMBS:
        err = np.linalg.norm(pose[s] - gt[s]) + np.linalg.norm(pose[e] - gt[e])
        sides.append((err / 2.0, 0.5 * np.linalg.norm(gt[s] - gt[e])))
    hip, gt_hip = (pose[2] + pose[3]) / 2.0, (gt[2] + gt[3]) / 2.0
    err = np.linalg.norm(hip - gt_hip) + np.linalg.norm(pose[12] - gt[12])
    sides.append((err / 2.0, 0.5 * np.linalg.norm(gt_hip - gt[12])))
    return sides


def pcp(preds, gt, present, convert, recall_threshold=500):
    """(metric, msg, records) of Shelf.evaluate (convert SHELF) / Campus.evaluate (CAMPUS); A >= 3."""
    rec, counts = match_actors(preds, gt, present, convert, recall_threshold)
    return score_pcp(*counts) + (rec,)


def match_actors(preds, gt, present, convert, recall_threshold=500):
    """gt [N, A, 14, 3] fp64 (already * 1000.0), present [N, A] bool.
    Returns (records, counts): mpjpe / pred_index / parts [N, A], valid_count [N];
    counts = (correct_parts [A], total_parts [A], match_gt, total_gt).
    Shelf raises ValueError on a frame with no valid prediction (the reference's
    np.stack of nothing); Campus skips it."""
    N, A = len(preds), gt.shape[1]
    rec = {"mpjpe": np.full((N, A), np.nan), "pred_index": np.full((N, A), -1, np.int32),
           "parts": np.zeros((N, A), np.uint32), "valid_count": np.zeros(N, np.int32)}
    correct, total = np.zeros(A), np.zeros(A)
    total_gt = match_gt = 0
    with np.errstate(invalid="ignore"):
        for i in range(N):
            pred = _host(preds[i])
            slots = np.nonzero(pred[:, 0, 3] >= 0)[0]
            rec["valid_count"][i] = len(slots)
            if len(slots) == 0:
                if convert == CAMPUS:
                    continue
                raise ValueError(f"frame {i}: no valid prediction")
            poses = np.stack([convert_pose(pred[k, :, :3], convert) for k in slots])
            for a in range(A):
                if not present[i, a]:
                    continue
                d = gt[i, a][None] - poses
                means = np.sqrt((d * d).sum(axis=-1)).mean(axis=-1)
                best = int(np.argmin(means))
                rec["mpjpe"][i, a], rec["pred_index"][i, a] = means[best], slots[best]
                match_gt += bool(np.min(means) < recall_threshold)
                total_gt += 1
                bits = 0
                for j, (left, right) in enumerate(part_sides(poses[best], gt[i, a])):
                    bits |= int(left <= right) << j
                rec["parts"][i, a] = bits
                total[a] += 10
                correct[a] += bin(bits).count("1")
    return rec, (correct, total, match_gt, total_gt)


def score_pcp(correct, total, match_gt, total_gt):
    actor_pcp = correct / (total + 1e-8)
    avg = np.mean(actor_pcp[:3])
    recall = match_gt / (total_gt + 1e-8)
    return np.mean(avg), PCP_MSG.format(actor_pcp[0] * 100, actor_pcp[1] * 100, actor_pcp[2] * 100, avg * 100, recall)
