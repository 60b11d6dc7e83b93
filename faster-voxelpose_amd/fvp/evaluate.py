"""Scoring a run: the reference's dataset.evaluate() with its per-frame loop on the device.

The reference scores ``all_fused_poses`` (lib/core/function.py:181) in a Python
loop over every frame: one ``preds[i].detach().cpu()`` (a device
synchronisation and a small copy) per frame, then a chain of small numpy calls
per predicted pose and ground-truth person (lib/dataset/panoptic.py:214-265,
shelf.py:162-227, campus.py:138-209).  Here the matching of ALL frames is one
launch (csrc/fvp_eval.hip: fvp_match_poses / fvp_match_actors), its small
per-slot / per-actor records come to the host in one copy, and the scoring
(AP, recall, MPJPE, PCP) runs on them in vectorised numpy float64 with the
reference's own operation order, so the counts are the reference's and the
message is its format string byte for byte.

    gt = PanopticGroundTruth.from_db(dataset.db).to(preds.device)      # once per dataset
    metric, msg = panoptic(all_fused_poses, gt)

    gt = ActorGroundTruth.from_actor3d(actor_3d, dataset.frame_range).to(preds.device)
    metric, msg = pcp(all_fused_poses, gt, SHELF)

fvp.integration.install(evaluate=True) patches the three dataset classes to
do this.  Distances are float64 sums in index order where numpy sums pairwise
and its norms go through BLAS: values agree with the reference to a few ulp,
and every count agrees wherever a decision's margin is above that.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _lib

SHELF, CAMPUS = 0, 1
AP_THRESHOLDS = (25, 50, 75, 100, 125, 150)

PANOPTIC_MSG = ("Evaluation results on Panoptic dataset:\nap@25: {:.4f}\tap@50: {:.4f}\tap@75: {:.4f}\t"
                "ap@100: {:.4f}\tap@125: {:.4f}\tap@150: {:.4f}\trecall@500mm: {:.4f}\tmpjpe@500mm: {:.3f}")
PCP_MSG = ("     | Actor 1 | Actor 2 | Actor 3 | Average | \n PCP |  {:.2f}  |  {:.2f}  |  {:.2f}  |  {:.2f}  |"
           "\t Recall@500mm: {:.4f}")


@dataclasses.dataclass
class PanopticGroundTruth:
    """The ground truth of a Panoptic db, stacked once: joints [N, G, J, 3] fp64,
    vis [N, G, J] uint8 (joints_3d_vis > 0.1), num_person [N] int32 (tensors; to()
    moves them), and on the host prefix [N] -- the people of all earlier frames,
    the reference's running total_gt -- and total_gt."""
    joints: torch.Tensor
    vis: torch.Tensor
    num_person: torch.Tensor
    prefix: np.ndarray
    total_gt: int

    @classmethod
    def from_db(cls, db) -> "PanopticGroundTruth":
        metas = [rec["meta"] for rec in db]
        joints = np.stack([np.asarray(m["joints_3d"], np.float64) for m in metas])
        vis = np.stack([np.asarray(m["joints_3d_vis"]) > 0.1 for m in metas])
        if vis.ndim == joints.ndim:  # a per-coordinate flag: the reference indexes joints with it as one
            raise _lib.FvpError(f"fvp: joints_3d_vis must be [G, J] per frame, got {vis.shape[1:]}")
        count = np.array([int(m["num_person"]) for m in metas], np.int64)
        if count.size and (count.min() < 0 or count.max() > joints.shape[1]):
            raise _lib.FvpError("fvp: num_person outside [0, max_people]")
        prefix = np.cumsum(count) - count
        return cls(torch.from_numpy(joints), torch.from_numpy(vis.astype(np.uint8)),
                   torch.from_numpy(count.astype(np.int32)), prefix, int(count.sum()))

    def to(self, device) -> "PanopticGroundTruth":
        return dataclasses.replace(self, joints=self.joints.to(device), vis=self.vis.to(device),
                                   num_person=self.num_person.to(device))


@dataclasses.dataclass
class ActorGroundTruth:
    """actorsGT.mat of Shelf / Campus over a frame range: joints [N, A, 14, 3] fp64
    (* 1000.0; zeros where absent) and present [N, A] uint8."""
    joints: torch.Tensor
    present: torch.Tensor

    @classmethod
    def from_actor3d(cls, actor_3d, frame_range) -> "ActorGroundTruth":
        """actor_3d: the object array [A][frames] the reference makes of
        scio.loadmat(...)['actor3D'] (shelf.py:164-165); an actor is present in a
        frame iff len(gt[0]) != 0 (:183)."""
        frames, A = list(frame_range), len(actor_3d)
        joints = np.zeros((len(frames), A, 14, 3))
        present = np.zeros((len(frames), A), np.uint8)
        for a in range(A):
            for i, fi in enumerate(frames):
                gt = actor_3d[a][fi] * 1000.0
                if len(gt[0]) != 0:
                    joints[i, a], present[i, a] = gt, 1
        return cls(torch.from_numpy(joints), torch.from_numpy(present))

    def to(self, device) -> "ActorGroundTruth":
        return dataclasses.replace(self, joints=self.joints.to(device), present=self.present.to(device))


def _preds(preds, frames: int, joints: int) -> torch.Tensor:
    if isinstance(preds, (list, tuple)):
        preds = torch.stack(list(preds)) if len(preds) else torch.empty((0, 1, joints, 5))
    if preds.device.type != "cuda":
        raise _lib.FvpError(f"fvp: preds must be on a HIP device, got {preds.device}")
    p = preds.detach().to(torch.float32).contiguous()
    if p.dim() != 4 or p.shape[2] != joints or p.shape[3] < 5:
        raise _lib.FvpError(f"fvp: preds must be [N, K, {joints}, C >= 5], got {tuple(p.shape)}")
    if p.shape[0] != frames:
        raise ValueError(f"number mismatch: {p.shape[0]} frames of predictions, {frames} of ground truth")
    return p


def _same_device(p: torch.Tensor, *tensors) -> None:
    for t in tensors:
        if t.device != p.device:
            raise _lib.FvpError(f"fvp: ground truth must be on the predictions' HIP device {p.device}, got "
                                f"{t.device} (use .to(device))")


def _stream(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def match_poses(preds, gt: PanopticGroundTruth) -> dict:
    """One fvp_match_poses launch over all frames; the [N, K] records mpjpe (fp64),
    gt_index (int32) and score (fp32) as numpy arrays (one copy to the host)."""
    G, J = gt.joints.shape[1], gt.joints.shape[2]
    p = _preds(preds, gt.joints.shape[0], J)
    _same_device(p, gt.joints, gt.vis, gt.num_person)
    N, K, _, C = p.shape
    mpjpe = torch.empty((N, K), dtype=torch.float64, device=p.device)
    idx = torch.empty((N, K), dtype=torch.int32, device=p.device)
    score = torch.empty((N, K), dtype=torch.float32, device=p.device)
    if N:
        _lib.call("fvp_match_poses", p.data_ptr(), N, K, J, C, gt.joints.data_ptr(), gt.vis.data_ptr(),
                  gt.num_person.data_ptr(), G, mpjpe.data_ptr(), idx.data_ptr(), score.data_ptr(), _stream(p))
    return _to_host(mpjpe=mpjpe, gt_index=idx, score=score)


def match_actors(preds, gt: ActorGroundTruth, convert: int) -> dict:
    """One fvp_match_actors launch over all frames; the records mpjpe (fp64),
    pred_index (int32), parts (uint32) [N, A] and valid_count (int32) [N] as numpy arrays."""
    if convert not in (SHELF, CAMPUS):
        raise ValueError(f"convert must be SHELF (0) or CAMPUS (1), got {convert!r}")
    A = gt.joints.shape[1]
    p = _preds(preds, gt.joints.shape[0], 17)
    _same_device(p, gt.joints, gt.present)
    N, K, _, C = p.shape
    mpjpe = torch.empty((N, A), dtype=torch.float64, device=p.device)
    idx = torch.empty((N, A), dtype=torch.int32, device=p.device)
    parts = torch.empty((N, A), dtype=torch.int32, device=p.device)  # the kernel's uint32 bits
    valid = torch.empty((N,), dtype=torch.int32, device=p.device)
    if N:
        _lib.call("fvp_match_actors", p.data_ptr(), N, K, C, gt.joints.data_ptr(), gt.present.data_ptr(), A,
                  int(convert), mpjpe.data_ptr(), idx.data_ptr(), parts.data_ptr(), valid.data_ptr(), _stream(p))
    rec = _to_host(mpjpe=mpjpe, pred_index=idx, parts=parts, valid_count=valid)
    rec["parts"] = rec["parts"].view(np.uint32)
    return rec


def _to_host(**records) -> dict:
    """The records in ONE device-to-host copy (and one synchronisation): packed as bytes on the device."""
    names = list(records)
    flat = torch.cat([records[n].reshape(-1).view(torch.uint8) for n in names]).cpu().numpy()
    out, at = {}, 0
    for n in names:
        t = records[n]
        nbytes = t.numel() * t.element_size()
        dtype = {torch.float64: np.float64, torch.float32: np.float32, torch.int32: np.int32}[t.dtype]
        out[n] = flat[at:at + nbytes].view(dtype).reshape(tuple(t.shape))
        at += nbytes
    return out


# -- host scoring (numpy float64, the reference's operation order) -----------------------

def _first_hits(under: np.ndarray, gt_id: np.ndarray) -> np.ndarray:
    """Flags of the items that are `under` and the first such of their gt_id, in array order."""
    hit = np.zeros(under.shape, bool)
    where = np.nonzero(under)[0]
    if where.size:
        _, first = np.unique(gt_id[where], return_index=True)
        hit[where[first]] = True
    return hit


def score_panoptic(mpjpe, gt_index, score, prefix, total_gt: int):
    """(metric, msg) of Panoptic.evaluate from the [N, K] records: exactly
    _eval_list_to_ap / _eval_list_to_mpjpe / _eval_list_to_recall
    (panoptic.py:247-312) on the records in (frame, slot) order."""
    keep = np.asarray(gt_index) >= 0  # row-major: (frame, slot) order
    m = np.asarray(mpjpe, np.float64)[keep]
    s = np.asarray(score)[keep].astype(np.float64)
    gt_id = (np.asarray(prefix, np.int64)[:, None] + gt_index)[keep]
    order = np.argsort(-s, kind="stable")  # descending, ties in (frame, slot) order
    m, gt_id = m[order], gt_id[order]
    aps = []
    for t in AP_THRESHOLDS:
        hit = _first_hits(m < t, gt_id)
        tp = np.cumsum(np.where(hit, 1.0, 0.0))
        fp = np.cumsum(np.where(hit, 0.0, 1.0))
        recall = tp / (total_gt + 1e-5)
        precise = tp / (tp + fp + 1e-5)
        precise = np.maximum.accumulate(precise[::-1])[::-1]  # right-to-left running maximum
        precise = np.concatenate(([0], precise, [0]))
        recall = np.concatenate(([0], recall, [1]))
        index = np.where(recall[1:] != recall[:-1])[0]
        aps.append(np.sum((recall[index + 1] - recall[index]) * precise[index + 1]))
    matched = m[_first_hits(m < 500, gt_id)]
    mean_mpjpe = np.mean(matched) if matched.size else np.inf
    recall500 = len(np.unique(gt_id[m < 500])) / total_gt
    return np.mean(aps), PANOPTIC_MSG.format(*aps, recall500, mean_mpjpe)


def score_pcp(mpjpe, pred_index, parts, valid_count, convert: int, recall_threshold=500):
    """(metric, msg) of Shelf.evaluate / Campus.evaluate from the [N, A] records
    (shelf.py:167-227): the counts, the mean over the first three actors, the 1e-8 terms."""
    empty = np.nonzero(np.asarray(valid_count) == 0)[0]
    if convert == SHELF and empty.size:
        raise ValueError(f"frame {int(empty[0])}: no valid prediction (Shelf.evaluate stacks the frame's "
                         f"predictions and raises on none; Campus skips the frame)")
    matched = np.asarray(pred_index) >= 0  # present actors of frames with a valid prediction
    if matched.shape[1] < 3:
        raise ValueError(f"PCP is reported over the first three actors; the ground truth has {matched.shape[1]}")
    total_gt = int(matched.sum())
    match_gt = int((np.asarray(mpjpe)[matched] < recall_threshold).sum())
    bits = np.asarray(parts).astype(np.uint32) & np.uint32(0x3FF)
    popcount = sum(((bits >> np.uint32(j)) & np.uint32(1)).astype(np.int64) for j in range(10))
    total_parts = 10.0 * matched.sum(axis=0)
    correct_parts = np.where(matched, popcount, 0).sum(axis=0).astype(np.float64)
    actor_pcp = correct_parts / (total_parts + 1e-8)
    avg_pcp = np.mean(actor_pcp[:3])
    recall = match_gt / (total_gt + 1e-8)
    msg = PCP_MSG.format(actor_pcp[0] * 100, actor_pcp[1] * 100, actor_pcp[2] * 100, avg_pcp * 100, recall)
    return np.mean(avg_pcp), msg


def panoptic(preds, gt: PanopticGroundTruth):
    """Panoptic.evaluate(preds) -> (metric, msg): preds [N, K, J, C >= 5] on the HIP
    device (or a sequence of N frames), x y z / valid flag at [.., 0, 3] / score at
    [.., 0, 4]; `gt` on the same device.  A CPU `preds` raises FvpError.

    NaN scores are outside the contract: the reference sorts its records by
    score with Python's comparison sort, whose order with a NaN key is
    undefined.  (A NaN coordinate or valid flag is inside it.)"""
    rec = match_poses(preds, gt)
    return score_panoptic(rec["mpjpe"], rec["gt_index"], rec["score"], gt.prefix, gt.total_gt)


def pcp(preds, gt: ActorGroundTruth, convert: int, recall_threshold=500):
    """Shelf.evaluate (convert=SHELF) / Campus.evaluate (CAMPUS) -> (metric, msg):
    preds [N, K, 17, C >= 5] on the HIP device, one frame per entry of the ground
    truth's frame range.  A frame with no valid prediction is skipped for Campus
    (campus.py:156) and raises ValueError naming the frame for Shelf."""
    rec = match_actors(preds, gt, convert)
    return score_pcp(rec["mpjpe"], rec["pred_index"], rec["parts"], rec["valid_count"], convert, recall_threshold)
