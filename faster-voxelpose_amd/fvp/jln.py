"""JLN post-processing on the fvp kernels.

* :class:`SoftArgmaxLayer` -- drop-in for
  ``models.joint_localization_net.SoftArgmaxLayer`` (joint_localization_net.py:15-56):
  same constructor (``cfg.NETWORK.BETA``), same ``forward(x, grids) -> (x, confs)``.
* :func:`fuse_pose_preds` -- ``JointLocalizationNet.fuse_pose_preds`` (:83-120).
* :func:`fused_jln_forward` -- ``JointLocalizationNet.forward`` (:122-182) for
  every proposal of a batch at once: one per-person planes launch
  (``project_layer.forward_batch``), the P2PNet / WeightNet CNNs on all
  proposals together, the soft-argmax + offsets and the fusion as two fvp
  launches; no per-frame loop and no per-frame host sync.  Eval mode only:
  in training the CNNs' BatchNorm statistics are per frame in the reference,
  so the original per-frame forward is kept.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .heatmaps import release_shared


class SoftArgmaxLayer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.beta = cfg.NETWORK.BETA

    def forward(self, x, grids):
        """x [3,B,C,H*W,1] or [3,B,C,H,W] -> (coords [3,B,C,2], confs [B])."""
        ops.forward_only(x)
        pose, maxprob = ops.soft_argmax(x, grids, None, float(self.beta))
        C = x.shape[2]
        confs = maxprob.sum(dim=(0, 2)) / (3 * C)
        return pose, confs


def fuse_pose_preds(pose_preds, weights):
    """pose_preds [3,P,J,2], weights [3P,J,1] -> fused [P,J,3] (joint_localization_net.py:83-120)."""
    P, J = pose_preds.shape[1], pose_preds.shape[2]
    fused, _ = ops.fuse_poses(pose_preds, weights, pose_preds.new_zeros((3, P, J)))
    return fused


def fused_jln_forward(self, meta, heatmaps, proposal_centers, mask, cameras, resize_transform):
    """JointLocalizationNet.forward (joint_localization_net.py:122-182), batched.

    Same inputs and outputs: (all_fused_pose_preds [B,K,J,3],
    all_pose_preds [3,B,K,J,2]); proposal_centers[..., 4] of valid proposals is
    overwritten with the confidences, as in the reference (:180)."""
    if self.training:
        out = self._fvp_original_forward(meta, heatmaps, proposal_centers, mask, cameras, resize_transform)
        release_shared(heatmaps)
        return out
    device = heatmaps.device
    if _wants_sync_free(self):
        out = _jln_sync_free(self, meta, heatmaps, proposal_centers, mask, cameras, resize_transform)
        release_shared(heatmaps)
        return out
    B, K = proposal_centers.shape[:2]
    J = heatmaps.shape[2]
    all_fused = torch.zeros((B, K, J, 3), device=device)
    all_pose = torch.zeros((3, B, K, J, 2), device=device)
    seqs = list(meta["seq"])[:B]
    if len(set(seqs)) != 1:  # frames of several sequences: one batched call per sequence
        for s in dict.fromkeys(seqs):
            sel = torch.tensor([q == s for q in seqs], device=device)
            _jln_batch(self, meta, heatmaps, proposal_centers, mask & sel[:, None], cameras, resize_transform,
                       all_fused, all_pose, first=seqs.index(s))
    else:
        _jln_batch(self, meta, heatmaps, proposal_centers, mask, cameras, resize_transform, all_fused, all_pose,
                   first=0)
    # the HDN's one-forward channels-last copy (fvp.heatmaps.share_channels_last) ends here,
    # with its last consumer: it is not kept alive on the caller's tensor
    release_shared(heatmaps)
    return all_fused, all_pose


def _wants_sync_free(self) -> bool:
    """FvpOptions.sync_free: None = exactly under a stream capture (where the synced route's count
    read cannot run); True / False = always / never -- never, under a capture, is an error raised
    here, before anything reads the device."""
    from . import _lib, integration

    want = integration.options_of(self).sync_free
    if want:
        return True
    capturing = torch.cuda.is_current_stream_capturing()
    if want is None:
        return capturing
    if capturing:
        raise _lib.FvpError("fvp: sync_free=False under a stream capture: the synced JLN route reads the number "
                            "of valid proposals back to the host, which a capture cannot record (leave "
                            "FvpOptions.sync_free at None or set it True)")
    return False


def _jln_sync_free(self, meta, heatmaps, proposal_centers, mask, cameras, resize_transform):
    """The JLN with no host read and fixed shapes: all B*K (frame, proposal) slots go through the
    person gather (dead slots as empty windows, ProjectLayer.forward_all), P2PNet, the soft-argmax
    and WeightNet, and one launch fuses, scatters and masks them (ops.fuse_scatter_poses).  Per
    live slot every step is the synced route's arithmetic on the same values, so the outputs are
    the same bit for bit; the price is P2PNet on 3*B*K planes instead of 3*(valid proposals)."""
    from . import _lib, cnn, integration

    if not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dim() == 2 and mask.dtype == torch.bool):
        got = (f"{tuple(mask.shape)} {mask.dtype} on {mask.device}" if isinstance(mask, torch.Tensor)
               else type(mask).__name__)
        raise _lib.FvpError(f"fvp: the sync-free JLN route needs a 2-D bool device mask, got {got}")
    if (proposal_centers.dtype != torch.float32 or proposal_centers.dim() != 3 or proposal_centers.stride(2) != 1
            or tuple(proposal_centers.shape[:2]) != tuple(mask.shape)):
        raise _lib.FvpError(f"fvp: the sync-free JLN route needs fp32 proposal centres [B, K, 7] with stride(2) == 1 "
                            f"matching the mask, got {tuple(proposal_centers.shape)} {proposal_centers.dtype} strides "
                            f"{proposal_centers.stride()}")
    B = heatmaps.shape[0]
    opts = integration.options_of(self)
    use = opts.cnn and not self.conv_net.training
    conv = cnn.cached(self.conv_net, opts.cnn_dtype) if use else self.conv_net
    wnet = cnn.cached(self.weight_net) if use and not self.weight_net.training else self.weight_net
    planes, offset, _ = self.project_layer.forward_all(heatmaps, meta, proposal_centers, mask, cameras,
                                                       resize_transform)
    P = planes.shape[0] // 3                                                        # B*K, dead slots included
    J = heatmaps.shape[2]
    if P == 0:
        K = proposal_centers.shape[1]
        return (torch.zeros((B, K, J, 3), device=heatmaps.device),
                torch.zeros((3, B, K, J, 2), device=heatmaps.device))
    out = conv(planes)                                                              # [3P,J,S,S]
    features = out.reshape((3, P) + tuple(out.shape[1:]))                           # [3,P,J,S,S]
    pose, maxprob = ops.soft_argmax(features, self.project_layer.center_grid, offset,
                                    float(self.soft_argmax_layer.beta))
    weights = wnet(features)                                                        # [3P,J,1]
    if weights.dtype != torch.float32 or not weights.is_contiguous():
        weights = weights.to(torch.float32).contiguous()
    return ops.fuse_scatter_poses(mask, pose, weights, maxprob, proposal_centers, 4)


def _jln_batch(self, meta, heatmaps, proposal_centers, mask, cameras, resize_transform, all_fused, all_pose, first):
    from . import cnn, integration

    sub_meta = dict(meta)
    sub_meta["seq"] = [meta["seq"][first]] * heatmaps.shape[0]
    # the CNN wrappers' staleness checks (host work) before the sync below, while the
    # GPU still runs the HDN: after it the GPU waits for every host step
    opts = integration.options_of(self)
    use = opts.cnn and not self.conv_net.training
    conv = cnn.cached(self.conv_net, opts.cnn_dtype) if use else self.conv_net
    wnet = cnn.cached(self.weight_net) if use and not self.weight_net.training else self.weight_net
    # mask.nonzero(), its frames and the selected proposal rows in one launch: the batch's one host
    # sync (only views after it); the scatters below index with idx
    sel = None
    if (mask.is_cuda and mask.dim() == 2 and mask.dtype == torch.bool and proposal_centers.dtype == torch.float32
            and proposal_centers.dim() == 3 and proposal_centers.stride(2) == 1):
        sel = ops.mask_select(mask, proposal_centers)
        idx = sel[0]
    else:
        idx = mask.nonzero()
    planes, offset, _ = self.project_layer.forward_batch(heatmaps, sub_meta, proposal_centers, mask, cameras,
                                                         resize_transform, idx=idx, sel=sel)
    P = planes.shape[0] // 3
    if P == 0:
        return
    out = conv(planes)                                                              # [3P,J,S,S]
    # torch.stack(torch.chunk(out, 3)) of joint_localization_net.py: a view for a contiguous
    # [3P, ...] tensor (chunk k, row p = row k*P + p), no copy
    features = out.reshape((3, P) + tuple(out.shape[1:]))                           # [3,P,J,S,S]
    pose, maxprob = ops.soft_argmax(features, self.project_layer.center_grid, offset,
                                    float(self.soft_argmax_layer.beta))
    weights = wnet(features)                                                        # [3P,J,1]
    fused, confs = ops.fuse_poses(pose, weights, maxprob)
    # mask's (frame, proposal) pairs in mask order, as the boolean scatters: one launch
    # (all_fused[fi, ki] = fused; all_pose[:, fi, ki] = pose; proposal_centers[fi, ki, 4] = confs)
    if (proposal_centers.dtype == torch.float32 and proposal_centers.stride(2) == 1 and all_fused.is_contiguous()
            and all_pose.is_contiguous()):
        ops.scatter_poses(idx, fused, pose, confs, all_fused, all_pose, proposal_centers, 4)
    else:
        fi, ki = idx[:, 0], idx[:, 1]
        all_fused[fi, ki] = fused
        all_pose[:, fi, ki] = pose
        proposal_centers[fi, ki, 4] = confs
