"""uint8 camera frames as the pipeline's input.

The reference makes its network input on the CPU, one view at a time:
run/service.py:219-282, 360-366 splits a 2 x 2 mosaic frame into four views,
runs ``transforms.ToTensor()`` and ``transforms.Normalize(mean, std)`` on each,
stacks them and uploads fp32; lib/dataset/JointsDataset.py:194-199 does the
same after ``cv2.imread`` and a BGR -> RGB swap.  :class:`Frames` wraps the
uint8 tensor a camera or decoder delivers instead -- a quarter of the bytes to
upload -- and the GPU normalises it: :meth:`Frames.views` in one launch
(``fvp_frames_to_views``), or not as a pass at all where the backbone's stem
reads the frames itself (``FvpPoseResNet.heatmaps_cl_frames``).

Every route computes ``((float)b / 255.0f - mean[c]) / std[c]`` in three
rounded fp32 operations, bit for bit the CPU chain.
"""
from __future__ import annotations

import torch

from . import ops

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class Frames:
    """``Frames(data, mosaic=None | (VR, VC), swap_rb=False, mean=IMAGENET_MEAN, std=IMAGENET_STD)``

    data: uint8, per-view ``[B,V,H,W,3|4]`` or, with ``mosaic=(VR, VC)``, frames
    ``[B,VR*H,VC*W,3|4]`` holding a ``VR x VC`` grid of views (view ``r*VC + c``:
    split_frame's TL, TR, BL, BR order).  Interleaved pixels (last stride 1, pixel
    stride 3 or 4; a 4th byte is ignored); any other strides, so a cropped or
    batch-sliced tensor is read in place.  swap_rb: output channel c reads byte
    ``2 - c`` (BGR sources).  mean / std are indexed by output channel."""

    def __init__(self, data: torch.Tensor, mosaic=None, swap_rb: bool = False, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.spec, self.B, self.V, self.H, self.W = ops.frame_spec(data, mosaic, swap_rb, mean, std)
        self.data = data
        self.mosaic = tuple(int(v) for v in mosaic) if mosaic is not None else None
        self.swap_rb = bool(swap_rb)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)

    @property
    def shape(self) -> tuple:
        """The shape of views(): (B, V, 3, H, W)."""
        return (self.B, self.V, 3, self.H, self.W)

    @property
    def device(self) -> torch.device:
        return self.data.device

    @property
    def is_cuda(self) -> bool:
        return self.data.is_cuda

    def views(self) -> torch.Tensor:
        """The normalised views [B,V,3,H,W] fp32: ``fvp_frames_to_views`` on a HIP tensor,
        the reference's own torch chain on a CPU tensor."""
        if self.data.is_cuda:
            return ops.frames_to_views(self.data, list(self.mosaic or ()), self.swap_rb, list(self.mean),
                                       list(self.std))
        x = self.data
        if self.mosaic is not None:  # [B,VR*H,VC*W,P] -> [B,VR,VC,H,W,P]
            VR, VC = self.mosaic
            x = x.unflatten(1, (VR, self.H)).unflatten(3, (VC, self.W)).permute(0, 1, 3, 2, 4, 5)
            x = x.reshape(self.B, self.V, self.H, self.W, x.shape[-1])
        x = x[..., :3]
        if self.swap_rb:
            x = x.flip(-1)
        mean = torch.tensor(self.mean, dtype=torch.float32)[:, None, None]
        std = torch.tensor(self.std, dtype=torch.float32)[:, None, None]
        # ToTensor (HWC uint8 -> CHW, / 255) then Normalize, on all views at once
        return x.permute(0, 1, 4, 2, 3).contiguous().float().div(255).sub_(mean).div_(std)
