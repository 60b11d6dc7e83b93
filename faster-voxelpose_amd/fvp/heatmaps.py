"""Channels-last heatmaps: the layout the voxelize and person gathers read.

The reference's heatmaps are ``[B, V, J, H, W]`` (one plane per joint).  The
fvp backbone (fvp.backbone) writes them channels-last, ``[B, V, H, W, Cp]``
with the J joints in channels 0..J-1 -- one 64-B pixel holds every joint of a
bilinear tap -- so the gathers read them in place instead of re-laying them
out first (fvp_voxelize_cl).  A :class:`ChannelsLastHeatmaps` can travel
through the reference's interfaces attached to the planar tensor it equals
(:func:`attach`), because those interfaces take a plain tensor.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib


class ChannelsLastHeatmaps:
    """Heatmaps [B, V, J, H, W] stored as ``t`` = [B, V, H, W, Cp] fp32 (Cp >= J),
    or fp16 with Cp % 8 == 0 and a 16-B aligned base: a 16-joint pixel is then
    32 B and the gathers read 8 joints per 16-B lane load (fvp_voxelize_cl_f16;
    the results are those of the fp16-rounded values computed in fp32)."""

    def __init__(self, t: torch.Tensor, num_joints: int):
        if t.dim() != 5 or t.dtype not in (torch.float32, torch.float16) or not t.is_contiguous() \
                or t.shape[4] < num_joints:
            raise _lib.FvpError(f"fvp: channels-last heatmaps must be contiguous fp32 / fp16 [B,V,H,W,Cp>=J], got "
                                f"{tuple(t.shape)} {t.dtype}")
        if t.dtype == torch.float16 and (t.shape[4] % 8 or t.data_ptr() % 16):
            raise _lib.FvpError(f"fvp: fp16 channels-last heatmaps need Cp % 8 == 0 and a 16-B aligned base, got "
                                f"{tuple(t.shape)} {t.dtype} at offset {t.data_ptr() % 16} mod 16")
        self.t, self.J = t, int(num_joints)

    @property
    def dtype(self) -> torch.dtype:
        return self.t.dtype

    def half(self) -> "ChannelsLastHeatmaps":
        """The fp16 copy of an fp32 object (Cp kept when a multiple of 8, else rounded up
        with zero channels); self if already fp16."""
        if self.t.dtype == torch.float16:
            return self
        cp = self.cp
        if cp % 8 == 0:
            return ChannelsLastHeatmaps(self.t.half(), self.J)
        t = torch.zeros(self.t.shape[:4] + (8 * ((cp + 7) // 8),), dtype=torch.float16, device=self.t.device)
        t[..., :cp] = self.t
        return ChannelsLastHeatmaps(t, self.J)

    @property
    def shape(self) -> tuple:
        B, V, H, W, _ = self.t.shape
        return (B, V, self.J, H, W)

    @property
    def device(self):
        return self.t.device

    @property
    def cp(self) -> int:
        return self.t.shape[4]

    def planar(self) -> torch.Tensor:
        """[B, V, J, H, W] in this object's dtype (the reference layout), carrying this
        object (attach)."""
        B, V, J, H, W = self.shape
        if self.t.dtype == torch.float16:  # (tensor-typed interfaces only: the gathers read self.t)
            return attach(self.t[..., :J].permute(0, 1, 4, 2, 3).contiguous(), self)
        out = torch.empty((B, V, J, H, W), dtype=torch.float32, device=self.t.device)
        if out.numel():
            from .ops import _ptr, _stream
            _lib.call("fvp_nhwc_to_nchw", _ptr(self.t), B * V, J, H, W, self.cp, _ptr(out), _stream(out))
        return attach(out, self)


def attach(planar: torch.Tensor, cl: ChannelsLastHeatmaps, shared: bool = False) -> torch.Tensor:
    """Mark `planar` (the same values in the reference layout) as also held
    channels-last.  Only this tensor object carries the mark: any op on it
    (view, stack, slice, in-place write) yields a tensor without it, so a
    consumer never reads a stale copy through the mark.  `shared`: the mark is
    a fused HDN's one-forward layout (share_channels_last), never reused by a
    later HDN call and dropped by the JLN that consumes it (release)."""
    if tuple(planar.shape) != cl.shape:
        raise _lib.FvpError(f"fvp: planar {tuple(planar.shape)} and channels-last {cl.shape} heatmaps differ")
    planar._fvp_cl = (cl, planar._version, bool(shared))
    return planar


def channels_last_of(heatmaps, reuse_shared: bool = True) -> ChannelsLastHeatmaps | None:
    """The channels-last copy of `heatmaps`, if it is one or carries one still valid
    (reuse_shared=False: not a copy an earlier share_channels_last made)."""
    if isinstance(heatmaps, ChannelsLastHeatmaps):
        return heatmaps
    mark = getattr(heatmaps, "_fvp_cl", None)
    if mark is None or mark[1] != heatmaps._version:  # written in place since: stale
        return None
    if mark[2] and not reuse_shared:
        return None
    return mark[0]


def release(heatmaps) -> None:
    """Drop the channels-last copy `heatmaps` carries (its memory goes with it)."""
    if isinstance(heatmaps, torch.Tensor) and getattr(heatmaps, "_fvp_cl", None) is not None:
        del heatmaps._fvp_cl


def release_shared(heatmaps) -> None:
    """Drop the copy only if share_channels_last made it (the JLN, its last consumer)."""
    mark = getattr(heatmaps, "_fvp_cl", None) if isinstance(heatmaps, torch.Tensor) else None
    if mark is not None and mark[2]:
        del heatmaps._fvp_cl


def to_channels_last(planar: torch.Tensor, dtype: torch.dtype | None = None) -> ChannelsLastHeatmaps:
    """[B, V, J, H, W] fp32 on a HIP device -> its channels-last copy
    [B, V, H, W, 16 * ceil(J / 16)] (J <= 32), one float4 layout launch
    (fvp_nchw_to_nhwc: the voxelize layout pass over the whole batch).

    dtype=torch.float16: planar fp32 or fp16 -> the fp16 channels-last copy
    (fvp_nchw_to_nhwc_f16: fp32 values rounded to nearest even as
    ``Tensor.half()``, 16-B stores, any J) -- the opt-in to the fp16 gathers."""
    from .ops import _ptr, _stream

    if dtype is not None:
        if dtype != torch.float16:
            raise _lib.FvpError(f"fvp: to_channels_last: dtype must be None or torch.float16, got {dtype}")
        if planar.dim() != 5 or planar.dtype not in (torch.float32, torch.float16) or planar.device.type != "cuda":
            raise _lib.FvpError(f"fvp: to_channels_last(dtype=float16) takes fp32 / fp16 [B,V,J,H,W] on a HIP "
                                f"device, got {tuple(planar.shape)} {planar.dtype} {planar.device}")
        B, V, J, H, W = planar.shape
        cp = 16 * ((J + 15) // 16)
        src = planar.contiguous()
        t = torch.empty((B, V, H, W, cp), dtype=torch.float16, device=planar.device)
        if t.numel():
            _lib.call("fvp_nchw_to_nhwc_f16", _ptr(src), int(src.dtype == torch.float16), B * V, J, H, W, cp,
                      _ptr(t), _stream(t))
        return ChannelsLastHeatmaps(t, J)
    if planar.dim() != 5 or planar.dtype != torch.float32 or planar.device.type != "cuda":
        raise _lib.FvpError(f"fvp: to_channels_last takes fp32 [B,V,J,H,W] on a HIP device, got "
                            f"{tuple(planar.shape)} {planar.dtype} {planar.device}")
    B, V, J, H, W = planar.shape
    if J > 32:
        raise _lib.FvpError(f"fvp: to_channels_last: {J} joints (at most 32 per pixel)")
    cp = 16 * ((J + 15) // 16)
    src = planar.contiguous()
    t = torch.empty((B, V, H, W, cp), dtype=torch.float32, device=planar.device)
    if t.numel():
        _lib.call("fvp_nchw_to_nhwc", _ptr(src), B * V, J, H, W, cp, _ptr(t), _stream(t))
    return ChannelsLastHeatmaps(t, J)


def share_channels_last(heatmaps, dtype: torch.dtype | None = None) -> ChannelsLastHeatmaps | None:
    """Lay `heatmaps` out channels-last once and attach the copy (the fused
    HDN forward does this so that the JLN, handed the same tensor object,
    reads the same copy, then drops it: release_shared): planar fp32 tensors of
    <= 32 joints on a HIP device.  A copy attached by the backbone path is used
    as it is; one left by an earlier call of this function is NOT -- the caller
    may have refilled the same buffer through ``.data``, DLPack or the C ABI,
    which do not move ``_version`` -- so every fused forward lays out anew.
    dtype=torch.float16 (FvpOptions.heatmaps_dtype): the one layout pass writes
    the fp16 copy (to_channels_last(dtype=torch.float16), half the bytes) and
    the gathers take their fp16 route; a copy already attached keeps its dtype.
    Returns the copy in use, if any."""
    if dtype not in (None, torch.float32, torch.float16):
        raise _lib.FvpError(f"fvp: share_channels_last: dtype must be None, torch.float32 or torch.float16, "
                            f"got {dtype}")
    cl = channels_last_of(heatmaps, reuse_shared=False)
    if cl is not None or not isinstance(heatmaps, torch.Tensor):
        return cl
    release(heatmaps)
    if (heatmaps.dim() != 5 or heatmaps.dtype != torch.float32 or heatmaps.device.type != "cuda"
            or heatmaps.shape[2] > 32 or heatmaps.shape[0] == 0
            or (torch.is_grad_enabled() and heatmaps.requires_grad)):
        return None
    cl = to_channels_last(heatmaps, dtype=torch.float16 if dtype == torch.float16 else None)
    attach(heatmaps, cl, shared=True)
    return cl


def pack_keypoints(all_preds, max_people: int | None = None):
    """One frame's 2-D detections as the reference dataset holds them -- a list
    over views of lists of ``[J, >= 2]`` arrays (x, y in image pixels after the
    resize transform; a score column is ignored, as generate_input_heatmap
    ignores it) -- as padded host tensors for :func:`render_keypoints`:
    ``joints`` [V, P, J, 2] fp64 and ``count`` [V] int32, with P =
    ``max_people`` or the largest view (at least 1).  Padded rows are zero and
    never read.  Batches are stacked by the caller (``torch.stack``)."""
    import numpy as np

    views = [[np.asarray(p, dtype=np.float64) for p in view] for view in all_preds]
    people = [p for view in views for p in view]
    if not views:
        raise _lib.FvpError("fvp: pack_keypoints: no views")
    for p in people:
        if p.ndim != 2 or p.shape[1] < 2 or p.shape[0] != people[0].shape[0]:
            raise _lib.FvpError(f"fvp: pack_keypoints: each person is [J, >= 2] with one J, got {p.shape}")
    most = max(len(view) for view in views)
    P = max(most, 1) if max_people is None else int(max_people)
    if most > P:
        raise _lib.FvpError(f"fvp: pack_keypoints: a view holds {most} people, max_people = {P}")
    if not people:
        raise _lib.FvpError("fvp: pack_keypoints: no person in any view (the joint count is unknown)")
    J = people[0].shape[0]
    joints = np.zeros((len(views), P, J, 2), dtype=np.float64)
    for v, view in enumerate(views):
        for n, p in enumerate(view):
            joints[v, n] = p[:, :2]
    count = np.array([len(view) for view in views], dtype=np.int32)
    return torch.from_numpy(joints), torch.from_numpy(count)


class Augmentation(NamedTuple):
    """The random draws of generate_input_heatmap with ``data_augmentation = True``, one record per
    joint (:func:`draw_augmentation`): ``scale`` [..., P, J] fp32, the factor a joint's patch is
    multiplied by, and ``rect`` [..., P, J, 4] int16 = (r0, r1, c0, c1), the rows and columns of
    the patch that are zeroed.  (1, empty rectangle) is the identity."""
    scale: torch.Tensor
    rect: torch.Tensor


def _host_array(t, dtype=None):
    import numpy as np

    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t) if dtype is None else np.asarray(t, dtype=dtype)


def _trunc(v) -> int:
    """Python's int(), pinned to +-2^30 as the kernel pins it."""
    return int(min(max(float(v), -1073741824.0), 1073741824.0))


def draw_augmentation(joints, count, vis=None, *, image_size, heatmap_size, sigma: float, py_rng=None,
                      np_rng=None) -> Augmentation:
    """The random draws JointsDataset.generate_input_heatmap makes with
    ``data_augmentation = True`` (lib/dataset/JointsDataset.py:413-432) for one
    frame, as the records ``render_keypoints(..., augment=)`` and
    ``render_poses3d(..., augment=)`` take: host tensors ``scale`` [V, P, J] fp32
    and ``rect`` [V, P, J, 4] int16.  Use it beside :func:`pack_keypoints` in the
    dataset's ``__getitem__``; the default collate stacks the frames.

    joints  [V, P, J, 2] host tensor or array, image pixels after the resize transform
            (pack_keypoints; for ``'gt'``, the keypoints of project_poses copied to the
            host, or the dataset's own)
    count   [V] people of each view;  vis [V, P, J] or None: 0 = joint not painted
    py_rng, np_rng  a ``random.Random`` and a ``np.random.RandomState``; default: the
            global ``random`` and ``np.random`` streams the reference reads

    The streams are consumed exactly as the reference consumes them: views, then
    people, then joints; a joint that is invisible, off the map (the painter's
    skip test) or of a person with a non-finite coordinate draws nothing and gets
    the identity record; every other joint -- one whose window ends at ``br == 0``
    and paints nothing included -- draws ``random()`` (< 0.6: ``randn(1)`` follows,
    scale = 0.9 + 0.03 randn), ``random()`` again for the second factor (joints 7,
    8: x0.5 below 0.1; joints 9, 10: x0.2 below 0.1; others: x0.5 below 0.05) and
    four ``uniform`` values for the rectangle.  The window is restated in float64
    in the reference's operation order, as the kernel computes it."""
    import math
    import random

    import numpy as np

    rnd = (py_rng if py_rng is not None else random).random
    npr = np_rng if np_rng is not None else np.random
    jn = _host_array(joints)
    if jn.ndim != 4 or jn.shape[3] != 2:
        raise _lib.FvpError(f"fvp: draw_augmentation takes joints [V,P,J,2], got {jn.shape}")
    V, P, J, _ = jn.shape
    cn = _host_array(count).reshape(-1)
    if cn.shape[0] != V:
        raise _lib.FvpError(f"fvp: draw_augmentation takes count [V] = {(V,)}, got {cn.shape}")
    vn = None if vis is None else _host_array(vis)
    if vn is not None and vn.shape != (V, P, J):
        raise _lib.FvpError(f"fvp: draw_augmentation takes vis [V,P,J] = {(V, P, J)}, got {vn.shape}")
    (img_w, img_h), (W, H) = image_size, heatmap_size
    W, H = int(W), int(H)
    stride = (float(img_w) / float(W), float(img_h) / float(H))
    scale = np.ones((V, P, J), np.float32)
    rect = np.zeros((V, P, J, 4), np.int16)
    for v in range(V):
        for p in range(min(max(int(cn[v]), 0), P)):
            q = jn[v, p].astype(np.float64) / np.asarray(stride, np.float64)
            if not np.isfinite(q).all():
                continue
            ext = np.maximum(q[:, 1].max() - q[:, 1].min(), q[:, 0].max() - q[:, 0].min())
            human = 2 * np.clip(ext * ext, 1.0 / 4 * 96 ** 2, 4 * 96 ** 2)
            tmp = float(np.float64(sigma) * np.sqrt(human / (96.0 * 96.0)) * 3)
            for j in range(J):
                if vn is not None and vn[v, p, j] == 0:
                    continue
                mu_x, mu_y = _trunc(q[j, 0]), _trunc(q[j, 1])
                ul = (_trunc(mu_x - tmp), _trunc(mu_y - tmp))
                br = (_trunc(mu_x + tmp + 1), _trunc(mu_y + tmp + 1))
                if ul[0] >= W or ul[1] >= H or br[0] < 0 or br[1] < 0:
                    continue
                s = 0.9 + float(npr.randn(1)[0]) * 0.03 if rnd() < 0.6 else 1.0
                second = rnd()
                if j in (7, 8):
                    s = s * 0.5 if second < 0.1 else s
                elif j in (9, 10):
                    s = s * 0.2 if second < 0.1 else s
                else:
                    s = s * 0.5 if second < 0.05 else s
                r0 = int(npr.uniform(0, H - 1))
                c0 = int(npr.uniform(0, W - 1))
                r1 = int(min(r0 + npr.uniform(H / 4, H * 0.75), H))
                c1 = int(min(c0 + npr.uniform(W / 4, W * 0.75), W))
                scale[v, p, j] = s
                rect[v, p, j] = [min(max(x, 0), 32767) for x in (r0, r1, c0, c1)]
    return Augmentation(torch.from_numpy(scale), torch.from_numpy(rect))


def _augment_records(name: str, augment, shape: tuple, device):
    """(scale, rect) of an ``augment=`` argument as the ops take them: checked, contiguous, on `device`
    (host records, as the collate stacks them, are uploaded)."""
    try:
        scale, rect = augment
    except (TypeError, ValueError):
        scale = rect = None
    if not isinstance(scale, torch.Tensor) or not isinstance(rect, torch.Tensor) \
            or tuple(scale.shape) != shape or tuple(rect.shape) != shape + (4,) \
            or scale.dtype != torch.float32 or rect.dtype != torch.int16:
        got = [(tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t) for t in (scale, rect)]
        raise _lib.FvpError(f"fvp: {name}: augment is (scale fp32 [B,V,P,J] = {shape}, rect int16 [B,V,P,J,4]) "
                            f"(heatmaps.draw_augmentation, stacked), got {got}")
    out = []
    for t in (scale, rect):
        if t.device.type == "cpu":
            t = t.to(device)
        elif t.device != device:
            raise _lib.FvpError(f"fvp: {name}: augment must be on the host or on {device}, got {t.device}")
        out.append(t.contiguous())
    return out


def render_keypoints(joints: torch.Tensor, count: torch.Tensor, vis: torch.Tensor | None = None, *, image_size,
                     heatmap_size, sigma: float, dtype: torch.dtype | None = None,
                     augment=None) -> ChannelsLastHeatmaps:
    """Input heatmaps painted from 2-D keypoints on the device, channels-last,
    in one launch (fvp_render_keypoints): JointsDataset.generate_input_heatmap
    (lib/dataset/JointsDataset.py:368-447) with ``data_augmentation = False``,
    quirks included -- the ``TEST_HEATMAP_SRC: 'pred'`` input of Shelf and
    Campus -- without the numpy painter, the planar host-to-device copy and
    the layout pass.  The result feeds ``ProjectLayer`` directly, or as
    ``.planar()`` through the reference's tensor-typed interfaces.

    joints  [B, V, P, J, 2] fp64 or fp32 on a HIP device: image pixels after the
            dataset's resize transform (what the reference hands to the painter)
    count   [B, V] int32: people of each view (rows at or beyond it are never read)
    vis     [B, V, P, J] uint8 or bool, optional: 0 = joint not painted
    image_size, heatmap_size  (W, H) as NETWORK.IMAGE_SIZE / HEATMAP_SIZE;  sigma: NETWORK.SIGMA
    dtype   None / torch.float32, or torch.float16: the fp16 channels-last layout the
            fp16 gathers read, written by the same launch (fvp_render_keypoints_f16) --
            bit for bit ``render_keypoints(...).half()`` without the cast pass
    augment None, or the :class:`Augmentation` of :func:`draw_augmentation` stacked to
            scale [B, V, P, J] fp32 and rect [B, V, P, J, 4] int16 (on the host or on the
            operands' device): ``data_augmentation = True`` (JointsDataset.py:413-432, the
            setting of the Shelf and Campus configs) in the same launch
            (fvp_render_keypoints_aug) -- each painted joint is multiplied by its scale and
            zeroed inside its rectangle, and the result is clamped at 1

    A person with a non-finite coordinate is skipped (the reference raises).
    The ``'gt'`` source (3-D joints projected through the cameras first) is
    :func:`render_poses3d`, which projects and paints in one launch."""
    from . import ops

    if dtype not in (None, torch.float32, torch.float16):
        raise _lib.FvpError(f"fvp: render_keypoints: dtype must be None, torch.float32 or torch.float16, got {dtype}")
    if not isinstance(joints, torch.Tensor) or joints.dim() != 5 or joints.shape[4] != 2 \
            or joints.dtype not in (torch.float32, torch.float64):
        raise _lib.FvpError(f"fvp: render_keypoints takes joints fp64 / fp32 [B,V,P,J,2], got "
                            f"{tuple(joints.shape)} {joints.dtype}")
    B, V, P, J, _ = joints.shape
    if J > 32 or P > 32 or J < 1 or P < 1:
        raise _lib.FvpError(f"fvp: render_keypoints: {P} people x {J} joints (1..32 each)")
    if not isinstance(count, torch.Tensor) or tuple(count.shape) != (B, V) or count.dtype != torch.int32:
        raise _lib.FvpError(f"fvp: render_keypoints takes count int32 [B,V] = {(B, V)}, got "
                            f"{tuple(count.shape)} {count.dtype}")
    if vis is not None:
        if tuple(vis.shape) != (B, V, P, J) or vis.dtype not in (torch.uint8, torch.bool):
            raise _lib.FvpError(f"fvp: render_keypoints takes vis uint8 / bool [B,V,P,J] = {(B, V, P, J)}, got "
                                f"{tuple(vis.shape)} {vis.dtype}")
        if vis.dtype == torch.bool:
            vis = vis.view(torch.uint8)
    for name, t in (("joints", joints), ("count", count), ("vis", vis)):
        if t is None:
            continue
        if t.device.type != "cuda" or t.device != joints.device:
            raise _lib.FvpError(f"fvp: render_keypoints: {name} must be on a HIP device (one for all operands), got "
                                f"{t.device}")
        if not t.is_contiguous():
            raise _lib.FvpError(f"fvp: render_keypoints: {name} must be contiguous")
    (img_w, img_h), (W, H) = image_size, heatmap_size
    if int(W) != W or int(H) != H or W < 1 or H < 1 or not (img_w > 0 and img_h > 0 and sigma > 0):
        raise _lib.FvpError(f"fvp: render_keypoints: image {image_size}, heatmap {heatmap_size}, sigma {sigma}")
    ops.forward_only(joints)
    if augment is not None:
        scale, rect = _augment_records("render_keypoints", augment, (B, V, P, J), joints.device)
        t = ops.render_keypoints_aug(joints, count, vis, scale, rect, float(img_w), float(img_h), int(H), int(W),
                                     float(sigma), dtype == torch.float16)
        return ChannelsLastHeatmaps(t, J)
    op = ops.render_keypoints_f16 if dtype == torch.float16 else ops.render_keypoints
    t = op(joints, count, vis, float(img_w), float(img_h), int(H), int(W), float(sigma))
    return ChannelsLastHeatmaps(t, J)


def pack_poses3d(joints_3d, joints_3d_vis=None, max_people: int | None = None):
    """One frame's 3-D ground truth as the reference dataset holds it
    (``meta['joints_3d']`` / ``meta['joints_3d_vis']``, JointsDataset.py:107-117)
    -- people as ``[J, >= 3]`` arrays (x, y, z in mm) and their visibility as
    ``[J]`` arrays, or as ``[J, 3]`` arrays as Panoptic stores it -- as padded host
    tensors for :func:`render_poses3d`: ``joints3d`` [P, J, 3] fp64, ``vis3d``
    [P, J] uint8 and ``count``, a 0-d int32 tensor, with P = ``max_people`` or
    the number of people (at least 1).  The default collate stacks the three
    into [B, P, J, 3], [B, P, J] and [B].

    A joint is visible where its flag is > 0 (JointsDataset.py:243); of a
    ``[J, 3]`` array column 0 is read (the three columns repeat one flag, and the
    reference's painter cannot read a row of three).  ``joints_3d_vis=None``:
    every joint visible.  Padded rows are zero and never read; the all-zero
    people meta['joints_3d'] is padded with may be passed too (their flags are
    0, so they paint nothing, as in the reference)."""
    import numpy as np

    people = [np.asarray(p, dtype=np.float64) for p in joints_3d]
    if not people and not (isinstance(joints_3d, np.ndarray) and joints_3d.ndim == 3):
        raise _lib.FvpError("fvp: pack_poses3d: no person (the joint count is unknown)")
    J = people[0].shape[0] if people else joints_3d.shape[1]
    for p in people:
        if p.ndim != 2 or p.shape[1] < 3 or p.shape[0] != J:
            raise _lib.FvpError(f"fvp: pack_poses3d: each person is [J, >= 3] with one J, got {p.shape}")
    P = max(len(people), 1) if max_people is None else int(max_people)
    if len(people) > P:
        raise _lib.FvpError(f"fvp: pack_poses3d: {len(people)} people, max_people = {P}")
    joints = np.zeros((P, J, 3), dtype=np.float64)
    vis = np.zeros((P, J), dtype=np.uint8)
    for n, p in enumerate(people):
        joints[n] = p[:, :3]
    if joints_3d_vis is None:
        vis[:len(people)] = 1
    else:
        flags = [np.asarray(f) for f in joints_3d_vis]
        if len(flags) != len(people):
            raise _lib.FvpError(f"fvp: pack_poses3d: {len(people)} people but {len(flags)} visibility arrays")
        for n, f in enumerate(flags):
            if f.shape not in ((J,), (J, 3)):
                raise _lib.FvpError(f"fvp: pack_poses3d: visibility is [J] or [J, 3] with J = {J}, got {f.shape}")
            vis[n] = (f if f.ndim == 1 else f[:, 0]) > 0
    return torch.from_numpy(joints), torch.from_numpy(vis), torch.tensor(len(people), dtype=torch.int32)


def _pose_call(name, joints3d, vis3d, count, cams, resize_transform, cam_index, ori_image_size, image_size):
    """The validation render_poses3d and project_poses share; returns the operands as the ops take them."""
    from . import ops

    if not isinstance(joints3d, torch.Tensor) or joints3d.dim() != 4 or joints3d.shape[3] != 3 \
            or joints3d.dtype != torch.float64:
        raise _lib.FvpError(f"fvp: {name} takes joints3d fp64 [B,P,J,3], got "
                            f"{tuple(getattr(joints3d, 'shape', ()))} {getattr(joints3d, 'dtype', type(joints3d))}")
    B, P, J, _ = joints3d.shape
    if J > 32 or P > 32 or J < 1 or P < 1:
        raise _lib.FvpError(f"fvp: {name}: {P} people x {J} joints (1..32 each)")
    if not isinstance(count, torch.Tensor) or tuple(count.shape) != (B,) or count.dtype != torch.int32:
        raise _lib.FvpError(f"fvp: {name} takes count int32 [B] = {(B,)}, got "
                            f"{tuple(getattr(count, 'shape', ()))} {getattr(count, 'dtype', type(count))}")
    if vis3d is not None:
        if not isinstance(vis3d, torch.Tensor) or tuple(vis3d.shape) != (B, P, J) \
                or vis3d.dtype not in (torch.uint8, torch.bool):
            raise _lib.FvpError(f"fvp: {name} takes vis3d uint8 / bool [B,P,J] = {(B, P, J)}, got "
                                f"{tuple(getattr(vis3d, 'shape', ()))} {getattr(vis3d, 'dtype', type(vis3d))}")
        if vis3d.dtype == torch.bool:
            vis3d = vis3d.view(torch.uint8)
    if not isinstance(cams, torch.Tensor) or cams.dim() not in (2, 3) or cams.shape[-1] != ops.CAM_STRIDE \
            or cams.dtype != torch.float64 or cams.numel() == 0:
        raise _lib.FvpError(f"fvp: {name} takes cams fp64 [V,{ops.CAM_STRIDE}] or [S,V,{ops.CAM_STRIDE}] "
                            f"(geometry.pack_cameras64), got {tuple(getattr(cams, 'shape', ()))} "
                            f"{getattr(cams, 'dtype', type(cams))}")
    if cams.dim() == 2:
        cams = cams.unsqueeze(0)
    if not isinstance(resize_transform, torch.Tensor) or tuple(resize_transform.shape) != (2, 3) \
            or resize_transform.dtype != torch.float64:
        raise _lib.FvpError(f"fvp: {name} takes resize_transform fp64 [2,3], got "
                            f"{tuple(getattr(resize_transform, 'shape', ()))} "
                            f"{getattr(resize_transform, 'dtype', type(resize_transform))}")
    if cam_index is not None:
        if not isinstance(cam_index, torch.Tensor):
            cam_index = torch.as_tensor(cam_index, dtype=torch.int32)
        if tuple(cam_index.shape) != (B,) or cam_index.dtype != torch.int32:
            raise _lib.FvpError(f"fvp: {name} takes cam_index int32 [B] = {(B,)}, got {tuple(cam_index.shape)} "
                                f"{cam_index.dtype}")
        if cam_index.device.type == "cpu":  # a host index is checked here; a device one is a precondition
            if B and (int(cam_index.min()) < 0 or int(cam_index.max()) >= cams.shape[0]):
                raise _lib.FvpError(f"fvp: {name}: cam_index must lie in 0..{cams.shape[0] - 1}, got "
                                    f"{cam_index.tolist()}")
            cam_index = cam_index.to(joints3d.device)
    for what, t in (("joints3d", joints3d), ("vis3d", vis3d), ("count", count), ("cams", cams),
                    ("resize_transform", resize_transform), ("cam_index", cam_index)):
        if t is None:
            continue
        if t.device.type != "cuda" or t.device != joints3d.device:
            raise _lib.FvpError(f"fvp: {name}: {what} must be on a HIP device (one for all operands), got {t.device}")
        if not t.is_contiguous():
            raise _lib.FvpError(f"fvp: {name}: {what} must be contiguous")
    (ori_w, ori_h), (img_w, img_h) = ori_image_size, image_size
    if not (ori_w > 0 and ori_h > 0 and img_w > 0 and img_h > 0):
        raise _lib.FvpError(f"fvp: {name}: original image {ori_image_size}, image {image_size}")
    ops.forward_only(joints3d, cams, resize_transform)
    return joints3d, vis3d, count, cams, cam_index, resize_transform, float(ori_w), float(ori_h), float(img_w), \
        float(img_h)


def project_poses(joints3d: torch.Tensor, vis3d: torch.Tensor | None, count: torch.Tensor, cams: torch.Tensor,
                  resize_transform: torch.Tensor, *, ori_image_size, image_size, cam_index=None):
    """The 2-D ground truth of the ``'gt'`` heatmap source on the device, in one
    launch (fvp_project_poses): ``project_pose_cpu`` (lib/utils/cameras.py:58-84),
    the original-image test, ``affine_transform`` (lib/utils/transforms.py:53-56)
    and the resized-image test of JointsDataset.py:231-254, for every view of
    every frame.  Operands as :func:`render_poses3d`.  Returns ``(joints2d, vis2d)``:
    [B, V, P, J, 2] fp64 image pixels after the resize transform and [B, V, P, J]
    uint8, bit for bit the reference's float64 values; rows at or beyond
    ``count`` are zero.  ``render_keypoints(joints2d, count[:, None].expand(B,
    V).contiguous(), vis2d, ...)`` then equals ``render_poses3d``."""
    from . import ops

    return ops.project_poses(*_pose_call("project_poses", joints3d, vis3d, count, cams, resize_transform, cam_index,
                                         ori_image_size, image_size))


def render_poses3d(joints3d: torch.Tensor, vis3d: torch.Tensor | None, count: torch.Tensor, cams: torch.Tensor,
                   resize_transform: torch.Tensor, *, ori_image_size, image_size, heatmap_size, sigma: float,
                   dtype: torch.dtype | None = None, cam_index=None, return_keypoints: bool = False,
                   augment=None):
    """Input heatmaps painted from 3-D ground-truth poses on the device,
    channels-last, in one launch (fvp_render_poses3d): the ``'gt'`` branch of
    JointsDataset.__getitem__ (lib/dataset/JointsDataset.py:221-259) --
    ``TRAIN_HEATMAP_SRC: 'gt'`` of configs/shelf/jln64.yaml and
    configs/campus/jln64.yaml, and the upper-bound ablation at test time -- with
    ``data_augmentation = False``, or ``True`` when ``augment`` is given.  The
    launch projects every person into every view in float64 in the reference's
    operation order, applies its two visibility tests and paints as
    :func:`render_keypoints` does, so the result is bit for bit
    ``render_keypoints(*project_poses(...))``.

    joints3d  [B, P, J, 3] fp64 on a HIP device: meta['joints_3d'] (mm), see pack_poses3d
    vis3d     [B, P, J] uint8 or bool, or None (all visible): meta['joints_3d_vis'] > 0
    count     [B] int32: people of each frame (rows at or beyond it are never read)
    cams      [V, 24] or [S, V, 24] fp64: geometry.pack_cameras64 of one or S sequences
    resize_transform  [2, 3] fp64: the dataset's resize_transform (geometry.resize_transform)
    ori_image_size, image_size, heatmap_size  (W, H);  sigma: NETWORK.SIGMA
    dtype     None / torch.float32, or torch.float16 (fvp_render_poses3d_f16: bit for bit
              the fp32 result's ``.half()``)
    cam_index [B] int32, optional: the camera set of each frame, so that one batch can mix
              sequences.  A host tensor or list is range-checked and uploaded; a device
              tensor must hold values in 0..S-1.
    return_keypoints  also return (joints2d, vis2d) as project_poses does, written by
              the same launch
    augment   None, or the :class:`Augmentation` records as :func:`render_keypoints` takes
              them, [B, V, P, J] and [B, V, P, J, 4] (fvp_render_poses3d_aug).  Draw them with
              :func:`draw_augmentation` from the frame's 2-D keypoints and flags --
              ``project_poses(...)`` copied to the host, or the dataset's own -- and the
              result is bit for bit ``render_keypoints(*project_poses(...), augment=augment)``

    Every joint of a person enters the human scale, visible or not; only visible
    joints are painted.  A person with a non-finite 2-D coordinate is skipped, a
    point behind a camera is not special-cased (as in the reference), and a frame
    without people is a frame of zeros (the reference raises)."""
    from . import ops

    if dtype not in (None, torch.float32, torch.float16):
        raise _lib.FvpError(f"fvp: render_poses3d: dtype must be None, torch.float32 or torch.float16, got {dtype}")
    args = _pose_call("render_poses3d", joints3d, vis3d, count, cams, resize_transform, cam_index, ori_image_size,
                      image_size)
    W, H = heatmap_size
    if int(W) != W or int(H) != H or W < 1 or H < 1 or not sigma > 0:
        raise _lib.FvpError(f"fvp: render_poses3d: heatmap {heatmap_size}, sigma {sigma}")
    if augment is not None:
        B, P, J, _ = joints3d.shape
        scale, rect = _augment_records("render_poses3d", augment, (B, args[3].shape[1], P, J), joints3d.device)
        t, joints2d, vis2d = ops.render_poses3d_aug(*args[:6], scale, rect, *args[6:], int(H), int(W), float(sigma),
                                                    bool(return_keypoints), dtype == torch.float16)
    else:
        op = ops.render_poses3d_f16 if dtype == torch.float16 else ops.render_poses3d
        t, joints2d, vis2d = op(*args, int(H), int(W), float(sigma), bool(return_keypoints))
    cl = ChannelsLastHeatmaps(t, joints3d.shape[2])
    return (cl, joints2d, vis2d) if return_keypoints else cl
