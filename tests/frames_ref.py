"""Reference for uint8 camera frames (include/fvp.h fvp_frame_spec), in numpy fp32.

The contract is ToTensor + Normalize on the CPU,
    v = ((float)b / 255.0f - mean[c]) / std[c]
three rounded fp32 operations with IEEE-correct divisions -- which numpy's
float32 arithmetic is.  A byte has 256 values, so the whole function is the
3 x 256 ``table``; ``views_ref`` applies it through the spec's byte addressing
and so is independent of both torch and the kernels."""
import numpy as np

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

_B = np.arange(256, dtype=np.float32)


def table(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """[3, 256] float32: row c, column b = ((float)b / 255.0f - mean[c]) / std[c]."""
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    t = ((_B[None, :] / np.float32(255.0)) - mean[:, None]) / std[:, None]
    assert t.dtype == np.float32
    return t


def table_reciprocal(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """A planted fault: b * (1/255) in place of b / 255."""
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    return ((_B[None, :] * (np.float32(1.0) / np.float32(255.0))) - mean[:, None]) / std[:, None]


def table_folded(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """A planted fault: the folded affine b * k + m, k = 1 / (255 std), m = -mean / std."""
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    k = np.float32(1.0) / (np.float32(255.0) * std)
    m = -mean / std
    return _B[None, :] * k[:, None] + m[:, None]


def spec_fields(spec):
    """The integer fields of a spec (ctypes FrameSpec or anything with its attributes) as a dict."""
    return {k: int(getattr(spec, k)) for k in ("H", "W", "VR", "VC", "frame_stride", "vr_stride", "vc_stride",
                                               "row_stride", "pix_stride", "swap_rb")}


def views_ref(buf, B, spec):
    """buf: 1-D uint8 array whose element 0 is the byte the frames pointer addresses;
    -> [B, VR*VC, 3, H, W] float32 by table lookup through the spec's strides."""
    buf = np.asarray(buf)
    assert buf.dtype == np.uint8 and buf.ndim == 1
    f = spec_fields(spec)
    tab = table(tuple(spec.mean), tuple(spec.std))
    b = np.arange(B, dtype=np.int64)[:, None, None, None, None, None]
    r = np.arange(f["VR"], dtype=np.int64)[None, :, None, None, None, None]
    cc = np.arange(f["VC"], dtype=np.int64)[None, None, :, None, None, None]
    c = np.arange(3, dtype=np.int64)[None, None, None, :, None, None]
    y = np.arange(f["H"], dtype=np.int64)[None, None, None, None, :, None]
    x = np.arange(f["W"], dtype=np.int64)[None, None, None, None, None, :]
    k = 2 - c if f["swap_rb"] else c
    idx = (b * f["frame_stride"] + r * f["vr_stride"] + cc * f["vc_stride"] + y * f["row_stride"]
           + x * f["pix_stride"] + k)
    out = tab[np.broadcast_to(c, idx.shape), buf[idx]]
    return out.reshape(B, f["VR"] * f["VC"], 3, f["H"], f["W"])


def buffer_of(t):
    """The bytes a strided uint8 torch tensor can address, from its first element, as a 1-D
    numpy array (for views_ref)."""
    import torch

    n = 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
    return torch.as_strided(t, (n,), (1,)).cpu().numpy()


def bits(a):
    """float32 array / tensor -> its int32 bit patterns (numpy), for bit-for-bit comparisons."""
    import torch

    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
