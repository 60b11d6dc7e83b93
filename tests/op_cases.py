"""One case table for every registered ``torch.ops.fvp.*`` op (fvp/ops.py).

A case names an op, its arguments and the outputs the IMPLEMENTATION produces.
Nothing here touches a device: a tensor argument is a ``T(shape, dtype, fill)``
spec, scalars and lists stand for themselves, and an output is ``(shape,
dtype)`` written from the implementation's own ``torch.empty`` statements and
docstrings -- never by calling the fake kernel, which is what the table is
there to check.  ``fake_args`` materialises a case as fake tensors on "cuda"
under a FakeTensorMode (no GPU needed), ``real_args`` as real tensors on a
device, filled from a seed with valid values: heatmaps in [0, 1), indices in
range, counts in 1..P, cameras that see the whole space.

Shapes are the smallest with every dimension larger than 1 and, where the
layout allows it, distinct within a tensor, so a fake that takes a size from
the wrong dimension is seen; no input tensor is above 64 KiB.

Cases per op: the fp32 baseline; every tensor argument the implementation
converts (``_dev_f32``, ``.to(dtype=...)``) once as fp64 and once as fp16, and
every integer argument it converts in the other integer width; fp16 heatmaps
on every half route; every optional tensor None and given; every
output-shaping flag both ways; the empty calls that return before any launch.

Left out, because the implementation itself rejects them with FvpError (or
ValueError):
  * fp64 channels-last heatmaps (``_cl_input``: fp32 / fp16 only) for
    voxelize_cl, voxelize_cl_cams, voxel_columns (cl_joints > 0) and
    person_planes_cl;
  * the painters' and project_poses' operands in any other dtype than the one
    documented: joints3d / cams / resize_t fp64, count / cam_index int32,
    vis uint8, aug_scale fp32, aug_rect int16 (``_pose_operands``,
    ``_aug_operands``, ``render_keypoints_into``); render_keypoints* takes
    fp32 and fp64 joints, and both are cases;
  * voxel_columns without packed_grids and without cams / resize_t;
  * nms_topk with K = 0 (fvp_nms_topk: FVP_ERR_SHAPE; only B = 0 returns early);
  * frames_to_views on an empty frame tensor (``frame_spec``), and frames that
    are not uint8;
  * max_planes on person volumes that are not cubic.
No opcheck utility is switched off for any op (``Case.opcheck_off`` is empty
everywhere): every op has at least one floating-point output.
"""
from __future__ import annotations

import collections

import numpy as np
import torch

f16, f32, f64 = torch.float16, torch.float32, torch.float64
i16, i32, i64, u8 = torch.int16, torch.int32, torch.int64, torch.uint8


class T(collections.namedtuple("T", "shape dtype fill")):
    """A tensor argument: shape, dtype and how real_args fills it (see _fill)."""

    def as_(self, dtype):
        return self._replace(dtype=dtype)

    def with_shape(self, *shape):
        return self._replace(shape=tuple(shape))


# op: name in torch.ops.fvp / fvp.ops; args: ordered {name: T | scalar | list | None};
# outs: ((shape, dtype), ...) of the implementation; opcheck_off: {utility: reason};
# launches: False for the calls that return before any launch (all outputs empty).
Case = collections.namedtuple("Case", "id op args outs opcheck_off launches")

CASES: list = []


def _case(op, tag, args, outs, opcheck_off=None):
    outs = tuple((tuple(s), d) for s, d in outs)
    launches = any(int(np.prod(s)) > 0 for s, _ in outs)
    CASES.append(Case(f"{op}-{tag}", op, args, outs, dict(opcheck_off or {}), launches))


# ---------------------------------------------------------------------------
# shared sizes and geometry
B, V, J, H, W = 2, 3, 5, 8, 12
GV = V + (V & 1)  # FVP_GRID_SLOTS(3) = 4 != V
CP = 16  # channels per pixel of channels-last heatmaps (render_cp(5); cp % 8 == 0 for fp16)
X, Y, Z = 3, 4, 2
N = X * Y * Z
S = 2  # sequences (packed grids / camera sets)
K = 3
CAM = 24  # FVP_CAM_STRIDE

SPACE = dict(start=[-1000.0, -1000.0, -1000.0], end=[1000.0, 1000.0, 1000.0], center=[0.0, 0.0, 0.0])
ORI_W, ORI_H = 96.0, 64.0  # original image = network image; the heatmaps are 12 x 8 (stride 8)
IMG = dict(ori_max=96.0, img_w=96.0, img_h=64.0)

HM = T((B, V, J, H, W), f32, "unit")
HMCL = T((B, V, H, W, CP), f32, "unit")
PG3 = T((N, GV, 2), f32, ("packed", V))
PG4 = T((S, N, GV, 2), f32, ("packed", V))
CAMS2 = T((V, CAM), f32, "cams")
CAMS3 = T((S, V, CAM), f32, "cams")
RT = T((2, 3), f32, "resize")
GI = T((B,), i32, ("index", S))  # the implementation converts grid_index to int32


def _with(base: dict, **over) -> dict:
    assert not set(over) - set(base), set(over) - set(base)
    out = dict(base)
    out.update(over)
    return out


def _variants(base: dict, names, dtypes=(f64, f16)):
    """(tag, args) with each named tensor argument given once in each other dtype."""
    tags = {f64: "f64", f16: "f16", i32: "i32", i64: "i64", f32: "f32"}
    for n in names:
        for d in dtypes:
            yield f"{n}-{tags[d]}", _with(base, **{n: base[n].as_(d)})


# ---------------------------------------------------------------------------
# project_grid, pack_grid
_pg = dict(cams=CAMS2, resize_t=RT, **SPACE, bins=[X, Y, Z], **IMG, hm_w=W, hm_h=H)
_case("project_grid", "f32", _pg, [((V, N, 2), f32)])
for tag, a in _variants(_pg, ("cams", "resize_t")):
    _case("project_grid", tag, a, [((V, N, 2), f32)])

_sg = T((V, N, 2), f32, "coords")
for tag, d in (("f32", f32), ("f64", f64), ("f16", f16)):
    _case("pack_grid", tag, dict(sample_grid=_sg.as_(d)), [((N, GV, 2), f32)])


# ---------------------------------------------------------------------------
# the four whole-space voxelize ops: (cube [B,J,X,Y,Z] | (0,), xy [B,J,X,Y] | (0,)), fp32
def _vox_outs(a, joints=J):
    b = (a.get("heatmaps") or a.get("heatmaps_cl")).shape[0]
    x = X
    if "x_end" in a:
        x = (X if a["x_end"] < 0 else a["x_end"]) - a["x_begin"]
    return [((b, joints, x, Y, Z) if a["want_cube"] else (0,), f32),
            ((b, joints, x, Y) if a["want_xy"] else (0,), f32)]


def _vox_cases(op, base, hm, convert, hm_dtypes):
    """The cases the four voxelize ops share: hm is the heatmap argument's name."""
    cases = [("f32", base)]
    cases += [(f"{hm}-{t}", _with(base, **{hm: base[hm].as_(d)})) for t, d in hm_dtypes]
    cases += list(_variants(base, convert))
    seqs = dict(packed_grids=PG4) if "packed_grids" in base else dict(cams=CAMS3)
    cases += [("seqs-grid_index", _with(base, grid_index=GI, **seqs)),
              ("seqs-grid_index-i64", _with(base, grid_index=GI.as_(i64), **seqs)),
              ("cube-only", _with(base, want_xy=False)), ("xy-only", _with(base, want_cube=False)),
              ("B0", _with(base, **{hm: base[hm].with_shape(0, *base[hm].shape[1:])}))]
    if "x_begin" in base:
        cases += [("slab", _with(base, x_begin=1, x_end=3)), ("slab-to-end", _with(base, x_begin=2, x_end=-1)),
                  ("slab-f16", _with(base, x_begin=1, x_end=3, **{hm: base[hm].as_(f16)}))]
    for tag, a in cases:
        _case(op, tag, a, _vox_outs(a))


_vox_cases("voxelize", dict(heatmaps=HM, packed_grids=PG3, grid_index=None, X=X, Y=Y, Z=Z, want_cube=True,
                            want_xy=True),
           "heatmaps", ("packed_grids",), (("f64", f64), ("f16-half-route", f16)))
_cams_tail = dict(resize_t=RT, **SPACE, bins=[X, Y, Z], **IMG, want_cube=True, want_xy=True, x_begin=0, x_end=-1)
_vox_cases("voxelize_cams", dict(heatmaps=HM, cams=CAMS2, grid_index=None, **_cams_tail),
           "heatmaps", ("cams", "resize_t"), (("f64", f64), ("f16-half-route", f16)))
_vox_cases("voxelize_cl", dict(heatmaps_cl=HMCL, J=J, packed_grids=PG3, grid_index=None, X=X, Y=Y, Z=Z,
                               want_cube=True, want_xy=True),
           "heatmaps_cl", ("packed_grids",), (("f16-half-route", f16),))
_vox_cases("voxelize_cl_cams", dict(heatmaps_cl=HMCL, J=J, cams=CAMS2, grid_index=None, **_cams_tail),
           "heatmaps_cl", ("cams", "resize_t"), (("f16-half-route", f16),))


# ---------------------------------------------------------------------------
# nms_topk: a 5 x 7 map, K = 3 -> (vals [B,K] fp32, xy [B,K,2] int64, flat [B,K] int64)
MX, MY = 5, 7
_prob = T((B, 1, MX, MY), f32, "unit")


def _nms_outs(b, k):
    return [((b, k), f32), ((b, k, 2), i64), ((b, k), i64)]


for tag, p in (("f32", _prob), ("f64", _prob.as_(f64)), ("f16", _prob.as_(f16)), ("B0", _prob.with_shape(0, 1, MX, MY))):
    _case("nms_topk", tag, dict(prob=p, K=K), _nms_outs(p.shape[0], K))

# nms_topk_columns: the same map over a cube [B,J,X,Y,Z] = [2,3,5,7,4] -> + columns [B,K,J,Z] fp32
CJ, CZ = 3, 4
_ncube = T((B, CJ, MX, MY, CZ), f32, "unit")
_ntc = dict(prob=_prob, K=2, cube=_ncube)
for tag, a in ([("f32", _ntc)] + list(_variants(_ntc, ("prob", "cube")))
               + [("B0", _with(_ntc, prob=_prob.with_shape(0, 1, MX, MY), cube=_ncube.with_shape(0, CJ, MX, MY, CZ))),
                  ("K0", _with(_ntc, K=0))]):
    b, k = a["prob"].shape[0], a["K"]
    _case("nms_topk_columns", tag, a, _nms_outs(b, k) + [((b, k, CJ, CZ), f32)])


# ---------------------------------------------------------------------------
# gather_columns: cube [2,5,3,4,6], flat [2,7] (< X*Y = 12) -> [B,K,J,Z] fp32
GK, GZ = 7, 6
_gcube = T((B, J, X, Y, GZ), f32, "unit")
_gflat = T((B, GK), i64, ("index", X * Y))  # the implementation converts flat to int64
_gc = dict(cube=_gcube, flat=_gflat)
for tag, a in ([("f32", _gc)] + list(_variants(_gc, ("cube",))) + list(_variants(_gc, ("flat",), (i32,)))
               + [("K0", _with(_gc, flat=_gflat.with_shape(B, 0)))]):
    _case("gather_columns", tag, a, [((B, a["flat"].shape[1], J, GZ), f32)])

# gather_bbox: size [B,2,X,Y] = [2,2,5,7], flat [2,3] -> [B,K,2] fp32
_bsize = T((B, 2, MX, MY), f32, "unit")
_bflat = T((B, K), i64, ("index", MX * MY))
_gb = dict(size=_bsize, flat=_bflat)
for tag, a in ([("f32", _gb)] + list(_variants(_gb, ("size",))) + list(_variants(_gb, ("flat",), (i32,)))
               + [("K0", _with(_gb, flat=_bflat.with_shape(B, 0)))]):
    _case("gather_bbox", tag, a, [((B, a["flat"].shape[1], 2), f32)])

# voxel_columns: planar [B,V,J,H,W] (cl_joints = 0) or channels-last [B,V,H,W,cp] (cl_joints = J),
# cached grid or cameras -> [B,K,J,Z] fp32
_vflat = T((B, K), i64, ("index", X * Y))
_vc_grid = dict(heatmaps=HM, cl_joints=0, packed_grids=PG3, cams=None, grid_index=None, resize_t=None, **SPACE,
                bins=[X, Y, Z], **IMG, flat=_vflat)
_vc_cams = _with(_vc_grid, packed_grids=None, cams=CAMS2, resize_t=RT)
_vc = ([("planar-grid", _vc_grid), ("planar-cams", _vc_cams),
        ("cl-grid", _with(_vc_grid, heatmaps=HMCL, cl_joints=J)), ("cl-cams", _with(_vc_cams, heatmaps=HMCL, cl_joints=J)),
        ("planar-f16-half-route", _with(_vc_grid, heatmaps=HM.as_(f16))),
        ("planar-cams-f16-half-route", _with(_vc_cams, heatmaps=HM.as_(f16))),
        ("cl-f16-half-route", _with(_vc_grid, heatmaps=HMCL.as_(f16), cl_joints=J)),
        ("cl-cams-f16-half-route", _with(_vc_cams, heatmaps=HMCL.as_(f16), cl_joints=J)),
        ("planar-f64", _with(_vc_grid, heatmaps=HM.as_(f64)))]
       + list(_variants(_vc_grid, ("packed_grids",))) + list(_variants(_vc_cams, ("cams", "resize_t")))
       + list(_variants(_vc_grid, ("flat",), (i32,)))
       + [("seqs-grid_index", _with(_vc_grid, packed_grids=PG4, grid_index=GI)),
          ("seqs-grid_index-i64", _with(_vc_grid, packed_grids=PG4, grid_index=GI.as_(i64))),
          ("cams-seqs-grid_index", _with(_vc_cams, cams=CAMS3, grid_index=GI)),
          ("K0", _with(_vc_grid, flat=_vflat.with_shape(B, 0)))])
for tag, a in _vc:
    _case("voxel_columns", tag, a, [((B, a["flat"].shape[1], J, Z), f32)])


# ---------------------------------------------------------------------------
# proposal_centers: index [B,K,2] + hm1d [B,K,Z], or index [B,K,3] alone -> centers [B,K,7] fp32
PZ = 4
_pc = dict(index=T((B, K, 2), i64, ("index", 5)), hm1d=T((B, K, PZ), f32, "unit"), confs=T((B, K), f32, "unit"),
           match_bbox=T((B, K, 2), f32, "unit"), scale=[100.0, 110.0, 120.0], bias=[-1000.0, -900.0, -800.0],
           min_score=0.3)
_pc3 = _with(_pc, index=T((B, K, 3), i64, ("index", 5)), hm1d=None)
for tag, a in ([("hm1d", _pc), ("index3", _pc3)] + list(_variants(_pc, ("hm1d", "confs", "match_bbox")))
               + list(_variants(_pc, ("index",), (i32,))) + list(_variants(_pc3, ("index",), (i32,)))
               + [("K0", _with(_pc, index=T((B, 0, 2), i64, ("index", 5)), hm1d=T((B, 0, PZ), f32, "unit"),
                               confs=T((B, 0), f32, "unit"), match_bbox=T((B, 0, 2), f32, "unit")))]):
    if tag == "index-i32" and a["hm1d"] is None:
        tag = "index3-i32"
    _case("proposal_centers", tag, a, [((B, a["confs"].shape[1], 7), f32)])


# ---------------------------------------------------------------------------
# the per-person ops: cubic person bins (4,4,4) over the fine grid (6,5,4) of a 2 m space with an
# individual space of (1200, 1500, 2000) mm, P = 3 (project_individual.py:43-85: fine =
# whole / ind * (bins - 1) + 1, scale = (fine - 1) / whole, bias = -ind / 2 / whole * (fine - 1)
# - scale * (centre - whole / 2))
P = 3
SB = 4
FINE = [6, 5, 4]
_spec = dict(fine=FINE, scale=[0.0025, 0.002, 0.0015], bias=[1.0, 0.5, 0.0], whole_size=[2000.0, 2000.0, 2000.0],
             ind_size=[1200.0, 1500.0, 2000.0], bins=[SB, SB, SB], want_cubes=True, want_planes=True)
_FG = T((FINE[0] * FINE[1] * FINE[2], GV, 2), f32, ("packed", V))
_PROPS = T((P, 7), f32, "proposals")
_FO = T((P,), i32, ("index", B))  # the implementation converts frame_of to int32


def _person_outs(a, joints=J):
    p = a["proposals"].shape[0]
    return [((p, joints, SB, SB, SB) if a["want_cubes"] else (0,), f32),
            ((3 * p, joints, SB, SB) if a["want_planes"] else (0,), f32), ((p, 3), f32)]


def _person_cases(op, base, hm, convert, hm_dtypes):
    cases = [("f32", base)]
    cases += [(f"{hm}-{t}", _with(base, **{hm: base[hm].as_(d)})) for t, d in hm_dtypes]
    cases += list(_variants(base, convert))
    cases += [("frame_of-none", _with(base, frame_of=None)), ("frame_of-i64", _with(base, frame_of=_FO.as_(i64))),
              ("cubes-only", _with(base, want_planes=False)), ("planes-only", _with(base, want_cubes=False)),
              ("P0", _with(base, proposals=_PROPS.with_shape(0, 7), frame_of=_FO.with_shape(0)))]
    for tag, a in cases:
        _case(op, tag, a, _person_outs(a))


_person_cases("person_planes", dict(heatmaps=HM, fine_grid=_FG, proposals=_PROPS, frame_of=_FO, **_spec),
              "heatmaps", ("fine_grid", "proposals"), (("f64", f64), ("f16", f16)))
_person_cases("person_planes_cl", dict(heatmaps_cl=HMCL, J=J, fine_grid=_FG, proposals=_PROPS, frame_of=_FO, **_spec),
              "heatmaps_cl", ("fine_grid", "proposals"), (("f16-half-route", f16),))
_person_cases("person_planes_cams", dict(heatmaps=HM, cams=CAMS2, resize_t=RT, **SPACE, **IMG, proposals=_PROPS,
                                         frame_of=_FO, **_spec),
              "heatmaps", ("cams", "resize_t", "proposals"), (("f64", f64), ("f16", f16)))

# max_planes: cubes [P,J,S,S,S] -> planes [3P,J,S,S] fp32
_mc = T((P, J, SB, SB, SB), f32, "unit")
for tag, c in (("f32", _mc), ("f64", _mc.as_(f64)), ("f16", _mc.as_(f16)), ("P0", _mc.with_shape(0, J, SB, SB, SB))):
    _case("max_planes", tag, dict(cubes=c), [((3 * c.shape[0], J, SB, SB), f32)])


# ---------------------------------------------------------------------------
# soft_argmax: planes 4 x 4, P = 2 -> (pose [3,P,J,2], maxprob [3,P,J]) fp32; fuse_poses -> ([P,J,3], [P])
JP = 2
_sa = dict(features=T((3, JP, J, SB, SB), f32, "signed"), center_grid=T((3, SB * SB, 2), f32, "signed"),
           offset=T((JP, 3), f32, "signed"), beta=100.0)
for tag, a in ([("f32", _sa), ("offset-none", _with(_sa, offset=None)),
                ("flat-planes", _with(_sa, features=T((3, JP, J, SB * SB, 1), f32, "signed")))]
               + list(_variants(_sa, ("features", "center_grid", "offset")))
               + [("P0", _with(_sa, features=T((3, 0, J, SB, SB), f32, "signed"), offset=T((0, 3), f32, "signed")))]):
    p = a["features"].shape[1]
    _case("soft_argmax", tag, a, [((3, p, J, 2), f32), ((3, p, J), f32)])

_fp = dict(pose=T((3, JP, J, 2), f32, "signed"), weights=T((3 * JP, J, 1), f32, "unit"),
           maxprob=T((3, JP, J), f32, "unit"))
for tag, a in ([("f32", _fp)] + list(_variants(_fp, ("pose", "weights", "maxprob")))
               + [("P0", dict(pose=T((3, 0, J, 2), f32, "signed"), weights=T((0, J, 1), f32, "unit"),
                              maxprob=T((3, 0, J), f32, "unit")))]):
    p = a["pose"].shape[1]
    _case("fuse_poses", tag, a, [((p, J, 3), f32), ((p,), f32)])


# ---------------------------------------------------------------------------
# the painters: maps 8 x 12 of a 64 x 96 image, P = 2 people, J = 5 -> channels-last [B,V,H,W,16]
RP = 2
_j2 = T((B, V, RP, J, 2), f64, ("pixels", ORI_W, ORI_H))
_rk = dict(joints=_j2, count=T((B, V), i32, ("count", RP)), vis=T((B, V, RP, J), u8, "vis"), image_w=ORI_W,
           image_h=ORI_H, H=H, W=W, sigma=1.0)


def _b0(a, *names):
    return _with(a, **{n: a[n].with_shape(0, *a[n].shape[1:]) for n in names if a[n] is not None})


for op, dt in (("render_keypoints", f32), ("render_keypoints_f16", f16)):
    for tag, a in (("f64-joints", _rk), ("f32-joints", _with(_rk, joints=_j2.as_(f32))), ("vis-none", _with(_rk, vis=None)),
                   ("B0", _b0(_rk, "joints", "count", "vis"))):
        _case(op, tag, a, [((a["joints"].shape[0], V, H, W, CP), dt)])

_aug = dict(aug_scale=T((B, V, RP, J), f32, "aug_scale"), aug_rect=T((B, V, RP, J, 4), i16, "aug_rect"))
_rka = dict(joints=_j2, count=_rk["count"], vis=_rk["vis"], **_aug, image_w=ORI_W, image_h=ORI_H, H=H, W=W, sigma=1.0,
            half=False)
for tag, a in (("f32-out", _rka), ("f16-out", _with(_rka, half=True)), ("f32-joints", _with(_rka, joints=_j2.as_(f32))),
               ("vis-none", _with(_rka, vis=None)), ("B0", _b0(_rka, "joints", "count", "vis", "aug_scale", "aug_rect"))):
    _case("render_keypoints_aug", tag, a, [((a["joints"].shape[0], V, H, W, CP), f16 if a["half"] else f32)])

# the 'gt' source: joints3d [B,P,J,3], cams [S,V,24], all fp64 -> joints2d [B,V,P,J,2] fp64, vis2d uint8
_pp = dict(joints3d=T((B, RP, J, 3), f64, "xyz"), vis3d=T((B, RP, J), u8, "vis"), count=T((B,), i32, ("count", RP)),
           cams=CAMS3.as_(f64), cam_index=T((B,), i32, ("index", S)), resize_t=RT.as_(f64), ori_w=ORI_W, ori_h=ORI_H,
           image_w=ORI_W, image_h=ORI_H)
_pp_b0 = _b0(_pp, "joints3d", "vis3d", "count", "cam_index")
for tag, a in (("f64", _pp), ("vis3d-none", _with(_pp, vis3d=None)), ("cam_index-none", _with(_pp, cam_index=None)),
               ("B0", _pp_b0)):
    b = a["joints3d"].shape[0]
    _case("project_poses", tag, a, [((b, V, RP, J, 2), f64), ((b, V, RP, J), u8)])


def _rp_outs(a, dt):
    b, kp = a["joints3d"].shape[0], a["keypoints"]
    return [((b, V, H, W, CP), dt), ((b, V, RP, J, 2) if kp else (0,), f64), ((b, V, RP, J) if kp else (0,), u8)]


_rp = dict(**_pp, H=H, W=W, sigma=1.0, keypoints=True)
_rp_set = (("keypoints", _rp), ("no-keypoints", _with(_rp, keypoints=False)), ("vis3d-none", _with(_rp, vis3d=None)),
           ("cam_index-none", _with(_rp, cam_index=None)), ("B0", _b0(_rp, "joints3d", "vis3d", "count", "cam_index")))
for op, dt in (("render_poses3d", f32), ("render_poses3d_f16", f16)):
    for tag, a in _rp_set:
        _case(op, tag, a, _rp_outs(a, dt))

_aug3 = dict(joints3d=_pp["joints3d"], vis3d=_pp["vis3d"], count=_pp["count"], cams=_pp["cams"],
             cam_index=_pp["cam_index"], resize_t=_pp["resize_t"], **_aug, ori_w=ORI_W, ori_h=ORI_H, image_w=ORI_W,
             image_h=ORI_H, H=H, W=W, sigma=1.0, keypoints=True, half=False)
for tag, a in (("f32-out-keypoints", _aug3), ("f16-out-keypoints", _with(_aug3, half=True)),
               ("f32-out-no-keypoints", _with(_aug3, keypoints=False)),
               ("f16-out-no-keypoints", _with(_aug3, keypoints=False, half=True)),
               ("vis3d-none", _with(_aug3, vis3d=None)), ("cam_index-none", _with(_aug3, cam_index=None)),
               ("B0", _b0(_aug3, "joints3d", "vis3d", "count", "cam_index", "aug_scale", "aug_rect"))):
    _case("render_poses3d_aug", tag, a, _rp_outs(a, f16 if a["half"] else f32))


# ---------------------------------------------------------------------------
# frames_to_views: uint8 frames per view [B,V,H,W,3|4] or a 2 x 2 mosaic [B,2H,2W,3] -> [B,V,3,H,W] fp32
FH, FW = 6, 10
_fv = dict(data=T((B, V, FH, FW, 3), u8, "bytes"), mosaic=[], swap_rb=False, mean=[0.485, 0.456, 0.406],
           std=[0.229, 0.224, 0.225])
_case("frames_to_views", "views-rgb", _fv, [((B, V, 3, FH, FW), f32)])
_case("frames_to_views", "views-bgrx-swap", _with(_fv, data=T((B, V, FH, FW, 4), u8, "bytes"), swap_rb=True),
      [((B, V, 3, FH, FW), f32)])
_case("frames_to_views", "mosaic", _with(_fv, data=T((B, 2 * FH, 2 * FW, 3), u8, "bytes"), mosaic=[2, 2]),
      [((B, 4, 3, FH, FW), f32)])

assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"
OPS_WITH_CASES = sorted({c.op for c in CASES})


# ---------------------------------------------------------------------------
# materialising a case
def registered_ops() -> list:
    """The names registered under torch.ops.fvp (importing fvp.ops registers them)."""
    from fvp import ops  # noqa: F401

    names = set()
    for qual in torch._C._dispatch_get_all_op_names():
        if qual.startswith("fvp::"):
            names.add(qual[len("fvp::"):].split(".")[0])
    return sorted(names)


def detection_chain(hm, packed, size):
    """voxelize -> nms_topk_columns -> gather_bbox -> proposal_centers through the fvp.ops names, with
    two dtype-sensitive torch ops on the cube: what the compile tests trace (hm [B,V,J,H,W] fp32 or
    fp16, packed [N,GV,2], size [B,2,X,Y])."""
    from fvp import ops

    cube, xy = ops.voxelize(hm, packed, None, X, Y, Z, True, True)
    total = cube.sum(dtype=None)  # a graph that believes the cube is fp16 sums, and returns, fp16
    low = cube.half()
    vals, idx, flat, cols = ops.nms_topk_columns(xy[:, 1:2], K, cube)
    bbox = ops.gather_bbox(size, flat)
    centers = ops.proposal_centers(idx, cols[:, :, 0], vals, bbox, [100.0, 110.0, 120.0], [-1000.0, -900.0, -800.0],
                                   0.3)
    return cube, xy, total, low, vals, idx, flat, cols, bbox, centers


def fake_args(case) -> list:
    """The case's arguments as fake tensors on "cuda"; call under a FakeTensorMode."""
    return [torch.empty(a.shape, dtype=a.dtype, device="cuda") if isinstance(a, T) else a
            for a in case.args.values()]


def _cams(shape, rng) -> np.ndarray:
    """Camera records [..., 24]: R = identity, the centre T about 4 m in front of the space (a
    different x per view), f = 150 px and the principal point in the middle of the 96 x 64 image,
    so the whole 2 m space projects into the image; small distortion."""
    rec = np.zeros(shape, np.float64)
    flat = rec.reshape(-1, CAM)
    for r in range(flat.shape[0]):
        flat[r, [0, 4, 8]] = 1.0
        flat[r, 9:12] = [(r % V - 1) * 200.0 + 20.0 * rng.rand(), 40.0 * rng.rand() - 20.0, -4000.0 - 200.0 * rng.rand()]
        flat[r, 12:14] = 150.0 + 10.0 * rng.rand(2)
        flat[r, 14:16] = [ORI_W / 2 + rng.rand(), ORI_H / 2 + rng.rand()]
        flat[r, 16:19] = 0.01 * rng.rand(3)
        flat[r, 19:21] = 0.001 * rng.rand(2)
    return rec


def _fill(t: T, seed: int, rng) -> np.ndarray:
    """float64 / integer numpy values of a tensor spec.  Float fills draw from `rng`; integer fills
    are patterns shifted by the seed, so two consecutive seeds differ in every element."""
    kind = t.fill if isinstance(t.fill, tuple) else (t.fill,)
    shape, n = t.shape, int(np.prod(t.shape))
    ar = np.arange(n).reshape(shape)
    if kind[0] == "unit":  # heatmaps, probabilities: [0, 1)
        return rng.rand(*shape)
    if kind[0] == "signed":
        return 2.0 * rng.rand(*shape) - 1.0
    if kind[0] == "coords":  # a sample grid: normalised coordinates, a little beyond the image
        return 2.1 * rng.rand(*shape) - 1.05
    if kind[0] == "packed":  # pack_grid's layout [..., GV, 2]: the padding slots hold (-2, -2)
        a = 2.1 * rng.rand(*shape) - 1.05
        a[..., kind[1]:, :] = -2.0
        return a
    if kind[0] == "cams":
        return _cams(shape, rng)
    if kind[0] == "resize":  # original image = network image: the identity, jittered
        return np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]) + 0.01 * rng.rand(2, 3)
    if kind[0] == "proposals":  # (x, y, z mm, gt, conf, bbox_w, bbox_h): centres well inside the space
        a = rng.rand(*shape)
        a[..., :3] = 600.0 * a[..., :3] - 300.0
        return a
    if kind[0] == "xyz":  # 3-D joints around the middle of the space: every view sees them
        return 600.0 * rng.rand(*shape) - 300.0
    if kind[0] == "pixels":  # 2-D joints inside the middle of the image
        return (0.2 + 0.6 * rng.rand(*shape)) * np.array([kind[1], kind[2]])
    if kind[0] == "aug_scale":
        return 0.6 + 0.8 * rng.rand(*shape)
    if kind[0] == "index":  # in [0, hi)
        return (ar * 5 + seed) % kind[1]
    if kind[0] == "count":  # in 1..P
        return 1 + (ar + seed) % kind[1]
    if kind[0] == "vis":  # 0 / 1, two of three visible
        return ((ar + seed) % 3 != 0).astype(np.int64)
    if kind[0] == "aug_rect":  # (r0, r1, c0, c1) of small rectangles, some empty
        return (ar * 3 + seed) % 4
    if kind[0] == "bytes":
        return rng.randint(0, 256, size=shape)
    raise KeyError(t.fill)


def real_args(case, device, seed: int) -> list:
    """The case's arguments as real tensors on `device`, filled from `seed` with valid values.
    Two seeds give the same shapes, dtypes and scalars, and different tensor values."""
    rng = np.random.RandomState(1000 + seed)
    out = []
    for a in case.args.values():
        if isinstance(a, T):
            a = torch.from_numpy(np.ascontiguousarray(_fill(a, seed, rng))).to(a.dtype).to(device)
        out.append(a)
    return out
