// 2-D keypoints -> channels-last input heatmaps, one launch.
//
// Replaces JointsDataset.generate_input_heatmap (lib/dataset/JointsDataset.py:
// 368-447, with compute_human_scale :265-279) with data_augmentation = False:
// the 'pred' heatmaps of Shelf and Campus, painted per (view, person, joint) in
// numpy on the host.  The output is the [B][V][H][W][Cp] layout the gathers
// read in place (fvp_voxelize_cl, fvp_person_planes_cl).
//
// Shape of the kernel.  One block owns a band of kBandH rows of one
// frame-view.  Its prologue rebuilds that view's count * J window records in
// LDS -- in fp64 and in the reference's operation order, so that every int()
// truncation lands where numpy's does -- and lists those whose clipped window
// meets the band.  The block then walks the band in tiles of kTileW pixels:
// per tile it keeps, per group of 4 channels, the listed records that meet the
// tile, and a lane that owns 4 channels of a pixel walks the kept records of
// its group, takes the max in registers and stores one float4 -- a wave's
// store instruction writes 1 KiB of consecutive bytes, a block its band's
// kBandH * W * Cp * 4 consecutive bytes.  Every element is written exactly
// once (padding channels and uncovered pixels as 0.0f): no memset, no atomics
// on global memory, and max is order-free, so the output is deterministic.
//
// fp16 output (fvp_render_keypoints_f16, the layout fvp_voxelize_cl_f16 reads):
// the same kernel with JPL = 8 joints per lane instead of 4.  A lane owns 8
// channels of a pixel, a channel group is 8 channels with up to 8 P kept
// records, and the lane converts each channel's fp32 maximum once, to nearest
// even, and stores one 16-B piece -- still 1 KiB per wave store.  Rounding is
// monotone, so max-then-round equals the fp32 render followed by Tensor.half()
// bit for bit.
//
// The per-pixel value is fp32: expf(-(dx^2 + dy^2) * (float)(1 / (2 sigma^2)))
// with the integer offsets from the window's centre pixel ul + floor(size / 2)
// (which is often mu - 1, not mu: the reference's Gaussian sits on its patch).
//
// 'gt' heatmaps (fvp_render_poses3d, fvp_render_poses3d_f16): the same kernel
// with POSE = true.  Its first loop, instead of reading 2-D keypoints, projects
// the frame's 3-D joints through the view's fp64 camera and the resize
// transform and applies the two visibility tests of JointsDataset.__getitem__
// (lib/dataset/JointsDataset.py:221-259 with lib/utils/cameras.py:58-84 and
// lib/utils/transforms.py:53-56) -- project_pose_point below, in the order
// numpy evaluates them -- and keeps the visibility byte in LDS.  Everything after
// that loop is the one body, so the result equals fvp_project_poses followed by
// fvp_render_keypoints bit for bit.
//
// Augmented heatmaps (fvp_render_keypoints_aug, fvp_render_poses3d_aug): the same
// kernel with AUG = true paints generate_input_heatmap with data_augmentation =
// True (JointsDataset.py:413-432).  The random draws are the caller's: one record
// per (frame, view, person, joint) holds the factor the patch is multiplied by and
// the rectangle of the patch that is zeroed.  The thread that builds a joint's
// window keeps the record in the 16 bytes of q[] it has just read for the last
// time, so an AUG block takes the LDS of a plain one; the pixel loop multiplies
// g by the factor outside the rectangle, contributes nothing inside it, and the
// maximum is clamped at 1 before the store (a factor can exceed 1).
#include <math.h>

#include <type_traits>

#include "fvp_device.h"

namespace fvp {

constexpr int kTileW = 32, kBandH = 4, kRenderThreads = 256;
constexpr int kMaxRenderJ = 32, kMaxRenderP = 32;

// Clipped window [x0, x1) x [y0, y1) in the heatmap (empty: x0 >= x1), the
// pixel the Gaussian is centred on, 1 / (2 sigma^2) and the joint.
struct RenderRec {
    int x0, x1, y0, y1;
    int cx, cy;
    float inv;
    int j;
};

struct RenderPerson {
    double tmp;  // 3 * cur_sigma
    int n;       // ceil(2 tmp + 1): the patch is n x n
    int c0;      // floor((2 tmp + 1) / 2): the patch's centre
    float inv;
    int ok;  // every coordinate finite
};

struct RenderArgs {
    const void *joints;
    const int *count;
    const unsigned char *vis;
    void *out;  // fp32 (JPL 4) or fp16 (JPL 8)
    double stride_x, stride_y, sigma;
    int joints_f64, P, J, H, W, tiles_x, bands;
};

// The 'gt' operands: 3-D joints and flags shared by a frame's views, fp64 camera records in the
// field order of the fp32 one (FVP_CAM_STRIDE), the 2x3 resize transform.
struct PoseArgs {
    const double *joints3d;      // [B][P][J][3]
    const unsigned char *vis3d;  // [B][P][J] or null
    const int *count;            // [B]
    const double *cams;          // [S][V][FVP_CAM_STRIDE]
    const int *cam_index;        // [B] or null
    const double *resize_t;      // [2][3]
    double *joints2d;            // [B][V][P][J][2] or null
    unsigned char *vis2d;        // [B][V][P][J] or null
    double ori_w1, ori_h1;       // ori_image_size - 1
    double image_w, image_h;
    int S, V;
};

struct RenderPoseArgs : RenderArgs {
    PoseArgs pose;
};

// The augmentation records, one per (frame, view, person, joint) as vis is laid out.
struct AugArgs {
    const float *scale;  // [B][V][P][J]
    const short *rect;   // [B][V][P][J][4]: rows r0, r1, columns c0, c1 of the patch
};

template <class Base>
struct WithAug : Base {
    AugArgs aug;
};

// A listed joint's augmentation in LDS: the factor, and the zeroed rectangle [r0, r1) x [c0, c1) in
// patch coordinates (negative values pinned to 0) with the patch's centre pc, so that the pixel at
// (dx, dy) from the Gaussian's centre is the patch's (dx + pc, dy + pc).
struct AugRec {
    float scale;
    int pc;
    short r0, r1, c0, c1;
};
static_assert(sizeof(AugRec) == sizeof(double2), "an AugRec takes the place of its joint's q");

// One joint through one camera: project_point_cpu (cameras.py:58-84), the original-image test
// (JointsDataset.py:238-244), affine_transform (transforms.py:53-56) and the resized-image test
// (JointsDataset.py:249-251).  fp64, one rounded operation per operator, fma() only where numpy's
// matmul (3x3 by 3xJ) and dot (2x3 by [x, y, 1]) use one; NaN compares false as in numpy.  A
// point behind the camera is not special-cased (the reference does not either).
__device__ __forceinline__ bool project_pose_point(const double *X, bool vis3d, const double *cam, const PoseArgs &a,
                                                   double &qx, double &qy) {
    const double *t = a.resize_t;
    const double d0 = X[0] - cam[9], d1 = X[1] - cam[10], d2 = X[2] - cam[11];
    const double xc0 = fma(cam[2], d2, fma(cam[1], d1, cam[0] * d0));
    const double xc1 = fma(cam[5], d2, fma(cam[4], d1, cam[3] * d0));
    const double xc2 = fma(cam[8], d2, fma(cam[7], d1, cam[6] * d0));
    const double den = xc2 + 1e-5;
    const double y0 = xc0 / den, y1 = xc1 / den;
    const double r = y0 * y0 + y1 * y1;
    const double k0 = cam[16], k1 = cam[17], k2 = cam[18], p0 = cam[19], p1 = cam[20];
    const double dd = ((1.0 + k0 * r) + (k1 * r) * r) + ((k2 * r) * r) * r;
    const double u = (y0 * dd + ((2.0 * p0) * y0) * y1) + p1 * (r + (2.0 * y0) * y0);
    const double w = (y1 * dd + ((2.0 * p1) * y0) * y1) + p0 * (r + (2.0 * y1) * y1);
    const double px = cam[12] * u + cam[14], py = cam[13] * w + cam[15];
    bool vis = vis3d && px >= 0.0 && px <= a.ori_w1 && py >= 0.0 && py <= a.ori_h1;
    qx = fma(t[0], px, t[1] * py) + t[2];
    qy = fma(t[3], px, t[4] * py) + t[5];
    // np.min(pose[i]) < 0: a NaN coordinate makes the minimum NaN, which compares false
    const bool neg = qx == qx && qy == qy && (qx < 0.0 || qy < 0.0);
    if (neg || qx >= a.image_w || qy >= a.image_h) vis = false;
    return vis;
}

// The camera record of frame b, view v: cam_index picks the frame's set (pinned into 0..S-1).
__device__ __forceinline__ const double *pose_camera(const PoseArgs &a, int b, int v) {
    const int set = a.cam_index ? min(max(a.cam_index[b], 0), a.S - 1) : 0;
    return a.cams + ((long long)set * a.V + v) * FVP_CAM_STRIDE;
}

// Python's int(): truncation toward zero.  Values beyond +-2^30 pixels are
// pinned there (a C conversion of them is undefined); such a window lies off
// every heatmap either way.
__device__ __forceinline__ int trunc_int(double v) {
    return (int)fmin(fmax(v, -1073741824.0), 1073741824.0);
}

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// A lane's running maxima: channels 0..3 of its group, and 4..7 with 8 joints per lane.
template <int JPL>
struct RenderAcc {
    float4 lo;
};
template <>
struct RenderAcc<8> {
    float4 lo, hi;
};

// JPL: joints (channels) per lane = per 16-B store: 4 fp32 or 8 fp16.
// POSE: the records start from 3-D joints (a.pose) instead of a.joints / a.vis.
// AUG: every painted joint is scaled and cut by its record of a.aug, and the output is clamped at 1.
template <bool POSE, bool AUG>
using RenderKernelArgs = std::conditional_t<AUG, WithAug<std::conditional_t<POSE, RenderPoseArgs, RenderArgs>>,
                                            std::conditional_t<POSE, RenderPoseArgs, RenderArgs>>;

template <int CP, int JPL, bool POSE = false, bool AUG = false>
__global__ __launch_bounds__(kRenderThreads) void render_keypoints_kernel(const RenderKernelArgs<POSE, AUG> a) {
    constexpr int QP = CP / JPL;              // channel groups (one 16-B piece) per pixel
    constexpr int PPP = kRenderThreads / QP;  // pixels per pass
    constexpr int PASSES = kTileW * kBandH / PPP;
    constexpr int SH = JPL == 4 ? 2 : 3;  // log2 JPL
    extern __shared__ double2 render_lds[];
    // kept records per tile and channel group; three sets in turn, so that one barrier per tile orders
    // a set's reset, its fill and its readers
    __shared__ int kept_n[3][QP];
    __shared__ unsigned short kept[3][QP][kMaxRenderP * JPL];  // id = record * JPL + channel in group < 2^13
    __shared__ int band_n;

    const int tid = threadIdx.x;
    const int bv = blockIdx.x / a.bands, ty0 = (blockIdx.x % a.bands) * kBandH;
    const int P = a.P, J = a.J, H = a.H, W = a.W;
    const int nrec = P * J;
    double2 *q = render_lds;                                             // [nrec] joint / stride
    RenderRec *recs = reinterpret_cast<RenderRec *>(q + nrec);           // [nrec]
    RenderPerson *pers = reinterpret_cast<RenderPerson *>(recs + nrec);  // [P]
    unsigned short *band = reinterpret_cast<unsigned short *>(pers + P);  // [nrec] records meeting the band
    unsigned char *seen2d = reinterpret_cast<unsigned char *>(band + nrec);  // [nrec] 2-D visibility (POSE only)

    int cnt;
    if constexpr (POSE)
        cnt = min(max(a.pose.count[bv / a.pose.V], 0), P);
    else
        cnt = min(max(a.count[bv], 0), P);
    const int live = cnt * J;
    if (tid < 3 * QP) kept_n[tid / QP][tid % QP] = 0;
    if (tid == 0) band_n = 0;

    if constexpr (POSE) {
        // q = project(joint3d) / stride; every band's block computes the same values, band 0 also
        // writes the optional outputs (rows at or beyond count as zeros)
        const PoseArgs &ps = a.pose;
        const int b = bv / ps.V;
        const double *cam = pose_camera(ps, b, bv - b * ps.V);
        const bool emit = ty0 == 0 && (ps.joints2d != nullptr || ps.vis2d != nullptr);
        for (int r = tid; r < (emit ? nrec : live); r += kRenderThreads) {
            double qx = 0.0, qy = 0.0;
            bool vis = false;
            if (r < live) {
                const long long e = (long long)b * nrec + r;
                vis = project_pose_point(ps.joints3d + e * 3, ps.vis3d == nullptr || ps.vis3d[e] != 0, cam, ps, qx,
                                         qy);
                q[r] = make_double2(qx / a.stride_x, qy / a.stride_y);
                seen2d[r] = vis ? 1 : 0;
            }
            if (emit) {
                const long long o = (long long)bv * nrec + r;
                if (ps.joints2d) {
                    ps.joints2d[o * 2] = qx;
                    ps.joints2d[o * 2 + 1] = qy;
                }
                if (ps.vis2d) ps.vis2d[o] = vis ? 1 : 0;
            }
        }
    } else {
        // q = joint / stride for the rows below count (the padded rows are never read)
        for (int r = tid; r < live; r += kRenderThreads) {
            const long long e = ((long long)bv * nrec + r) * 2;
            double jx, jy;
            if (a.joints_f64) {
                const double *src = reinterpret_cast<const double *>(a.joints);
                jx = src[e];
                jy = src[e + 1];
            } else {
                const float *src = reinterpret_cast<const float *>(a.joints);
                jx = (double)src[e];
                jy = (double)src[e + 1];
            }
            q[r] = make_double2(jx / a.stride_x, jy / a.stride_y);
        }
    }
    __syncthreads();

    // per person: compute_human_scale over all J joints (visibility plays no part), the sigma and the patch
    if (tid < cnt) {
        double minx = q[tid * J].x, maxx = minx, miny = q[tid * J].y, maxy = miny;
        bool ok = true;
        for (int j = 0; j < J; ++j) {
            const double2 v = q[tid * J + j];
            ok = ok && isfinite(v.x) && isfinite(v.y);
            minx = fmin(minx, v.x);
            maxx = fmax(maxx, v.x);
            miny = fmin(miny, v.y);
            maxy = fmax(maxy, v.y);
        }
        const double ext = fmax(maxy - miny, maxx - minx);
        const double scale = 2.0 * fmin(fmax(ext * ext, 1.0 / 4 * 9216.0), 4 * 9216.0);
        const double cur = a.sigma * sqrt(scale / (96.0 * 96.0));
        const double tmp = cur * 3.0;
        const double size = 2.0 * tmp + 1.0;
        RenderPerson pr;
        pr.tmp = tmp;
        pr.n = trunc_int(ceil(size));
        pr.c0 = trunc_int(floor(size / 2.0));
        pr.inv = (float)(1.0 / (2.0 * (cur * cur)));
        pr.ok = ok ? 1 : 0;
        pers[tid] = pr;
    }
    __syncthreads();

    // per joint: the window, clipped as numpy's slices clip it; listed if it meets this band
    for (int r = tid; r < live; r += kRenderThreads) {
        const int p = r / J, j = r - p * J;
        const RenderPerson pr = pers[p];
        RenderRec rec;
        rec.x0 = rec.x1 = rec.y0 = rec.y1 = rec.cx = rec.cy = 0;
        rec.inv = pr.inv;
        rec.j = j;
        bool seen;
        if constexpr (POSE)
            seen = seen2d[r] != 0;
        else
            seen = a.vis == nullptr || a.vis[(long long)bv * nrec + r] != 0;
        if (pr.ok && seen) {
            const int mux = trunc_int(q[r].x), muy = trunc_int(q[r].y);
            const int ulx = trunc_int((double)mux - pr.tmp), uly = trunc_int((double)muy - pr.tmp);
            const int brx = trunc_int(((double)mux + pr.tmp) + 1.0), bry = trunc_int(((double)muy + pr.tmp) + 1.0);
            if (!(ulx >= W || uly >= H || brx < 0 || bry < 0)) {
                rec.x0 = max(0, ulx);
                rec.y0 = max(0, uly);
                rec.x1 = (int)min((long long)min(brx, W), (long long)ulx + pr.n);
                rec.y1 = (int)min((long long)min(bry, H), (long long)uly + pr.n);
                rec.cx = ulx + pr.c0;
                rec.cy = uly + pr.c0;
            }
        }
        if (rec.x0 < rec.x1 && rec.y0 < ty0 + kBandH && rec.y1 > ty0) {
            recs[r] = rec;
            if constexpr (AUG) {  // over q[r], which only this thread read since the last barrier
                const long long e = (long long)bv * nrec + r;
                const short *rc = a.aug.rect + e * 4;
                AugRec ar;
                ar.scale = a.aug.scale[e];
                ar.pc = pr.c0;
                ar.r0 = rc[0] < 0 ? (short)0 : rc[0];
                ar.r1 = rc[1] < 0 ? (short)0 : rc[1];
                ar.c0 = rc[2] < 0 ? (short)0 : rc[2];
                ar.c1 = rc[3] < 0 ? (short)0 : rc[3];
                reinterpret_cast<AugRec *>(q)[r] = ar;
            }
            band[atomicAdd(&band_n, 1)] = (unsigned short)r;
        }
    }
    __syncthreads();

    const int nband = band_n;
    const int grp = tid % QP, pix = tid / QP;
    using OutT = std::conditional_t<JPL == 4, float, _Float16>;
    OutT *obase = reinterpret_cast<OutT *>(a.out) + (long long)bv * H * W * CP + grp * JPL;
    for (int t = 0; t < a.tiles_x; ++t) {
        const int tx0 = t * kTileW, set = t % 3;
        // the listed records that meet this tile, per channel group (at most JPL P each: fits kept[][][])
        for (int i = tid; i < nband; i += kRenderThreads) {
            const int r = band[i];
            if (recs[r].x0 < tx0 + kTileW && recs[r].x1 > tx0) {
                const int j = recs[r].j;
                kept[set][j >> SH][atomicAdd(&kept_n[set][j >> SH], 1)] = (unsigned short)(r * JPL + (j & (JPL - 1)));
            }
        }
        if (tid < QP) kept_n[(t + 1) % 3][tid] = 0;  // (its readers finished before the previous barrier)
        __syncthreads();
        const int nk = kept_n[set][grp];
#pragma unroll
        for (int pass = 0; pass < PASSES; ++pass) {
            const int pp = pass * PPP + pix;
            const int x = tx0 + pp % kTileW, y = ty0 + pp / kTileW;
            RenderAcc<JPL> va;
            float4 &acc = va.lo;
            acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if constexpr (JPL == 8) va.hi = acc;
            for (int i = 0; i < nk; ++i) {
                const int id = kept[set][grp][i];
                const RenderRec rec = recs[id >> SH];
                if (x >= rec.x0 && x < rec.x1 && y >= rec.y0 && y < rec.y1) {
                    const int dxi = x - rec.cx, dyi = y - rec.cy;
                    const float dx = (float)dxi, dy = (float)dyi;
                    float g = expf(-((dx * dx + dy * dy) * rec.inv));
                    if constexpr (AUG) {  // nothing inside the rectangle; a NaN or negative product loses to acc >= 0
                        const AugRec ar = reinterpret_cast<const AugRec *>(q)[id >> SH];
                        const int px = dxi + ar.pc, py = dyi + ar.pc;
                        const bool cut = px >= ar.c0 && px < ar.c1 && py >= ar.r0 && py < ar.r1;
                        g = cut ? 0.0f : g * ar.scale;
                    }
                    const int k = id & (JPL - 1);
                    acc.x = k == 0 ? fmaxf(acc.x, g) : acc.x;
                    acc.y = k == 1 ? fmaxf(acc.y, g) : acc.y;
                    acc.z = k == 2 ? fmaxf(acc.z, g) : acc.z;
                    acc.w = k == 3 ? fmaxf(acc.w, g) : acc.w;
                    if constexpr (JPL == 8) {
                        va.hi.x = k == 4 ? fmaxf(va.hi.x, g) : va.hi.x;
                        va.hi.y = k == 5 ? fmaxf(va.hi.y, g) : va.hi.y;
                        va.hi.z = k == 6 ? fmaxf(va.hi.z, g) : va.hi.z;
                        va.hi.w = k == 7 ? fmaxf(va.hi.w, g) : va.hi.w;
                    }
                }
            }
            if constexpr (AUG) {  // np.clip(target, 0, 1): a factor above 1 lifts the centre pixel over it
                acc = make_float4(fminf(acc.x, 1.0f), fminf(acc.y, 1.0f), fminf(acc.z, 1.0f), fminf(acc.w, 1.0f));
                if constexpr (JPL == 8)
                    va.hi = make_float4(fminf(va.hi.x, 1.0f), fminf(va.hi.y, 1.0f), fminf(va.hi.z, 1.0f),
                                        fminf(va.hi.w, 1.0f));
            }
            if (x < W && y < H) {
                OutT *o = obase + (y * W + x) * CP;
                if constexpr (JPL == 4) {
                    *reinterpret_cast<float4 *>(o) = acc;
                } else {  // one rounding per channel, to nearest even (a plain conversion, as Tensor.half())
                    const f16x8 h = {(_Float16)acc.x,   (_Float16)acc.y,   (_Float16)acc.z,   (_Float16)acc.w,
                                     (_Float16)va.hi.x, (_Float16)va.hi.y, (_Float16)va.hi.z, (_Float16)va.hi.w};
                    *reinterpret_cast<f16x8 *>(o) = h;
                }
            }
        }
    }
}

// The projection alone: one thread per (frame, view, person, joint); rows at or beyond count are
// written as zeros, so every element of both outputs is written.
__global__ __launch_bounds__(kRenderThreads) void project_poses_kernel(const PoseArgs a, int nrec, int J,
                                                                       long long total) {
    const long long i = (long long)blockIdx.x * kRenderThreads + threadIdx.x;
    if (i >= total) return;
    const int bv = (int)(i / nrec), r = (int)(i - (long long)bv * nrec);
    const int b = bv / a.V;
    const int live = min(max(a.count[b], 0), nrec / J) * J;
    double qx = 0.0, qy = 0.0;
    bool vis = false;
    if (r < live) {
        const long long e = (long long)b * nrec + r;
        vis = project_pose_point(a.joints3d + e * 3, a.vis3d == nullptr || a.vis3d[e] != 0,
                                 pose_camera(a, b, bv - b * a.V), a, qx, qy);
    }
    a.joints2d[i * 2] = qx;
    a.joints2d[i * 2 + 1] = qy;
    a.vis2d[i] = vis ? 1 : 0;
}

}  // namespace fvp

namespace fvp {

// Host checks of the 'gt' operands shared by fvp_project_poses and fvp_render_poses3d(_f16).
static int pose_args(const double *joints3d, const unsigned char *vis3d, const int *count, int B, int P, int J,
                     const double *cams64, const int *cam_index, int S, int V, const double *resize_t64, double ori_w,
                     double ori_h, double image_w, double image_h, double *joints2d, unsigned char *vis2d,
                     PoseArgs *a) {
    if (!joints3d || !count || !cams64 || !resize_t64) return FVP_ERR_NULL;
    if (B <= 0 || P <= 0 || J <= 0 || J > kMaxRenderJ || P > kMaxRenderP) return FVP_ERR_SHAPE;
    if (V <= 0 || V > FVP_MAX_VIEWS || S <= 0) return FVP_ERR_SHAPE;
    if ((long long)B * V > 0x7fffffffLL) return FVP_ERR_SHAPE;  // 32-bit frame-view index
    if (!(ori_w > 0.0) || !(ori_h > 0.0) || !(image_w > 0.0) || !(image_h > 0.0) || !isfinite(ori_w) ||
        !isfinite(ori_h) || !isfinite(image_w) || !isfinite(image_h))
        return FVP_ERR_SHAPE;
    a->joints3d = joints3d;
    a->vis3d = vis3d;
    a->count = count;
    a->cams = cams64;
    a->cam_index = cam_index;
    a->resize_t = resize_t64;
    a->joints2d = joints2d;
    a->vis2d = vis2d;
    a->ori_w1 = ori_w - 1.0;
    a->ori_h1 = ori_h - 1.0;
    a->image_w = image_w;
    a->image_h = image_h;
    a->S = S;
    a->V = V;
    return FVP_OK;
}

// Fills the painter's part of the arguments after the host checks both launches share.
static int render_args(int B, int V, int P, int J, int H, int W, double image_w, double image_h, double sigma, int Cp,
                       void *out_cl, bool half, RenderArgs *a) {
    if (B <= 0 || V <= 0 || P <= 0 || J <= 0 || H <= 0 || W <= 0) return FVP_ERR_SHAPE;
    if (J > kMaxRenderJ || P > kMaxRenderP || Cp < J || Cp % 16 || Cp > 32) return FVP_ERR_SHAPE;
    if ((long long)H * W * Cp > 0x7fffffffLL) return FVP_ERR_SHAPE;  // 32-bit element offsets within a view
    if (!(image_w > 0.0) || !(image_h > 0.0) || !(sigma > 0.0) || !isfinite(image_w) || !isfinite(image_h) ||
        !isfinite(sigma))
        return FVP_ERR_SHAPE;
    if (half && (reinterpret_cast<uintptr_t>(out_cl) & 15)) return FVP_ERR_SHAPE;  // 16-B stores
    a->out = out_cl;
    a->stride_x = image_w / (double)W;  // feat_stride = image_size / heatmap_size
    a->stride_y = image_h / (double)H;
    a->sigma = sigma;
    a->P = P;
    a->J = J;
    a->H = H;
    a->W = W;
    a->tiles_x = (W + kTileW - 1) / kTileW;
    a->bands = (H + kBandH - 1) / kBandH;
    if ((long long)B * V * a->bands > 0x7fffffffLL) return FVP_ERR_SHAPE;
    return FVP_OK;
}

static size_t render_lds_bytes(int P, int J) {
    return (size_t)P * J * (sizeof(double2) + sizeof(RenderRec) + sizeof(unsigned short)) +
           (size_t)P * sizeof(RenderPerson);
}

// One of the 16 instantiations: Cp 16 or 32, fp32 (4 joints per lane) or fp16 (8) output.
template <bool POSE, bool AUG>
static int render_dispatch(int Cp, bool half, dim3 grid, size_t lds, void *stream,
                           const RenderKernelArgs<POSE, AUG> &a) {
    const dim3 block(kRenderThreads);
    if (Cp == 16 && !half)
        hipLaunchKernelGGL((render_keypoints_kernel<16, 4, POSE, AUG>), grid, block, lds, (hipStream_t)stream, a);
    else if (!half)
        hipLaunchKernelGGL((render_keypoints_kernel<32, 4, POSE, AUG>), grid, block, lds, (hipStream_t)stream, a);
    else if (Cp == 16)
        hipLaunchKernelGGL((render_keypoints_kernel<16, 8, POSE, AUG>), grid, block, lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((render_keypoints_kernel<32, 8, POSE, AUG>), grid, block, lds, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// Host checks and the launch shared by fvp_render_poses3d (half = false), fvp_render_poses3d_f16 and
// fvp_render_poses3d_aug (aug_scale and aug_rect given).
static int render_poses_launch(const double *joints3d, const unsigned char *vis3d, const int *count, int B, int P,
                               int J, const double *cams64, const int *cam_index, int S, int V,
                               const double *resize_t64, double ori_w, double ori_h, double image_w, double image_h,
                               int H, int W, double sigma, int Cp, void *out_cl, double *joints2d,
                               unsigned char *vis2d, bool half, void *stream, const float *aug_scale = nullptr,
                               const short *aug_rect = nullptr) {
    if (!out_cl) return FVP_ERR_NULL;
    RenderPoseArgs a;
    int st = pose_args(joints3d, vis3d, count, B, P, J, cams64, cam_index, S, V, resize_t64, ori_w, ori_h, image_w,
                       image_h, joints2d, vis2d, &a.pose);
    if (st != FVP_OK) return st;
    st = render_args(B, V, P, J, H, W, image_w, image_h, sigma, Cp, out_cl, half, &a);
    if (st != FVP_OK) return st;
    a.joints = nullptr;
    a.count = nullptr;
    a.vis = nullptr;
    a.joints_f64 = 1;
    const size_t lds = render_lds_bytes(P, J) + (size_t)P * J;  // + the 2-D visibility bytes
    const dim3 grid((unsigned)((long long)B * V * a.bands));
    if (aug_scale) {
        WithAug<RenderPoseArgs> g;
        static_cast<RenderPoseArgs &>(g) = a;
        g.aug.scale = aug_scale;
        g.aug.rect = aug_rect;
        return render_dispatch<true, true>(Cp, half, grid, lds, stream, g);
    }
    return render_dispatch<true, false>(Cp, half, grid, lds, stream, a);
}

// Host checks and the launch shared by the fp32 (half = false), fp16 and augmented (aug_scale and
// aug_rect given) entry points.
static int render_launch(const void *joints, int joints_f64, const int *count, const unsigned char *vis, int B, int V,
                         int P, int J, int H, int W, double image_w, double image_h, double sigma, int Cp, void *out_cl,
                         bool half, void *stream, const float *aug_scale = nullptr, const short *aug_rect = nullptr) {
    if (!joints || !count || !out_cl) return FVP_ERR_NULL;
    RenderArgs a;
    const int st = render_args(B, V, P, J, H, W, image_w, image_h, sigma, Cp, out_cl, half, &a);
    if (st != FVP_OK) return st;
    a.joints = joints;
    a.count = count;
    a.vis = vis;
    a.joints_f64 = joints_f64 != 0;
    const size_t lds = render_lds_bytes(P, J);
    const dim3 grid((unsigned)((long long)B * V * a.bands));
    if (aug_scale) {
        WithAug<RenderArgs> g;
        static_cast<RenderArgs &>(g) = a;
        g.aug.scale = aug_scale;
        g.aug.rect = aug_rect;
        return render_dispatch<false, true>(Cp, half, grid, lds, stream, g);
    }
    return render_dispatch<false, false>(Cp, half, grid, lds, stream, a);
}

}  // namespace fvp

extern "C" int fvp_render_keypoints(const void *joints, int joints_f64, const int *count, const unsigned char *vis,
                                    int B, int V, int P, int J, int H, int W, double image_w, double image_h,
                                    double sigma, int Cp, float *out_cl, void *stream) {
    return fvp::render_launch(joints, joints_f64, count, vis, B, V, P, J, H, W, image_w, image_h, sigma, Cp, out_cl,
                              false, stream);
}

extern "C" int fvp_render_keypoints_f16(const void *joints, int joints_f64, const int *count,
                                        const unsigned char *vis, int B, int V, int P, int J, int H, int W,
                                        double image_w, double image_h, double sigma, int Cp, void *out_cl_f16,
                                        void *stream) {
    return fvp::render_launch(joints, joints_f64, count, vis, B, V, P, J, H, W, image_w, image_h, sigma, Cp,
                              out_cl_f16, true, stream);
}

extern "C" int fvp_project_poses(const double *joints3d, const unsigned char *vis3d, const int *count, int B, int P,
                                 int J, const double *cams64, const int *cam_index, int S, int V,
                                 const double *resize_t64, double ori_w, double ori_h, double image_w, double image_h,
                                 double *joints2d, unsigned char *vis2d, void *stream) {
    if (!joints2d || !vis2d) return FVP_ERR_NULL;
    fvp::PoseArgs a;
    const int st = fvp::pose_args(joints3d, vis3d, count, B, P, J, cams64, cam_index, S, V, resize_t64, ori_w, ori_h,
                                  image_w, image_h, joints2d, vis2d, &a);
    if (st != FVP_OK) return st;
    const long long total = (long long)B * V * P * J;
    const long long blocks = (total + fvp::kRenderThreads - 1) / fvp::kRenderThreads;
    if (blocks > 0x7fffffffLL) return FVP_ERR_SHAPE;
    hipLaunchKernelGGL(fvp::project_poses_kernel, dim3((unsigned)blocks), dim3(fvp::kRenderThreads), 0,
                       (hipStream_t)stream, a, P * J, J, total);
    return (int)hipGetLastError();
}

extern "C" int fvp_render_poses3d(const double *joints3d, const unsigned char *vis3d, const int *count, int B, int P,
                                  int J, const double *cams64, const int *cam_index, int S, int V,
                                  const double *resize_t64, double ori_w, double ori_h, double image_w, double image_h,
                                  int H, int W, double sigma, int Cp, float *out_cl, double *joints2d,
                                  unsigned char *vis2d, void *stream) {
    return fvp::render_poses_launch(joints3d, vis3d, count, B, P, J, cams64, cam_index, S, V, resize_t64, ori_w, ori_h,
                                    image_w, image_h, H, W, sigma, Cp, out_cl, joints2d, vis2d, false, stream);
}

extern "C" int fvp_render_poses3d_f16(const double *joints3d, const unsigned char *vis3d, const int *count, int B,
                                      int P, int J, const double *cams64, const int *cam_index, int S, int V,
                                      const double *resize_t64, double ori_w, double ori_h, double image_w,
                                      double image_h, int H, int W, double sigma, int Cp, void *out_cl_f16,
                                      double *joints2d, unsigned char *vis2d, void *stream) {
    return fvp::render_poses_launch(joints3d, vis3d, count, B, P, J, cams64, cam_index, S, V, resize_t64, ori_w, ori_h,
                                    image_w, image_h, H, W, sigma, Cp, out_cl_f16, joints2d, vis2d, true, stream);
}

extern "C" int fvp_render_keypoints_aug(const void *joints, int joints_f64, const int *count,
                                        const unsigned char *vis, const float *aug_scale, const short *aug_rect,
                                        int B, int V, int P, int J, int H, int W, double image_w, double image_h,
                                        double sigma, int Cp, void *out_cl, int out_half, void *stream) {
    if (!aug_scale || !aug_rect) return FVP_ERR_NULL;
    return fvp::render_launch(joints, joints_f64, count, vis, B, V, P, J, H, W, image_w, image_h, sigma, Cp, out_cl,
                              out_half != 0, stream, aug_scale, aug_rect);
}

extern "C" int fvp_render_poses3d_aug(const double *joints3d, const unsigned char *vis3d, const int *count, int B,
                                      int P, int J, const double *cams64, const int *cam_index, int S, int V,
                                      const double *resize_t64, double ori_w, double ori_h, double image_w,
                                      double image_h, const float *aug_scale, const short *aug_rect, int H, int W,
                                      double sigma, int Cp, void *out_cl, int out_half, double *joints2d,
                                      unsigned char *vis2d, void *stream) {
    if (!aug_scale || !aug_rect) return FVP_ERR_NULL;
    return fvp::render_poses_launch(joints3d, vis3d, count, B, P, J, cams64, cam_index, S, V, resize_t64, ori_w, ori_h,
                                    image_w, image_h, H, W, sigma, Cp, out_cl, joints2d, vis2d, out_half != 0, stream,
                                    aug_scale, aug_rect);
}
