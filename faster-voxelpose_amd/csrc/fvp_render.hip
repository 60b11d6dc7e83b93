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
// The per-pixel value is fp32: expf(-(dx^2 + dy^2) * (float)(1 / (2 sigma^2)))
// with the integer offsets from the window's centre pixel ul + floor(size / 2)
// (which is often mu - 1, not mu: the reference's Gaussian sits on its patch).
#include <math.h>

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
    float *out;
    double stride_x, stride_y, sigma;
    int joints_f64, P, J, H, W, tiles_x, bands;
};

// Python's int(): truncation toward zero.  Values beyond +-2^30 pixels are
// pinned there (a C conversion of them is undefined); such a window lies off
// every heatmap either way.
__device__ __forceinline__ int trunc_int(double v) {
    return (int)fmin(fmax(v, -1073741824.0), 1073741824.0);
}

template <int CP>
__global__ __launch_bounds__(kRenderThreads) void render_keypoints_kernel(const RenderArgs a) {
    constexpr int QP = CP / 4;                // channel groups (float4) per pixel
    constexpr int PPP = kRenderThreads / QP;  // pixels per pass
    constexpr int PASSES = kTileW * kBandH / PPP;
    extern __shared__ double2 render_lds[];
    // kept records per tile and channel group; three sets in turn, so that one barrier per tile orders
    // a set's reset, its fill and its readers
    __shared__ int kept_n[3][QP];
    __shared__ unsigned short kept[3][QP][kMaxRenderP * 4];
    __shared__ int band_n;

    const int tid = threadIdx.x;
    const int bv = blockIdx.x / a.bands, ty0 = (blockIdx.x % a.bands) * kBandH;
    const int P = a.P, J = a.J, H = a.H, W = a.W;
    const int nrec = P * J;
    double2 *q = render_lds;                                             // [nrec] joint / stride
    RenderRec *recs = reinterpret_cast<RenderRec *>(q + nrec);           // [nrec]
    RenderPerson *pers = reinterpret_cast<RenderPerson *>(recs + nrec);  // [P]
    unsigned short *band = reinterpret_cast<unsigned short *>(pers + P);  // [nrec] records meeting the band

    const int cnt = min(max(a.count[bv], 0), P);
    const int live = cnt * J;
    if (tid < 3 * QP) kept_n[tid / QP][tid % QP] = 0;
    if (tid == 0) band_n = 0;

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
        const bool seen = a.vis == nullptr || a.vis[(long long)bv * nrec + r] != 0;
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
            band[atomicAdd(&band_n, 1)] = (unsigned short)r;
        }
    }
    __syncthreads();

    const int nband = band_n;
    const int grp = tid % QP, pix = tid / QP;
    float *obase = a.out + (long long)bv * H * W * CP + grp * 4;
    for (int t = 0; t < a.tiles_x; ++t) {
        const int tx0 = t * kTileW, set = t % 3;
        // the listed records that meet this tile, per channel group (at most 4 P each: fits kept[][][])
        for (int i = tid; i < nband; i += kRenderThreads) {
            const int r = band[i];
            if (recs[r].x0 < tx0 + kTileW && recs[r].x1 > tx0) {
                const int j = recs[r].j;
                kept[set][j >> 2][atomicAdd(&kept_n[set][j >> 2], 1)] = (unsigned short)(r * 4 + (j & 3));
            }
        }
        if (tid < QP) kept_n[(t + 1) % 3][tid] = 0;  // (its readers finished before the previous barrier)
        __syncthreads();
        const int nk = kept_n[set][grp];
#pragma unroll
        for (int pass = 0; pass < PASSES; ++pass) {
            const int pp = pass * PPP + pix;
            const int x = tx0 + pp % kTileW, y = ty0 + pp / kTileW;
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (int i = 0; i < nk; ++i) {
                const int id = kept[set][grp][i];
                const RenderRec rec = recs[id >> 2];
                if (x >= rec.x0 && x < rec.x1 && y >= rec.y0 && y < rec.y1) {
                    const float dx = (float)(x - rec.cx), dy = (float)(y - rec.cy);
                    const float g = expf(-((dx * dx + dy * dy) * rec.inv));
                    const int k = id & 3;
                    acc.x = k == 0 ? fmaxf(acc.x, g) : acc.x;
                    acc.y = k == 1 ? fmaxf(acc.y, g) : acc.y;
                    acc.z = k == 2 ? fmaxf(acc.z, g) : acc.z;
                    acc.w = k == 3 ? fmaxf(acc.w, g) : acc.w;
                }
            }
            if (x < W && y < H) *reinterpret_cast<float4 *>(obase + (y * W + x) * CP) = acc;
        }
    }
}

}  // namespace fvp

extern "C" int fvp_render_keypoints(const void *joints, int joints_f64, const int *count, const unsigned char *vis,
                                    int B, int V, int P, int J, int H, int W, double image_w, double image_h,
                                    double sigma, int Cp, float *out_cl, void *stream) {
    using namespace fvp;
    if (!joints || !count || !out_cl) return FVP_ERR_NULL;
    if (B <= 0 || V <= 0 || P <= 0 || J <= 0 || H <= 0 || W <= 0) return FVP_ERR_SHAPE;
    if (J > kMaxRenderJ || P > kMaxRenderP || Cp < J || Cp % 16 || Cp > 32) return FVP_ERR_SHAPE;
    if ((long long)H * W * Cp > 0x7fffffffLL) return FVP_ERR_SHAPE;  // 32-bit element offsets within a view
    if (!(image_w > 0.0) || !(image_h > 0.0) || !(sigma > 0.0) || !isfinite(image_w) || !isfinite(image_h) ||
        !isfinite(sigma))
        return FVP_ERR_SHAPE;
    RenderArgs a;
    a.joints = joints;
    a.count = count;
    a.vis = vis;
    a.out = out_cl;
    a.stride_x = image_w / (double)W;  // feat_stride = image_size / heatmap_size
    a.stride_y = image_h / (double)H;
    a.sigma = sigma;
    a.joints_f64 = joints_f64 != 0;
    a.P = P;
    a.J = J;
    a.H = H;
    a.W = W;
    a.tiles_x = (W + kTileW - 1) / kTileW;
    a.bands = (H + kBandH - 1) / kBandH;
    const long long blocks = (long long)B * V * a.bands;
    if (blocks > 0x7fffffffLL) return FVP_ERR_SHAPE;
    const size_t lds = (size_t)P * J * (sizeof(double2) + sizeof(RenderRec) + sizeof(unsigned short)) +
                       (size_t)P * sizeof(RenderPerson);
    if (Cp == 16)
        hipLaunchKernelGGL(render_keypoints_kernel<16>, dim3((unsigned)blocks), dim3(kRenderThreads), lds,
                           (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(render_keypoints_kernel<32>, dim3((unsigned)blocks), dim3(kRenderThreads), lds,
                           (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
