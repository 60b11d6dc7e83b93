// Matching step of the reference's dataset.evaluate() methods, for every frame
// of a run in one launch (fvp.evaluate):
//
//   fvp_match_poses   lib/dataset/panoptic.py:220-245  each valid prediction against
//                     the frame's ground-truth people over the visible joints
//   fvp_match_actors  lib/dataset/shelf.py:176-209, campus.py:153-190  each present
//                     actor against the frame's valid predictions converted to the
//                     14-joint skeleton, plus the ten PCP part tests
//
// Arithmetic: plain float64 expressions (-ffp-contract=off, so no fused
// multiply-add), every sum in index order.  numpy's own sums are pairwise and
// np.linalg.norm goes through BLAS, so values agree with the reference to a
// few ulp, not bit for bit; every discrete output (argmin, part bits) is exact
// wherever the decision has a margin above that.
//
// One block per frame; lanes loop over the (prediction, person) pairs, each
// walking the joints in order; the pair means go to LDS and a second pass of
// one lane per output element scans them in index order (np.argmin: the first
// NaN if there is one, otherwise the first minimum).  One writer per output
// element, no atomics, nothing allocated, nothing synchronised.
#include "fvp_device.h"

namespace fvp {

constexpr int kEvalBlock = 128;

// np.argmin / np.min over values visited in index order: a NaN, once held, stays.
__device__ __forceinline__ void first_min(double v, int idx, double &best, int &best_idx) {
    if (best_idx < 0 || (best == best && (v != v || v < best))) {
        best = v;
        best_idx = idx;
    }
}

__device__ __forceinline__ double dist3(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

__global__ __launch_bounds__(kEvalBlock) void match_poses_kernel(
    const float *__restrict__ preds, int K, int J, int C, const double *__restrict__ gt,
    const unsigned char *__restrict__ gt_vis, const int *__restrict__ num_person, int G, double *__restrict__ mpjpe,
    int *__restrict__ gt_index, float *__restrict__ score) {
    __shared__ double pair[FVP_EVAL_MAX_PAIRS];
    const long long i = blockIdx.x;
    const float *p = preds + i * K * J * C;
    const double *g3 = gt + i * G * J * 3;
    const unsigned char *vis = gt_vis + i * G * J;
    const int np = min(max(num_person[i], 0), G);

    for (int t = threadIdx.x; t < K * np; t += kEvalBlock) {
        const int k = t / np, g = t - k * np;
        const float *pk = p + (long long)k * J * C;
        if (!(pk[3] >= 0.0f)) continue;
        double sum = 0.0, count = 0.0;
        for (int j = 0; j < J; ++j) {
            if (!vis[g * J + j]) continue;
            const double *q = g3 + ((long long)g * J + j) * 3;
            sum += dist3((double)pk[j * C], (double)pk[j * C + 1], (double)pk[j * C + 2], q[0], q[1], q[2]);
            count += 1.0;
        }
        pair[k * G + g] = sum / count;  // no visible joint: 0 / 0 = NaN (np.mean of nothing)
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += kEvalBlock) {
        const float *pk = p + (long long)k * J * C;
        double best = __builtin_nan("");
        int best_g = -1;
        if (np > 0 && pk[3] >= 0.0f)
            for (int g = 0; g < np; ++g) first_min(pair[k * G + g], g, best, best_g);
        mpjpe[i * K + k] = best;
        gt_index[i * K + k] = best_g;
        score[i * K + k] = pk[4];
    }
}

// coco2shelf3D (shelf.py:230-256) / coco2campus3D (campus.py:212-230) of one fp32
// [17][C] pose into fp64 [14][3], in the reference's mixed precision: the head
// points are float32 expressions of the float32 joints, the rest float64.
__device__ __forceinline__ void convert_pose(const float *__restrict__ c, int C, int convert, double *__restrict__ o) {
    const int order[12] = {16, 14, 12, 11, 13, 15, 10, 8, 6, 5, 7, 9};
    for (int r = 0; r < 12; ++r)
        for (int d = 0; d < 3; ++d) o[r * 3 + d] = (double)c[order[r] * C + d];
    const double w13[3] = {0.75, 0.75, 1.5};
    for (int d = 0; d < 3; ++d) {
        const float mid_sho = (c[5 * C + d] + c[6 * C + d]) / 2.0f;
        const float head_center = (c[3 * C + d] + c[4 * C + d]) / 2.0f;
        const float head_bottom = (mid_sho + head_center) / 2.0f;
        const float head_top = head_bottom + (head_center - head_bottom) * 2.0f;
        if (convert == 1) {
            o[12 * 3 + d] = (double)head_bottom;
            o[13 * 3 + d] = (double)head_top;
        } else {
            const double c0 = (double)c[d];
            double s12 = (o[8 * 3 + d] + o[9 * 3 + d]) / 2.0;
            double s13 = s12 + (c0 - s12) * w13[d];
            s12 = s12 + (c0 - s12) * 0.5;
            s13 = s13 * 0.75 + (double)head_top * 0.25;
            s12 = s12 * 0.75 + (double)head_bottom * 0.25;
            o[12 * 3 + d] = s12;
            o[13 * 3 + d] = s13;
        }
    }
}

// (error_s + error_e) / 2 <= 0.5 * limb_length (shelf.py:195-198); false with a NaN on either side.
__device__ __forceinline__ bool part_ok(double es, double ee, double len) { return (es + ee) / 2.0 <= 0.5 * len; }

__global__ __launch_bounds__(kEvalBlock) void match_actors_kernel(
    const float *__restrict__ preds, int K, int C, const double *__restrict__ gt,
    const unsigned char *__restrict__ present, int A, int convert, double *__restrict__ mpjpe,
    int *__restrict__ pred_index, unsigned *__restrict__ parts, int *__restrict__ valid_count) {
    __shared__ double pose[FVP_EVAL_MAX_PREDS * 14 * 3];
    __shared__ double pair[FVP_EVAL_MAX_PREDS * FVP_EVAL_MAX_ACTORS];
    __shared__ unsigned char valid[FVP_EVAL_MAX_PREDS];
    const long long i = blockIdx.x;
    const float *p = preds + i * K * 17 * C;
    const double *g3 = gt + i * A * 14 * 3;
    const unsigned char *pres = present + i * A;

    for (int k = threadIdx.x; k < K; k += kEvalBlock) {
        const float *pk = p + (long long)k * 17 * C;
        const bool ok = pk[3] >= 0.0f;
        valid[k] = ok;
        if (ok) convert_pose(pk, C, convert, pose + k * 42);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int k = 0; k < K; ++k) n += valid[k];
        valid_count[i] = n;
    }
    for (int t = threadIdx.x; t < A * K; t += kEvalBlock) {
        const int a = t / K, k = t - a * K;
        if (!pres[a] || !valid[k]) continue;
        const double *q = g3 + a * 42, *o = pose + k * 42;
        double sum = 0.0;
        for (int j = 0; j < 14; ++j)
            sum += dist3(q[j * 3], q[j * 3 + 1], q[j * 3 + 2], o[j * 3], o[j * 3 + 1], o[j * 3 + 2]);
        pair[a * K + k] = sum / 14.0;
    }
    __syncthreads();
    for (int a = threadIdx.x; a < A; a += kEvalBlock) {
        double best = __builtin_nan("");
        int best_k = -1;
        if (pres[a])
            for (int k = 0; k < K; ++k)
                if (valid[k]) first_min(pair[a * K + k], k, best, best_k);
        unsigned bits = 0;
        if (best_k >= 0) {
            const double *q = g3 + a * 42, *o = pose + best_k * 42;
            const int limbs[9][2] = {{0, 1}, {1, 2}, {3, 4}, {4, 5}, {6, 7}, {7, 8}, {9, 10}, {10, 11}, {12, 13}};
            for (int l = 0; l < 9; ++l) {
                const int s = limbs[l][0] * 3, e = limbs[l][1] * 3;
                const double es = dist3(o[s], o[s + 1], o[s + 2], q[s], q[s + 1], q[s + 2]);
                const double ee = dist3(o[e], o[e + 1], o[e + 2], q[e], q[e + 1], q[e + 2]);
                const double len = dist3(q[s], q[s + 1], q[s + 2], q[e], q[e + 1], q[e + 2]);
                if (part_ok(es, ee, len)) bits |= 1u << l;
            }
            double ph[3], gh[3];
            for (int d = 0; d < 3; ++d) {
                ph[d] = (o[2 * 3 + d] + o[3 * 3 + d]) / 2.0;
                gh[d] = (q[2 * 3 + d] + q[3 * 3 + d]) / 2.0;
            }
            const double es = dist3(ph[0], ph[1], ph[2], gh[0], gh[1], gh[2]);
            const double ee = dist3(o[36], o[37], o[38], q[36], q[37], q[38]);
            const double len = dist3(gh[0], gh[1], gh[2], q[36], q[37], q[38]);
            if (part_ok(es, ee, len)) bits |= 1u << 9;
        }
        mpjpe[i * A + a] = best;
        pred_index[i * A + a] = best_k;
        parts[i * A + a] = bits;
    }
}

}  // namespace fvp

extern "C" int fvp_match_poses(const float *preds, int N, int K, int J, int C, const double *gt,
                               const unsigned char *gt_vis, const int *num_person, int G, double *mpjpe,
                               int *gt_index, float *score, void *stream) {
    if (!preds || !gt || !gt_vis || !num_person || !mpjpe || !gt_index || !score) return FVP_ERR_NULL;
    if (N < 0 || K <= 0 || J <= 0 || G <= 0 || C < 5) return FVP_ERR_SHAPE;
    if (J > FVP_MAX_JOINTS || C > FVP_EVAL_MAX_CHANNELS || (long long)K * G > FVP_EVAL_MAX_PAIRS) return FVP_ERR_SHAPE;
    if (N == 0) return FVP_OK;
    hipLaunchKernelGGL(fvp::match_poses_kernel, dim3((unsigned)N), dim3(fvp::kEvalBlock), 0, (hipStream_t)stream,
                       preds, K, J, C, gt, gt_vis, num_person, G, mpjpe, gt_index, score);
    return (int)hipGetLastError();
}

extern "C" int fvp_match_actors(const float *preds, int N, int K, int C, const double *gt,
                                const unsigned char *present, int A, int convert, double *mpjpe, int *pred_index,
                                unsigned *parts, int *valid_count, void *stream) {
    if (!preds || !gt || !present || !mpjpe || !pred_index || !parts || !valid_count) return FVP_ERR_NULL;
    if (N < 0 || K <= 0 || A <= 0 || C < 5 || convert < 0 || convert > 1) return FVP_ERR_SHAPE;
    if (K > FVP_EVAL_MAX_PREDS || A > FVP_EVAL_MAX_ACTORS || C > FVP_EVAL_MAX_CHANNELS) return FVP_ERR_SHAPE;
    if (N == 0) return FVP_OK;
    hipLaunchKernelGGL(fvp::match_actors_kernel, dim3((unsigned)N), dim3(fvp::kEvalBlock), 0, (hipStream_t)stream,
                       preds, K, C, gt, present, A, convert, mpjpe, pred_index, parts, valid_count);
    return (int)hipGetLastError();
}
