// uint8 camera frames (fvp_frame_spec) as the kernels read them: the host checks,
// the view addressing and the 3 x 256 normalisation table, shared by the
// stand-alone pass (fvp_frames.hip) and the u8 stems (fvp_conv.hip).
//
// The contract is ToTensor + Normalize on the CPU, three rounded fp32 operations
//   v = ((float)b / 255.0f - mean[c]) / std[c]
// with IEEE-correct divisions (the library's compile flags make a plain `/`
// one).  A byte has 256 values, so every kernel builds the 768 results once per
// block in LDS with exactly these operations and looks pixels up: b * (1/255) or
// a folded b*k + m would differ in hundreds of the 768 entries.
#pragma once

#include <climits>
#include <cmath>

#include "fvp_device.h"

namespace fvp {

struct FrameSrc {
    const unsigned char *base;
    long long frame_stride, vr_stride, vc_stride, row_stride;
    int H, W, VC, V;  // V = VR * VC views per frame
    int pix_stride, swap_rb;
    float mean0, mean1, mean2, std0, std1, std2;  // by output channel (scalars: no indexed kernel arguments)
};

// The checks of include/fvp.h on (frames, B, spec), made before any launch; *N = B * VR * VC.
inline int frame_src(const void *frames, int B, const fvp_frame_spec *sp, FrameSrc *s, int *N) {
    if (!frames || !sp) return FVP_ERR_NULL;
    if (B <= 0 || sp->H <= 0 || sp->W <= 0 || sp->VR <= 0 || sp->VC <= 0) return FVP_ERR_SHAPE;
    if (sp->pix_stride != 3 && sp->pix_stride != 4) return FVP_ERR_SHAPE;
    if (sp->row_stride < (long long)sp->W * sp->pix_stride) return FVP_ERR_SHAPE;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(sp->mean[c]) || !std::isfinite(sp->std[c]) || sp->std[c] == 0.0f) return FVP_ERR_SHAPE;
    const long long v = (long long)sp->VR * sp->VC;  // two positive ints: below 2^62
    if (v > INT_MAX) return FVP_ERR_SHAPE;
    const long long n = v * B;  // below 2^62 again
    if (n > INT_MAX) return FVP_ERR_SHAPE;
    *s = FrameSrc{static_cast<const unsigned char *>(frames),
                  sp->frame_stride,
                  sp->vr_stride,
                  sp->vc_stride,
                  sp->row_stride,
                  sp->H,
                  sp->W,
                  sp->VC,
                  sp->VR * sp->VC,
                  sp->pix_stride,
                  sp->swap_rb != 0,
                  sp->mean[0],
                  sp->mean[1],
                  sp->mean[2],
                  sp->std[0],
                  sp->std[1],
                  sp->std[2]};
    *N = (int)n;
    return FVP_OK;
}

constexpr int kFrameTab = 3 * 256;  // floats: tab[c * 256 + byte]

// Pixel (0, 0) of view n = b * V + r * VC + c.
__device__ __forceinline__ const unsigned char *frame_view(const FrameSrc &s, int n) {
    const int b = n / s.V, v = n - b * s.V, r = v / s.VC, c = v - r * s.VC;
    return s.base + b * s.frame_stride + r * s.vr_stride + c * s.vc_stride;
}

// The table, by every thread of the block; the caller's barrier publishes it.
__device__ __forceinline__ void frame_table(float *tab, const FrameSrc &s, int t, int nthreads) {
    for (int e = t; e < kFrameTab; e += nthreads) {
        const int c = e >> 8;
        const float mean = c == 0 ? s.mean0 : c == 1 ? s.mean1 : s.mean2;
        const float sd = c == 0 ? s.std0 : c == 1 ? s.std1 : s.std2;
        tab[e] = ((float)(e & 255) / 255.0f - mean) / sd;
    }
}

}  // namespace fvp
