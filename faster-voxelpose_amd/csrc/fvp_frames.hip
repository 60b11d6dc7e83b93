// uint8 camera frames -> the normalised fp32 views the backbone takes.
//
// The reference makes its network input on the CPU, one view at a time
// (run/service.py:219-282, 360-366: split the 2 x 2 mosaic, ToTensor, Normalize,
// stack, upload fp32; lib/dataset/JointsDataset.py:194-199: the same after a
// BGR -> RGB swap).  Here the uint8 frames are uploaded as they are (a quarter
// of the bytes) and one launch writes [B*VR*VC][3][H][W]: a block owns 8 rows x
// 256 columns of one view, a thread one column of them, so a wave reads 64
// consecutive pixels (192 or 256 contiguous bytes, any alignment) and writes
// three 256-B runs, one per plane.  The values come from the block's 3 x 256
// table (fvp_frames.h), bit for bit the CPU chain.  The u8 stems of
// fvp_conv.hip read the frames themselves and skip this pass.
#include "fvp_frames.h"

namespace fvp {

constexpr int kF2VRows = 8, kF2VCols = 256;

__global__ __launch_bounds__(256) void frames_to_views_kernel(FrameSrc s, int tiles_x, int tiles_y,
                                                              float *__restrict__ out) {
    __shared__ float tab[kFrameTab];
    const int t = threadIdx.x;
    frame_table(tab, s, t, 256);
    __syncthreads();
    const int per_view = tiles_x * tiles_y;
    const int n = blockIdx.x / per_view, tr = blockIdx.x - n * per_view;
    const int ty = tr / tiles_x, y0 = ty * kF2VRows, x = (tr - ty * tiles_x) * kF2VCols + t;
    if (x >= s.W) return;
    const size_t HW = (size_t)s.H * s.W;
    const unsigned char *__restrict__ src = frame_view(s, n) + (long long)x * s.pix_stride;
    float *__restrict__ dst = out + (size_t)n * 3 * HW + x;
    const int k0 = s.swap_rb ? 2 : 0, k2 = 2 - k0;
#pragma unroll
    for (int r = 0; r < kF2VRows; ++r) {
        const int y = y0 + r;
        if (y < s.H) {
            const unsigned char *px = src + y * s.row_stride;
            float *o = dst + (size_t)y * s.W;
            o[0] = tab[px[k0]];
            o[HW] = tab[256 + px[1]];
            o[2 * HW] = tab[512 + px[k2]];
        }
    }
}

}  // namespace fvp

extern "C" int fvp_frames_to_views(const void *frames, int B, const fvp_frame_spec *spec, float *views,
                                   void *stream) {
    if (!frames || !spec || !views) return FVP_ERR_NULL;
    fvp::FrameSrc s;
    int N = 0;
    const int st = fvp::frame_src(frames, B, spec, &s, &N);
    if (st != FVP_OK) return st;
    const int tx = (s.W - 1) / fvp::kF2VCols + 1, ty = (s.H - 1) / fvp::kF2VRows + 1;
    if ((long long)N * tx * ty > 0x7fffffffLL) return FVP_ERR_SHAPE;
    hipLaunchKernelGGL(fvp::frames_to_views_kernel, dim3((unsigned)(N * tx * ty)), dim3(256), 0, (hipStream_t)stream,
                       s, tx, ty, views);
    return (int)hipGetLastError();
}
