// The backbone's last layer written as fp16 channels-last heatmaps, one launch.
//
// Replaces PoseResNet's final_layer (lib/models/resnet.py:122-128, with
// FINAL_CONV_KERNEL: 1 a 1x1 convolution 256 -> J plus bias) followed by the
// fp32 -> fp16 cast pass: the [pixel][Cp] fp16 rows it writes are the
// [B][V][H][W][Cp] layout fvp_voxelize_cl_f16 / fvp_person_planes_cl_f16 read
// in place.
//
//   out[p][co] = half_rne(scale[co] * sum_ci in[p][ci] * w[ci * ldw + co] + shift[co])   (co < Cout)
//              = +0                                                                  (Cout <= co < Cp)
//
// Shape of the kernel.  By arithmetic the layer is memory-bound (at Cpi = 256
// a pixel is 1 KiB in, 32 B out, 8 KFLOP), so the aim is a clean stream.  A
// block of 128 threads (2 waves) walks tiles of 32 pixels, tile blockIdx.x,
// + gridDim.x, ..., with the next tile's loads in flight during this tile's
// MFMAs (the up2_head_nchw_kernel pattern):
//   0. the tile's rows [32 px][Cpi] arrive by 16-B loads whose lanes walk the
//      rows' consecutive bytes (at Cpi = 256 a wave-load is one pixel's 1 KiB
//      row) and go to LDS as they are, one ds_write_b128 each, pitch Cpi + 4;
//   1. wave v owns pixels 16 v .. 16 v + 15.  The weights are the A operand of
//      v_mfma_f32_16x16x4_f32 and the pixels the B operand, so an accumulator
//      gives a lane 4 consecutive channels of one pixel.  One ds_read_b128 of a
//      pixel's row at channel 16 s + 4 cm feeds 4 successive MFMAs: MFMA k of
//      step s takes channels 16 s + 4 cm + k over its K index cm = lane >> 4.
//      up2_head permutes the activations to [s][kq][c4] in LDS for the same
//      single read; here the block's weights, staged once, carry that
//      permutation instead ([s][cm][co][k]), which saves three LDS stores in
//      four on the per-tile path;
//   2. epilogue in registers: * scale + shift, one conversion to nearest even
//      per channel, 8-B stores -- at Cp = 16 a wave's store is its 16 pixels'
//      512 consecutive bytes.
// Weights, scale and shift live in LDS / registers for the block's life.  A
// pixel's result is one MFMA column: it depends on its own row and the weights
// only, in a fixed K order, not on npix, the grid or its place in a tile.
// Rows at or beyond npix are read from the last real row (addresses clamped)
// and not stored.
#include "fvp_device.h"

namespace fvp {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int kHeadThreads = 128, kHeadTile = 32;
__host__ __device__ constexpr int head_x_pitch(int Cpi) { return Cpi + 4; }  // conflict-free b128 reads
__host__ __device__ constexpr size_t head_lds_bytes(int Cpi, int Cp) {
    return ((size_t)Cpi * Cp + (size_t)kHeadTile * head_x_pitch(Cpi)) * sizeof(float);
}

// MT: 16-channel output tiles (Cp = 16 MT); NU: 16-B loads per thread and tile (>= Cpi / 16).
template <int MT, int NU>
__global__ __launch_bounds__(kHeadThreads) void conv1x1_cl_f16_kernel(const float *__restrict__ in, long long npix,
                                                                      int Cpi, const float *__restrict__ w, int ldw,
                                                                      int Cout, const float *__restrict__ scale,
                                                                      const float *__restrict__ shift,
                                                                      _Float16 *__restrict__ out) {
    constexpr int CP = 16 * MT;
    extern __shared__ __attribute__((aligned(16))) float head_lds[];
    const int XP = head_x_pitch(Cpi);
    float *const wl = head_lds, *const xl = head_lds + Cpi * CP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, cm = lane >> 4;
    const int nq = Cpi >> 2, nx = kHeadTile * nq, ks = Cpi >> 4;
    const float inv_nq = 1.0f / (float)nq;  // e / nq below: exact for e < 2^14, nq <= 128
    const int tiles = (int)((npix + kHeadTile - 1) / kHeadTile);

    // the block's constants: weights as A fragments [s][cm][co][k] <- w[16 s + 4 cm + k][co], columns
    // at or beyond Cout as zeros (never read from w), and each lane's scale / shift
    for (int i = tid; i < Cpi * CP; i += kHeadThreads) {
        const int ci = i / CP, co = i - ci * CP;
        wl[(((ci >> 2) * CP) + co) * 4 + (ci & 3)] = co < Cout ? w[(size_t)ci * ldw + co] : 0.0f;
    }
    float sc[MT][4], sh[MT][4];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = 16 * m + 4 * cm + r;
            sc[m][r] = co < Cout ? scale[co] : 0.0f;
            sh[m][r] = co < Cout ? shift[co] : 0.0f;
        }

    auto load = [&](int tile, f32x4 (&xv)[NU]) {
        // every address clamped into the buffer; what lies past npix is never stored
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int e = min(tid + kHeadThreads * u, nx - 1);
            const int px = (int)(((float)e + 0.5f) * inv_nq), q = e - px * nq;
            const long long p = min((long long)tile * kHeadTile + px, npix - 1);
            xv[u] = *reinterpret_cast<const f32x4 *>(in + (size_t)p * Cpi + 4 * q);
        }
    };
    f32x4 xv[NU];
    if ((int)blockIdx.x < tiles) load(blockIdx.x, xv);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int e = tid + kHeadThreads * u;
            if (e < nx) {
                const int px = (int)(((float)e + 0.5f) * inv_nq), q = e - px * nq;
                *reinterpret_cast<f32x4 *>(xl + px * XP + 4 * q) = xv[u];
            }
        }
        __syncthreads();  // (B1) rows (and, the first time, the weights) staged
        if (tile + (int)gridDim.x < tiles) load(tile + gridDim.x, xv);
        f32x4 acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *xrow = xl + (16 * wave + l16) * XP + 4 * cm;
        const float *wrow = wl + (cm * CP + l16) * 4;
        for (int s = 0; s < ks; ++s) {
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(xrow + 16 * s);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const f32x4 av = *reinterpret_cast<const f32x4 *>(wrow + (s * 4 * CP + 16 * m) * 4);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[k], bv[k], acc[m], 0, 0, 0);
            }
        }
        const long long p = (long long)tile * kHeadTile + 16 * wave + l16;
        if (p < npix) {
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                f16x4 h;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = 16 * m + 4 * cm + r < Cout ? acc[m][r] * sc[m][r] + sh[m][r] : 0.0f;
                    h[r] = (_Float16)v;  // to nearest even, +-inf beyond 65504 (as Tensor.half())
                }
                *reinterpret_cast<f16x4 *>(out + (size_t)p * CP + 16 * m + 4 * cm) = h;
            }
        }
        __syncthreads();  // (B2) rows read: the next tile may overwrite them
    }
}

template <int MT>
static int head_launch(int nu, const void *&fn) {
    switch (nu) {
    case 1: fn = reinterpret_cast<const void *>(conv1x1_cl_f16_kernel<MT, 1>); return 0;
    case 2: fn = reinterpret_cast<const void *>(conv1x1_cl_f16_kernel<MT, 2>); return 0;
    case 4: fn = reinterpret_cast<const void *>(conv1x1_cl_f16_kernel<MT, 4>); return 0;
    case 8: fn = reinterpret_cast<const void *>(conv1x1_cl_f16_kernel<MT, 8>); return 0;
    case 16: fn = reinterpret_cast<const void *>(conv1x1_cl_f16_kernel<MT, 16>); return 0;
    case 32: fn = reinterpret_cast<const void *>(conv1x1_cl_f16_kernel<MT, 32>); return 0;
    }
    return FVP_ERR_SHAPE;
}

}  // namespace fvp

extern "C" int fvp_conv1x1_cl_f16(const float *in, long long npix, int Cpi, const float *w, int ldw, int Cout,
                                  const float *scale, const float *shift, int Cp, void *out_f16, void *stream) {
    using namespace fvp;
    if (!in || !w || !scale || !shift || !out_f16) return FVP_ERR_NULL;
    if (npix <= 0 || Cpi < 16 || Cpi > 512 || Cpi % 16 || (Cp != 16 && Cp != 32) || Cout <= 0 || Cout > Cp ||
        ldw < Cout || (reinterpret_cast<uintptr_t>(in) & 15) || (reinterpret_cast<uintptr_t>(out_f16) & 15))
        return FVP_ERR_SHAPE;
    const long long tiles = (npix + kHeadTile - 1) / kHeadTile;
    if (tiles > 0x7fffffffLL) return FVP_ERR_SHAPE;
    int nu = 1;
    while (nu < Cpi / 16) nu *= 2;  // 16-B loads per thread and tile: 32 px * Cpi / 4 / 128 threads, rounded up
    const void *fn = nullptr;
    const int st = Cp == 16 ? head_launch<1>(nu, fn) : head_launch<2>(nu, fn);
    if (st) return st;
    const size_t lds = head_lds_bytes(Cpi, Cp);
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return (int)hipGetLastError();
    // the blocks walk the tiles in turn: as many as are resident at once (LDS, VGPRs)
    int dev = 0, cus = 256, per_cu = 2;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kHeadThreads, lds) != hipSuccess || per_cu <= 0)
        per_cu = 2;
    const long long slots = (long long)cus * per_cu;
    const long long blocks = tiles < slots ? tiles : slots;
    _Float16 *out = reinterpret_cast<_Float16 *>(out_f16);
    void *args[] = {&in, &npix, &Cpi, &w, &ldw, &Cout, &scale, &shift, &out};
    const hipError_t err =
        hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(kHeadThreads), args, lds, (hipStream_t)stream);
    return err != hipSuccess ? (int)err : (int)hipGetLastError();
}
