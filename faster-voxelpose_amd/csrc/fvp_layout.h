// Channels-last heatmap layout shared by the whole-space and per-person
// gathers (see fvp_voxelize.hip for why): [b][V][H*W][JP] fp32, JP = 4*LPV,
// joints zero padded; out-of-image taps read 0 through a buffer descriptor's
// range check.
#pragma once

#include <type_traits>
#include <utility>

#include "fvp_device.h"

namespace fvp {

constexpr unsigned kOOB = 0x80000000u;  // beyond any descriptor range -> loads return 0

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void *base, unsigned bytes) {
    const unsigned long long p = (unsigned long long)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)p);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(p >> 32));
    void *b = (void *)(((unsigned long long)hi << 32) | lo);
    return __builtin_amdgcn_make_buffer_rsrc(b, (short)0, (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

// The same descriptor as four SGPR words, for the inline-asm LDS-DMA below.
__device__ __forceinline__ u32x4 uniform_rsrc4(const void *base, unsigned bytes) {
    const unsigned long long p = (unsigned long long)base;
    u32x4 r;
    r.x = __builtin_amdgcn_readfirstlane((unsigned)p);
    r.y = __builtin_amdgcn_readfirstlane((unsigned)(p >> 32)) & 0xffffu;  // stride 0
    r.z = __builtin_amdgcn_readfirstlane(bytes);
    r.w = 0x00020000u;
    return r;
}

// One 16-B piece per lane of a global -> LDS copy (buffer_load_dwordx4 ... lds) into the wave's
// 1-KiB run at LDS byte address lds_base (M0; wave-uniform).  Inline asm rather than
// __builtin_amdgcn_raw_ptr_buffer_load_lds: the compiler then does not track the copy as an LDS
// write, so it puts no s_waitcnt vmcnt(0) before the LDS reads of the OTHER stage buffer (with
// the builtin it drained the next stage's copies before every step's reads: a double buffer
// with no overlap).  The caller orders it with counted vmcnt waits and barriers.
__device__ __forceinline__ void lds_dma16(u32x4 rsrc, unsigned lds_base, unsigned voffset) {
    asm volatile("buffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voffset), "s"(rsrc), "{m0}"(lds_base) : "memory");
}

// -- layout pass ----------------------------------------------------------------
// thread = (pixel, joint quad q): reads joints 4q..4q+3 of one pixel (the lanes
// of a wave cover 64/LPV consecutive pixels -> coalesced plane reads), writes
// one float4 (a wave writes a contiguous 1 KiB run; NF > 1: runs of JP*4 B,
// the NF frames of a group interleaved per pixel: [b/NF][V][H*W][NF][JP]).
// (J joints of a slice; Jst = the planes per (frame, view) of the source)
template <int LPV, typename T, int NF = 1>
__global__ __launch_bounds__(256) void heatmaps_to_cl_kernel(const T *__restrict__ hm, float4 *__restrict__ cl, int J,
                                                             int Jst, int HW, int V, long long total_px) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long pxg = gid / LPV;
    const int q = (int)(gid - pxg * LPV);
    if (pxg >= total_px) return;
    const long long bv = pxg / HW;
    const int pix = (int)(pxg - bv * HW);
    const T *__restrict__ src = hm + (size_t)bv * Jst * HW + pix;
    const int j = 4 * q;
    float4 o;
    o.x = (j + 0 < J) ? to_f32(src[(size_t)(j + 0) * HW]) : 0.f;
    o.y = (j + 1 < J) ? to_f32(src[(size_t)(j + 1) * HW]) : 0.f;
    o.z = (j + 2 < J) ? to_f32(src[(size_t)(j + 2) * HW]) : 0.f;
    o.w = (j + 3 < J) ? to_f32(src[(size_t)(j + 3) * HW]) : 0.f;
    if constexpr (NF == 1) {
        cl[pxg * LPV + q] = o;
    } else {
        const long long fr = bv / V;  // frame within the chunk
        const long long g = fr / NF, f = fr - (fr / NF) * NF, v = bv - fr * V;
        cl[(((g * V + v) * HW + pix) * NF + f) * LPV + q] = o;
    }
}

// -- fp16 pixel-pair table ------------------------------------------------------
// [b][V][H][W+1] entries of 64 B; entry (y, e) holds pixels x0 = e-1 and x0+1
// of row y, lane q's 16 B = [x0: joints 4q..4q+3 | x0+1: joints 4q..4q+3] fp16,
// zeros outside the image (J <= 16).  One thread per (entry, q).
template <typename T, int NF = 1>  // T = _Float16; NF frames per entry: [b/NF][V][H][W+1][NF] x 64 B
__global__ __launch_bounds__(256) void heatmaps_to_pairs_kernel(const T *__restrict__ hm,
                                                                uint4 *__restrict__ tab, int J, int H, int W, int V,
                                                                long long total) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int q = (int)(gid & 3);
    const long long ent = gid >> 2;
    const int W1 = W + 1;
    const long long row = ent / W1;
    const int e = (int)(ent - row * W1);
    const long long bv = row / H;
    const int y = (int)(row - bv * H);
    const size_t HW = (size_t)H * W;
    const T *__restrict__ src = hm + (size_t)bv * J * HW + (size_t)y * W;
    unsigned short h[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = 4 * q + k;
        const T z = (T)0.0f;
        const T a = (j < J && e >= 1) ? src[j * HW + e - 1] : z;
        const T b = (j < J && e < W) ? src[j * HW + e] : z;
        h[k] = __builtin_bit_cast(unsigned short, a);
        h[4 + k] = __builtin_bit_cast(unsigned short, b);
    }
    const uint4 val = make_uint4(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16),
                                 h[4] | ((unsigned)h[5] << 16), h[6] | ((unsigned)h[7] << 16));
    if constexpr (NF == 1) {
        tab[gid] = val;
    } else {
        const long long fr = bv / V, v = bv - fr * V;
        const long long g = fr / NF, f = fr - (fr / NF) * NF;
        tab[(((((g * V + v) * H + y) * W1 + e) * NF) + f) * 4 + q] = val;
    }
}

// The same table, one block per (frame group, view, row): the NF frames' J
// joint rows are read with coalesced 4-B loads (a wave covers 256 B of one
// row) into LDS as [NF][16][W+4] halves (pixel x at x+2, zeros at x = -1, W
// and for joints >= J), then the row's (W+1) x NF entries go out as one
// contiguous run of 16-B stores.  The per-entry kernel above reads 2-B values
// per lane (8 loads per 16-B store) and writes 64-B pieces NF*64 B apart:
// C5, 4 frames per entry, 132 -> 97.5 us per launch (profiles/round3/c5/pairs_layout.txt).
// Needs W even (4-B aligned rows); LDS NF*16*(W/2+2)*4 B.
template <int NF>
__global__ __launch_bounds__(256) void pairs_rows_kernel(const _Float16 *__restrict__ hm, uint4 *__restrict__ tab,
                                                         int J, int H, int W, int V) {
    extern __shared__ unsigned s32[];
    const int P2 = W / 2 + 2;  // words per staged joint row
    const int row = blockIdx.x;  // (g * V + v) * H + y
    const int gv = row / H, y = row - gv * H;
    const int g = gv / V, v = gv - g * V;
    const size_t HW = (size_t)H * W;
    for (int t = threadIdx.x; t < NF * 16 * P2; t += 256) {  // the zero borders and padding joints
        const int jr = t / P2, w = t - jr * P2;
        if ((jr & 15) >= J || w == 0 || w == P2 - 1) s32[t] = 0u;
    }
    // all U loads of a lane issued before their LDS writes (clamped, always
    // legal addresses): a row is one dependent HBM round trip per block
    constexpr int U = 16;
    const int HWc = W / 2, total = NF * J * HWc;
    for (int t0 = threadIdx.x; t0 < total; t0 += 256 * U) {
        unsigned val[U];
        int at[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = min(t0 + u * 256, total - 1);
            const int fj = t / HWc, c = t - fj * HWc;
            const int f = fj / J, j = fj - f * J;
            val[u] = reinterpret_cast<const unsigned *>(hm + (((size_t)(g * NF + f) * V + v) * J + j) * HW +
                                                        (size_t)y * W)[c];
            at[u] = (f * 16 + j) * P2 + 1 + c;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (t0 + u * 256 < total) s32[at[u]] = val[u];
    }
    __syncthreads();
    const unsigned short *s16 = reinterpret_cast<const unsigned short *>(s32);
    const int W1 = W + 1;
    uint4 *__restrict__ dst = tab + (size_t)row * W1 * NF * 4;
    for (int t = threadIdx.x; t < W1 * NF * 4; t += 256) {  // t = (e * NF + f) * 4 + q
        const int q = t & 3, ef = t >> 2;
        const int e = ef / NF, f = ef - e * NF;
        const unsigned short *r = s16 + (f * 16 + 4 * q) * (2 * P2) + e + 1;  // pixel e-1, then pixel e
        unsigned h[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            h[k] = r[k * 2 * P2];
            h[4 + k] = r[k * 2 * P2 + 1];
        }
        dst[t] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    }
}

// The same table without LDS, 8 entries per thread (W % 8 == 0, 16-B aligned
// rows): thread = (row, 8-pixel group m, frame f, joint quad q) loads pixels
// 8m .. 8m+7 of its 4 joint rows with one 16-B load each (+ pixel 8m-1), and
// writes entries 8m .. 8m+7 (pixels e-1, e) -- and entry W for the last group.
// A wave's 16 (f, q) lanes of one m write 256 contiguous bytes per entry.
template <int NF>
__global__ __launch_bounds__(256) void pairs_vec8_kernel(const _Float16 *__restrict__ hm, uint4 *__restrict__ tab,
                                                         int J, int H, int W, int V, long long total) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int M = W / 8;
    const int q = (int)(gid & 3);
    const long long r1 = gid >> 2;
    const int f = (int)(r1 % NF);
    const long long r2 = r1 / NF;
    const int m = (int)(r2 % M);
    const long long row = r2 / M;  // (g * V + v) * H + y
    const long long gv = row / H;
    const int y = (int)(row - gv * H);
    const long long g = gv / V, v = gv - g * V;
    const size_t HW = (size_t)H * W;
    unsigned px[4][4], prev[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = 4 * q + k;
        const unsigned short *src = reinterpret_cast<const unsigned short *>(hm) +
                                    (((size_t)(g * NF + f) * V + v) * J + j) * HW + (size_t)y * W;
        uint4 a = make_uint4(0u, 0u, 0u, 0u);
        unsigned b = 0u;
        if (j < J) {
            a = *reinterpret_cast<const uint4 *>(src + 8 * m);
            b = m > 0 ? src[8 * m - 1] : 0u;
        }
        px[k][0] = a.x; px[k][1] = a.y; px[k][2] = a.z; px[k][3] = a.w;
        prev[k] = b;
    }
    auto pix = [&](int k, int i) -> unsigned { return (px[k][i >> 1] >> (16 * (i & 1))) & 0xffffu; };
    const int W1 = W + 1;
    uint4 *__restrict__ dst = tab + ((size_t)row * W1 * NF + f) * 4 + q;
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // entry e = 8m + i: pixels e - 1 and e
        unsigned lo[4], hi[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo[k] = i == 0 ? prev[k] : pix(k, i - 1);
            hi[k] = pix(k, i);
        }
        dst[(size_t)(8 * m + i) * NF * 4] =
            make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16));
    }
    if (m == M - 1) {  // entry W: pixel W - 1 and the zero past the row
        dst[(size_t)W * NF * 4] = make_uint4(pix(0, 7) | (pix(1, 7) << 16), pix(2, 7) | (pix(3, 7) << 16), 0u, 0u);
    }
}

inline size_t pair_frame_bytes(int V, int H, int W) { return (size_t)V * H * (W + 1) * 64; }

// Which kernel lays the pair table out (fvp_pair_layout_kind reports it): 8 entries a
// thread wherever rows are 16-B aligned: C5, 4 frames per entry 98.2 -> 72.5 us, one
// frame 20.4 -> 15.9 us (profiles/round4/pairs8/).  Otherwise row blocks for frame
// groups (a 15 KB row per block leaves its load / store phases exposed at one frame:
// 40.8 vs 20.8 us per entry), and the per-entry kernel for single frames, odd widths,
// 2-B-aligned pointers (a C-ABI caller may pass any fp16 pointer; the row kernel loads
// 4 B) and rows beyond 64 KiB of LDS.
enum PairLayout { kPairsVec8 = 0, kPairsRows = 1, kPairsEntry = 2 };

inline size_t pairs_rows_lds(int NF, int W) { return (size_t)NF * 16 * (W / 2 + 2) * 4; }

inline PairLayout pair_layout_kind(int NF, int W, unsigned long long hm) {
    if (W % 8 == 0 && (hm & 15ull) == 0) return kPairsVec8;
    if (NF > 1 && (hm & 3ull) == 0 && W % 2 == 0 && pairs_rows_lds(NF, W) <= 64 * 1024) return kPairsRows;
    return kPairsEntry;
}

// Launch the pair-table layout for nb frames (a multiple of NF).
template <int NF>
inline void launch_pairs(const _Float16 *hm, int nb, int V, int J, int H, int W, uint4 *tab, hipStream_t s) {
    const PairLayout kind = pair_layout_kind(NF, W, (unsigned long long)hm);
    if (kind == kPairsVec8) {
        const long long total = (long long)nb / NF * V * H * (W / 8) * NF * 4;
        hipLaunchKernelGGL((pairs_vec8_kernel<NF>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, hm, tab,
                           J, H, W, V, total);
    } else if (kind == kPairsRows) {
        hipLaunchKernelGGL((pairs_rows_kernel<NF>), dim3((unsigned)((long long)nb / NF * V * H)), dim3(256),
                           pairs_rows_lds(NF, W), s, hm, tab, J, H, W, V);
    } else {
        const long long total = (long long)nb * V * H * (W + 1) * 4;
        hipLaunchKernelGGL((heatmaps_to_pairs_kernel<_Float16, NF>), dim3((unsigned)((total + 255) / 256)), dim3(256),
                           0, s, hm, tab, J, H, W, V, total);
    }
}

// -- lane-group helpers -----------------------------------------------------------
// Broadcast lane S of each LPV-lane voxel group to the whole group (DPP quad
// permutes for LPV <= 4, ds_swizzle bit mode for 8-lane groups).
template <int LPV, int S>
__device__ __forceinline__ unsigned group_bcast(unsigned x) {
    if constexpr (LPV == 1) {
        return x;
    } else if constexpr (LPV == 2) {
        return (unsigned)__builtin_amdgcn_mov_dpp((int)x, S | (S << 2) | ((2 + S) << 4) | ((2 + S) << 6), 0xf, 0xf,
                                                  false);
    } else if constexpr (LPV == 4) {
        return (unsigned)__builtin_amdgcn_mov_dpp((int)x, S | (S << 2) | (S << 4) | (S << 6), 0xf, 0xf, false);
    } else {
        static_assert(LPV == 8, "voxel groups of 1, 2, 4 or 8 lanes");
        return (unsigned)__builtin_amdgcn_ds_swizzle((int)x, 0x18 | (S << 5));
    }
}

// Unsigned maximum over the lanes of the wave that hold the same group slot
// (lane mod LPV), all in VALU: DPP row rotations by LPV, 2 LPV, .. 8 within each
// 16-lane row, then v_permlane16_swap / v_permlane32_swap (gfx950) across the
// rows.  Every lane ends with its slot's maximum.  (A __shfl_xor chain compiles
// to ds_bpermute, an LDS round trip and an lgkmcnt(0) wait per step.)
template <int LPV>
__device__ __forceinline__ unsigned slot_umax(unsigned m) {
    static_assert(LPV == 1 || LPV == 2 || LPV == 4 || LPV == 8, "voxel groups of 1, 2, 4 or 8 lanes");
    // row_ror:s = DPP control 0x120 + s
    auto ror = [](unsigned v, auto sc) {
        return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x120 + decltype(sc)::value, 0xf, 0xf, false);
    };
    unsigned r;
    if constexpr (LPV <= 1) { r = ror(m, std::integral_constant<int, 1>{}); m = m > r ? m : r; }
    if constexpr (LPV <= 2) { r = ror(m, std::integral_constant<int, 2>{}); m = m > r ? m : r; }
    if constexpr (LPV <= 4) { r = ror(m, std::integral_constant<int, 4>{}); m = m > r ? m : r; }
    r = ror(m, std::integral_constant<int, 8>{});
    m = m > r ? m : r;
    const auto h = __builtin_amdgcn_permlane16_swap(m, m, false, false);
    m = h[0] > h[1] ? h[0] : h[1];
    const auto w = __builtin_amdgcn_permlane32_swap(m, m, false, false);
    return w[0] > w[1] ? w[0] : w[1];
}

template <int LPV, int S>
__device__ __forceinline__ float group_bcast(float x) {
    return __builtin_bit_cast(float, group_bcast<LPV, S>(__builtin_bit_cast(unsigned, x)));
}

// Compile-time loop: f(std::integral_constant<int, K>) for K in the sequence.
template <int... K, typename F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, K...>, F &&f) {
    (f(std::integral_constant<int, K>{}), ...);
}


__device__ __forceinline__ float h_lo(unsigned u) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)(u & 0xffffu));
}
__device__ __forceinline__ float h_hi(unsigned u) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(u >> 16)); }

// fmaf(h, b, c) with h the fp16 in half HI of u, as one v_fma_mix_f32: the
// fp16 -> fp32 conversion is exact and the fma rounds once, so this equals
// fmaf(HI ? h_hi(u) : h_lo(u), b, c) bit for bit -- without the separate
// v_cvt_f32_f16 (the compiler packs the fp32 fmas instead and keeps the
// conversions).  With c = -0.0f it is the product h * b exactly (x + -0 = x,
// signed zeros included).
template <int HI>
__device__ __forceinline__ float fma_h(unsigned u, float b, float c) {
    float d;
    if constexpr (HI)
        asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(u), "v"(b), "v"(c));
    else
        asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(u), "v"(b), "v"(c));
    return d;
}

// Bilinear setup of one voxel-camera (aten grid_sampler_2d, align_corners=True,
// zeros padding): weights nw, ne, sw, se and the byte offsets of the taps
// (kOOB when outside).  CL: 4 pixel offsets.  PAIR: 2 row-entry offsets.
template <bool PAIR>
struct Taps4 {
    static constexpr int NO = PAIR ? 2 : 4;
    unsigned o[NO];
    float w[4];
};

// Top-left tap (x0, y0) of a sample at heatmap pixel (ix, iy).  NaN
// coordinates read in-image taps so the NaN weights propagate (as in
// grid_sample); far-off coordinates are clamped before the int conversion.
__device__ __forceinline__ void tap_origin(float ix, float iy, int W, int H, int &x0, int &y0) {
    const bool nan_ = (ix != ix) || (iy != iy);
    x0 = nan_ ? 0 : (int)fminf(fmaxf(floorf(ix), -4.0f), (float)W + 4.0f);
    y0 = nan_ ? 0 : (int)fminf(fmaxf(floorf(iy), -4.0f), (float)H + 4.0f);
}

template <bool PAIR>
__device__ __forceinline__ Taps4<PAIR> setup_taps(float gx, float gy, float sxs, float sys, int W, int H,
                                                  unsigned unit) {
    Taps4<PAIR> t;
    const float ix = (gx + 1.0f) * sxs;
    const float iy = (gy + 1.0f) * sys;
    const float x0f = floorf(ix), y0f = floorf(iy);
    const float wx = ix - x0f, ex = 1.0f - wx;
    const float ny = iy - y0f, syw = 1.0f - ny;
    t.w[0] = syw * ex;
    t.w[1] = syw * wx;
    t.w[2] = ny * ex;
    t.w[3] = ny * wx;
    int x0, y0;
    tap_origin(ix, iy, W, H, x0, y0);
    const bool vy0 = (unsigned)y0 < (unsigned)H, vy1 = (unsigned)(y0 + 1) < (unsigned)H;
    if constexpr (PAIR) {
        const bool vx = (x0 >= -1) & (x0 < W);
        const unsigned e0 = (unsigned)(y0 * (W + 1) + x0 + 1) * unit;
        t.o[0] = (vx & vy0) ? e0 : kOOB;
        t.o[1] = (vx & vy1) ? e0 + (unsigned)(W + 1) * unit : kOOB;
    } else {
        const bool vx0 = (unsigned)x0 < (unsigned)W, vx1 = (unsigned)(x0 + 1) < (unsigned)W;
        const unsigned p = (unsigned)(y0 * W + x0) * unit;
        t.o[0] = (vy0 & vx0) ? p : kOOB;
        t.o[1] = (vy0 & vx1) ? p + unit : kOOB;
        t.o[2] = (vy1 & vx0) ? p + (unsigned)W * unit : kOOB;
        t.o[3] = (vy1 & vx1) ? p + (unsigned)(W + 1) * unit : kOOB;
    }
    return t;
}

// -- the camera sum of one voxel ----------------------------------------------------
// Where the sampling coordinates come from: a packed per-sequence grid
// (OTF = false), or the camera records, projected on the fly with the exact
// fp32 sequence of project_grid_kernel (OTF = true; used when the grid would
// not stay cache-resident, e.g. 31 cameras x 160x160x64 = 420 MB).  The
// per-person gather samples the fine grid: gs is the fine grid, x_off 0.
struct CoordSource {
    const float *grids;     // packed grids [S][N][GV][2]            (!OTF)
    const float *cams;      // camera records [S][V][FVP_CAM_STRIDE] (OTF)
    const float *resize_t;  // [2][3]                                (OTF)
    fvp_grid_spec gs;       // (OTF) the whole grid: x-row i of a launch is row x_off + i of gs
    ImageConsts im;
    int x_off;              // (OTF) first x-row of an x-slab launch (0: the whole grid)
};

struct NoPark {};

// acc[f][m] = the V cameras' bilinear taps of one voxel, summed in the reference's
// order (fvp_device.h: torch's CPU mean over the views folds complete blocks of 16
// cameras, CASC = V > 16), before the division; `valid` false gives 0.  A group of
// LPV lanes shares the voxel: lane q (qo = 16 q, its bytes within a pixel / pair
// entry) holds joints JPL q .. JPL q + JPL - 1 of the NF frames of a table entry, and
// sets up cameras v0+2q, v0+2q+1 of each group of 2 LPV, which the group picks up
// through lane broadcasts -- one grid load and one tap setup per 2 LPV voxel-cameras.
// Coordinates: the slots of voxel gn of the packed grid behind grs, or the centre
// (wx, wy, wz) projected through the GV camera records at lcam (LDS) with rt / im.
// frame_tab: the frame group's per-camera images of img bytes, entries of NF * pix.
// JPL joints per lane: 4 (a lane's 16 B = 4 fp32 joints, or the pair table's 2 x 4
// fp16) or 8 (fp16 channels-last pixels read in place: 16 B = 8 fp16 joints, so a
// voxel needs half the lanes and a wave's four tap loads serve twice the voxels).
// park (other than NoPark): called as park(v0, sums) at the top of every camera
// group; the caller keeps the completed 16-camera blocks itself (2 LPV divides 16, so
// a block only ever completes at a group's first camera), and there is no register
// fold and no final add here.
// MODE (replay probe, tools/person_probe.hip; the product instantiates 0): 2 = zeros
// instead of the tap loads, 3 = every tap offset off-image (range-checked loads, no
// memory access), 4 = grid loads and tap setup only.
// INPLACE: the running sums are acc itself instead of a local array copied out at the
// end.  The arithmetic is the same; the compiler optimises this function before it
// inlines it, with the sums in registers or behind the reference, and each gather
// keeps the form its registers were tuned with: the whole-space kernels the local
// array (in place, three of the 8-joint cascade kernels move by 1-2 VGPRs), the
// per-person kernels in place (local: person_cl_kernel<2, true, true> 111 VGPRs for
// 115) -- profiles/gather_sum/.
template <int LPV, bool PAIR, bool OTF, bool CASC, int NF, int JPL, int MODE = 0, bool INPLACE = false,
          typename Park = NoPark>
__device__ __forceinline__ void camera_sum(float (&acc)[NF][JPL], bool valid, long long gn, float wx, float wy,
                                           float wz, const __amdgpu_buffer_rsrc_t &grs, const float *lcam,
                                           const float *rt, const ImageConsts &im, const char *frame_tab,
                                           unsigned img, unsigned pix, unsigned qo, int q, int V, int GV, int W, int H,
                                           float sxs, float sys, Park park = {}) {
    static_assert(!PAIR || LPV == 4, "the fp16 pair table has 4 lanes per voxel");
    static_assert(JPL == 4 || (JPL == 8 && !PAIR && NF == 1), "fp16 channels-last: one frame per pixel, no table");
    static_assert(MODE == 0 || (!PAIR && NF == 1 && JPL == 4), "the probe modes: fp32 pixels");
    constexpr bool PARK = !std::is_same<Park, NoPark>::value;
    constexpr int CPG = 2 * LPV;  // cameras per grid load (2 per lane)
    const unsigned unit = pix * NF;  // bytes per entry
    float own[NF][JPL];
    float (&sum)[NF][JPL] = INPLACE ? acc : own;
    float blk[NF][JPL];  // blk (CASC): completed 16-camera blocks (view_sum order)
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int m = 0; m < JPL; ++m) sum[f][m] = blk[f][m] = 0.0f;
    for (int v0 = 0; v0 < V; v0 += CPG) {
        if constexpr (PARK) park(v0, sum);
        // cameras v0+2q, v0+2q+1 of voxel gn (past V: padding, unused)
        float g[4];
        if constexpr (OTF) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const Cam c = load_cam(lcam + min(v0 + 2 * q + h, GV - 1) * FVP_CAM_STRIDE);
                float px, py;
                project_point(c, wx, wy, wz, px, py);
                pixel_to_sample(px, py, rt, im, g[2 * h], g[2 * h + 1]);
            }
        } else {
            // slots v0+2q, v0+2q+1 (past the row: the next voxel's or 0)
            const u32x4 graw = __builtin_amdgcn_raw_buffer_load_b128(grs, (unsigned)((gn * GV + v0 + 2 * q) * 8), 0, 0);
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = __builtin_bit_cast(float, (unsigned)graw[k]);
        }
        // invalid slots sample (-2, -2): off-image, every tap kOOB, contributes exactly 0
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = valid ? g[k] : -2.0f;
        const Taps4<PAIR> t0 = setup_taps<PAIR>(g[0], g[1], sxs, sys, W, H, unit);
        const Taps4<PAIR> t1 = setup_taps<PAIR>(g[2], g[3], sxs, sys, W, H, unit);
        static_for(std::make_integer_sequence<int, CPG>{}, [&](auto kc) {
            constexpr int k = decltype(kc)::value;
            constexpr int S = k >> 1;  // lane of the group that set this camera up
            const int v = v0 + k;
            if (v >= V) return;
            if constexpr (CASC && !PARK) {
                if ((v & 15) == 0 && v > 0) {  // a block of 16 cameras is complete: fold it (fvp_device.h)
#pragma unroll
                    for (int f = 0; f < NF; ++f)
#pragma unroll
                        for (int m = 0; m < JPL; ++m) {
                            blk[f][m] = blk[f][m] + sum[f][m];
                            sum[f][m] = 0.0f;
                        }
                }
            }
            const Taps4<PAIR> &src = (k & 1) ? t1 : t0;
            unsigned o[Taps4<PAIR>::NO];
            unsigned all = kOOB;
#pragma unroll
            for (int m = 0; m < Taps4<PAIR>::NO; ++m) {
                o[m] = group_bcast<LPV, S>(src.o[m]);
                all &= o[m];
            }
            // whole wave off-image (every tap's kOOB bit set): contributes exactly 0
            if (!__builtin_amdgcn_ballot_w64((all & kOOB) == 0u)) return;
            float w[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) w[m] = group_bcast<LPV, S>(src.w[m]);
            if constexpr (MODE == 4) {
#pragma unroll
                for (int m = 0; m < 4; ++m) sum[0][m] = sum[0][m] + w[m] + __builtin_bit_cast(float, o[m]);
                return;
            }
            if constexpr (MODE == 3) {
#pragma unroll
                for (int m = 0; m < 4; ++m) o[m] = kOOB;
            }
            const __amdgpu_buffer_rsrc_t rs = uniform_rsrc(frame_tab + (size_t)v * img, img);
            if constexpr (PAIR) {
                // r0 = [a j0 j1 | a j2 j3 | b j0 j1 | b j2 j3] (row y0), r1 likewise (c, d; row y1)
                u32x4 r0[NF], r1[NF];
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    r0[f] = __builtin_amdgcn_raw_buffer_load_b128(rs, o[0] + f * pix + qo, 0, 0);
                    r1[f] = __builtin_amdgcn_raw_buffer_load_b128(rs, o[1] + f * pix + qo, 0, 0);
                }
#pragma unroll
                for (int f = 0; f < NF; ++f)
                    static_for(std::make_integer_sequence<int, 4>{}, [&](auto mc) {
                        constexpr int m = decltype(mc)::value, HI = m & 1;
                        const unsigned ua = r0[f][m >> 1], ub = r0[f][2 + (m >> 1)];
                        const unsigned uc = r1[f][m >> 1], ud = r1[f][2 + (m >> 1)];
                        // fd*w3 + (fc*w2 + (fb*w1 + fa*w0)), the fp16 taps converted inside the fmas
                        const float t = fma_h<HI>(ua, w[0], -0.0f);
                        sum[f][m] = sum[f][m] + fma_h<HI>(ud, w[3], fma_h<HI>(uc, w[2], fma_h<HI>(ub, w[1], t)));
                    });
            } else {
                u32x4 a[NF], bq[NF], c[NF], d[NF];
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    if constexpr (MODE == 2) {
                        a[f] = bq[f] = c[f] = d[f] = u32x4{0u, 0u, 0u, 0u};
                    } else {
                        a[f] = __builtin_amdgcn_raw_buffer_load_b128(rs, o[0] + f * pix + qo, 0, 0);
                        bq[f] = __builtin_amdgcn_raw_buffer_load_b128(rs, o[1] + f * pix + qo, 0, 0);
                        c[f] = __builtin_amdgcn_raw_buffer_load_b128(rs, o[2] + f * pix + qo, 0, 0);
                        d[f] = __builtin_amdgcn_raw_buffer_load_b128(rs, o[3] + f * pix + qo, 0, 0);
                    }
                }
                if constexpr (JPL == 8) {
                    // word i of a pixel piece = joints 8q+2i (low half), 8q+2i+1 (high half):
                    // fd*w3 + (fc*w2 + (fb*w1 + fa*w0)), the fp16 taps converted inside the fmas
                    static_for(std::make_integer_sequence<int, 8>{}, [&](auto mc) {
                        constexpr int m = decltype(mc)::value, HI = m & 1, wd = m >> 1;
                        const float t = fma_h<HI>(a[0][wd], w[0], -0.0f);
                        sum[0][m] = sum[0][m] +
                                    fma_h<HI>(d[0][wd], w[3], fma_h<HI>(c[0][wd], w[2], fma_h<HI>(bq[0][wd], w[1], t)));
                    });
                } else {
#pragma unroll
                    for (int f = 0; f < NF; ++f)
#pragma unroll
                        for (int m = 0; m < 4; ++m) {
                            const float fa = __builtin_bit_cast(float, (unsigned)a[f][m]);
                            const float fb = __builtin_bit_cast(float, (unsigned)bq[f][m]);
                            const float fc = __builtin_bit_cast(float, (unsigned)c[f][m]);
                            const float fd = __builtin_bit_cast(float, (unsigned)d[f][m]);
                            sum[f][m] = sum[f][m] + __builtin_fmaf(fd, w[3], __builtin_fmaf(fc, w[2],
                                                                   __builtin_fmaf(fb, w[1], fa * w[0])));
                        }
                }
            }
        });
    }
    // the sum's final levels (fvp_device.h): remainder + blocks, or + 0 (a -0 sum becomes +0)
    if constexpr (!PARK) {
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int m = 0; m < JPL; ++m) sum[f][m] = sum[f][m] + (CASC ? blk[f][m] : 0.0f);
    }
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int m = 0; m < JPL; ++m) acc[f][m] = sum[f][m];
}

inline int lanes_per_voxel(int J) { return J <= 4 ? 1 : J <= 8 ? 2 : J <= 16 ? 4 : 8; }

// fp16 channels-last pixels: a lane's 16 B hold 8 joints (J <= 32 per slice).
inline int lanes_per_voxel_h(int J) { return J <= 8 ? 1 : J <= 16 ? 2 : 4; }

inline size_t cl_frame_bytes(int V, int J, int H, int W) {
    return (size_t)V * H * W * 4 * lanes_per_voxel(J) * sizeof(float);
}

template <int LPV, typename T, int NF = 1>
inline void launch_layout(const T *hm, int nb, int V, int J, int Jst, int H, int W, float *cl, hipStream_t s) {
    const long long px = (long long)nb * V * H * W;
    const long long threads = px * LPV;
    hipLaunchKernelGGL((heatmaps_to_cl_kernel<LPV, T, NF>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s,
                       hm, reinterpret_cast<float4 *>(cl), J, Jst, H * W, V, px);
}

// -- planar -> channels-last fp16 --------------------------------------------------
// [N][C][H*W] fp32 or fp16 -> [N][H*W][Cp] fp16 (Cp % 8 == 0, channels C..Cp-1
// zero): thread = (pixel, 8-channel group q) reads 8 planes at its pixel (the
// lanes of a wave cover 64 / (Cp/8) consecutive pixels) and writes one 16-B
// piece; a wave writes a contiguous 1 KiB run.  fp32 -> fp16 rounds to nearest
// even (v_cvt_f16_f32), as Tensor.half().
template <typename T>
__global__ __launch_bounds__(256) void planar_to_cl_half_kernel(const T *__restrict__ in, uint4 *__restrict__ out,
                                                                int C, int HW, int G, long long total_px) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long pxg = gid / G;
    const int q = (int)(gid - pxg * G);
    if (pxg >= total_px) return;
    const long long n = pxg / HW;
    const int pix = (int)(pxg - n * HW);
    const T *__restrict__ src = in + (size_t)n * C * HW + pix;
    unsigned h[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = 8 * q + k;
        const _Float16 v = c < C ? (_Float16)src[(size_t)c * HW] : (_Float16)0.0f;
        h[k] = __builtin_bit_cast(unsigned short, v);
    }
    out[gid] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

}  // namespace fvp
