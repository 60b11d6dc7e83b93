// Per-person voxel cubes from the cached fine sample grid (A11-A13) and the
// JLN xy/xz/yz max-projections (A8).
//
// fvp_person_planes replaces project_individual.ProjectLayer.forward
// (project_individual.py:222-293) and, fused, the max-projections of
// joint_localization_net.py:158-160, for every proposal of a batch in one
// launch and without host syncs: each block recomputes its proposal's window
// (centers_tl, margins, start/end, skip flag, :255-275) from the proposal
// row.  The frames are first re-laid out channels-last (fvp_layout.h) so the
// taps are quad-coalesced (see fvp_voxelize.hip).
//
// max_planes (planes of an already materialised cube) replaces torch.cat([max(c,4), max(c,3), max(c,2)])
// (joint_localization_net.py:158-160): one block per (person, joint) reads the
// S^3 cube once; lane = z, each wave owns S/4 y-rows; yz is a register max
// over x, xz a register + LDS max over y, xy a wave reduction over z.
#include "fvp_layout.h"

namespace fvp {

struct Window {
    int ctl[3], start[3], end[3];
    bool skip;
};

__device__ __forceinline__ Window person_window(const float *__restrict__ pc, const fvp_person_spec &s) {
    Window w;
    // centers_tl = round(center * scale + bias).int()   (:255, round half to even)
#pragma unroll
    for (int a = 0; a < 3; ++a) w.ctl[a] = (int)rintf(pc[a] * s.scale[a] + s.bias[a]);
    // mask = ((1 - bbox) / 2 * (vpa[0:2] - 1)).int(), negatives -> 0, z margin 0  (:262-265)
    int m[3];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const float f = ((1.0f - pc[5 + a]) / 2.0f) * (float)(s.bins[a] - 1);
        int mi = (int)f;  // trunc toward zero, as .int()
        m[a] = mi < 0 ? 0 : mi;
    }
    m[2] = 0;
    w.skip = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int lo = w.ctl[a] + m[a];
        const int hi = w.ctl[a] + s.bins[a] - m[a];
        w.start[a] = lo >= 0 ? lo : 0;                   // :268
        w.end[a] = hi <= s.fine[a] ? hi : s.fine[a];     // :269
        w.skip |= (w.start[a] >= w.end[a]);              // :274-275
    }
    return w;
}

// planes: [3P][J][S][S]; block (p, j); 256 threads = 4 waves, lane = z.
__global__ __launch_bounds__(256) void max_planes_kernel(const float *__restrict__ cubes, float *__restrict__ planes,
                                                         int P, int J, int S) {
    __shared__ float xz_part[4][64];
    const int p = blockIdx.x / J, j = blockIdx.x % J;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool zok = lane < S;
    const size_t SS = (size_t)S * S;
    const float *__restrict__ c = cubes + ((size_t)p * J + j) * SS * S;
    float *__restrict__ pxy = planes + ((size_t)(0 * P + p) * J + j) * SS;
    float *__restrict__ pxz = planes + ((size_t)(1 * P + p) * J + j) * SS;
    float *__restrict__ pyz = planes + ((size_t)(2 * P + p) * J + j) * SS;
    constexpr int kRows = 16;  // y rows per wave (S <= 64)
    float yz[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) yz[r] = -INFINITY;

    for (int x = 0; x < S; ++x) {
        float xzm = -INFINITY;
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int y = wave + 4 * r;
            const bool ok = zok && y < S;
            const float v = ok ? c[((size_t)x * S + y) * S + lane] : -INFINITY;
            yz[r] = nanmax(yz[r], v);
            xzm = nanmax(xzm, v);
            // xy[x][y] = max over z (wave reduction; y is wave-uniform)
            float m = v;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) m = nanmax(m, __shfl_xor(m, off));
            if (lane == 0 && y < S) pxy[(size_t)x * S + y] = m;
        }
        xz_part[wave][lane] = xzm;
        __syncthreads();
        if (wave == 0 && zok) {
            float m = xz_part[0][lane];
            m = nanmax(m, xz_part[1][lane]);
            m = nanmax(m, xz_part[2][lane]);
            m = nanmax(m, xz_part[3][lane]);
            pxz[(size_t)x * S + lane] = m;
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int y = wave + 4 * r;
        if (zok && y < S) pyz[(size_t)y * S + lane] = yz[r];
    }
}

// Planes of cubes deeper than 64 (one thread per plane cell, a loop over the
// reduced axis; NaN-propagating like torch.max).
__global__ __launch_bounds__(256) void max_planes_generic_kernel(const float *__restrict__ cubes,
                                                                 float *__restrict__ planes, int P, int J, int S) {
    const size_t SS = (size_t)S * S;
    const size_t per_plane = (size_t)P * J * SS;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * per_plane) return;
    const int k = (int)(e / per_plane);  // 0 xy (max z), 1 xz (max y), 2 yz (max x)
    const size_t r = e - k * per_plane;
    const size_t pj = r / SS;
    const int a = (int)((r - pj * SS) / S), b = (int)(r - pj * SS - (size_t)a * S);
    const float *__restrict__ c = cubes + pj * SS * S;
    const size_t base = k == 0 ? ((size_t)a * S + b) * S : k == 1 ? (size_t)a * SS + b : (size_t)a * S + b;
    const size_t step = k == 0 ? 1 : k == 1 ? (size_t)S : SS;
    float m = -INFINITY;
    for (int t = 0; t < S; ++t) m = nanmax(m, c[base + t * step]);
    planes[e] = m;
}

// Channels-last per-person kernel (batched over frames, optional fused planes).
// Block = (proposal p, one y-row, x part, 64-deep z chunk); threads = 64 z-lanes
// x LPV joint quads.  The block walks the x-planes of its row:
//   xy[x][y] = max_z   -> per-wave z maxima in VALU (slot_umax), then either kept
//                         in LDS and stored once per (x, joint) at the block's end
//                         (xy_direct: the block owns the row's xy cells) or one
//                         atomicMax per wave into the pre-zeroed plane
//   yz[y][z] = max_x   -> registers (the block owns its row), stored at the end
//                         (atomics into a pre-zeroed plane when x is split)
//   xz[x][z] = max_y   -> one atomicMax per (x, z, joint) into the pre-zeroed plane
// (values are clamped to [0,1] or NaN, so unsigned order == float order.)
// Outside-window voxels are 0 exactly as in the reference cube.
// Sampling coordinates of the fine grid: the packed per-sequence grid
// (OTF = false) or projected on the fly from the camera records with the fp32
// sequence of fvp_project_grid (OTF = true: no 197 MB fine grid to stream).
// (CoordSource, fvp_layout.h, with gs the fine grid; the kernels take the packed fine grid
// as an argument of its own, fgrid: read through the struct, person_cl_h8_kernel<1, true>
// needs 75 VGPRs instead of 72 and loses an occupancy step.)
// MODE (replay probe, tools/person_probe.hip; the product launches 0): 1 = no
// plane reductions / stores (the sums folded into `offset`), 2 / 3 / 4 = inside the
// camera sum (camera_sum, fvp_layout.h; 4 also without the planes),
// 5 / 6 = no xz / xy plane atomics or stores, 7 = xz atomics from even z lanes only,
// 8 = plain stores instead of the xz atomics (timing only: wrong maxima).
// JPL joints per lane: 4 (fp32 pixels) or 8 (fp16 pixels, JP = 8 * LPV joints per block).
template <int LPV, bool OTF, bool CASC, int MODE, int JPL>
__device__ __forceinline__ void person_cl_body(const float *__restrict__ cl,
                                               const float *__restrict__ fgrid, const CoordSource &src,
                                               const float *__restrict__ props,
                                               const int32_t *__restrict__ frame_of, const fvp_person_spec &s,
                                               float *__restrict__ cubes, float *__restrict__ planes,
                                               float *__restrict__ offset, int P, int V, int J, int Jst,
                                               int H, int W, int xmap, int xsplit, int zsplit,
                                               unsigned pix_bytes, int xy_direct) {
    constexpr int JP = JPL * LPV;  // joint slots of the block
    __shared__ float lcam[OTF ? 64 * FVP_CAM_STRIDE : 1];  // OTF: camera records (V <= 64)
    // xy_direct: [wave][x][joint slot] per-wave z maxima, stored at the block's end
    constexpr bool DXY = LPV <= 4;
    __shared__ unsigned lxy[DXY ? LPV * 64 * JP : 1];
    const int SX = s.bins[0], SY = s.bins[1], SZ = s.bins[2];
    // XCD-aware: each XCD runs whole proposals, so the rows of one proposal
    // (walking x together) share that XCD's L2 footprint (L2 hit 35 % with
    // round-robin placement)
    const int L = xmap ? xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    // block -> (proposal, row, x part, z chunk): a proposal's blocks stay contiguous
    const int parts = xsplit * zsplit;
    const int p = L / (SY * parts);
    const int rem = L - p * SY * parts;
    const int y = rem / parts;
    const int part = rem - y * parts;
    const int xpart = part % xsplit, zc = part / xsplit;
    const Window w = person_window(props + (size_t)p * 7, s);
    if (offset && y == 0 && part == 0 && threadIdx.x < 3) {
        const int a = threadIdx.x;
        // (JPL == 8: the window's element by selects -- indexing the register-held struct
        // by thread puts it in scratch; the fp32 kernels keep their code as it was)
        const int ca = JPL == 8 ? (a == 0 ? w.ctl[0] : a == 1 ? w.ctl[1] : w.ctl[2]) : w.ctl[a];
        offset[(size_t)p * 3 + a] =
            ((float)ca / (float)(s.fine[a] - 1)) * s.whole_size[a] - s.whole_size[a] / 2.0f + s.ind_size[a] / 2.0f;
    }
    const int lane = threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int zl = zc * 64 + (int)threadIdx.x / LPV, q = threadIdx.x % LPV;
    const int b = frame_of ? frame_of[p] : 0;
    const unsigned HW = (unsigned)(H * W);
    const unsigned img = HW * pix_bytes;  // pix_bytes >= JP * 4: one channels-last pixel
    const unsigned qo = (unsigned)q * 16u;
    const float sxs = (float)(W - 1) * 0.5f, sys = (float)(H - 1) * 0.5f;
    const float fV = (float)V;
    const int GV = V + (V & 1);
    const long long FN = (long long)s.fine[0] * s.fine[1] * s.fine[2];
    __amdgpu_buffer_rsrc_t grs;
    float rt[6];
    if constexpr (OTF) {
        for (int e = threadIdx.x; e < GV * FVP_CAM_STRIDE; e += 64 * LPV)
            lcam[e] = e < V * FVP_CAM_STRIDE ? src.cams[e] : 0.0f;
#pragma unroll
        for (int k = 0; k < 6; ++k) rt[k] = src.resize_t[k];
        __syncthreads();
    } else {
        grs = uniform_rsrc(fgrid, (unsigned)(FN * GV * 8));
    }
    const char *__restrict__ frame_cl = (const char *)cl + (size_t)b * V * img;
    const size_t SS = (size_t)SY * SZ;
    const size_t S3 = (size_t)SX * SS;
    // (planes / cubes start at this joint slice; Jst joints per proposal)
    float *xy_pl = planes ? planes + (size_t)p * Jst * SX * SY : nullptr;
    float *xz_pl = planes ? planes + ((size_t)P + p) * Jst * SX * SZ : nullptr;
    float *yz_pl = planes ? planes + ((size_t)2 * P + p) * Jst * SY * SZ : nullptr;
    const bool zok = zl < SZ;
    const int gz = w.ctl[2] + zl;
    const bool zin = zok && gz >= w.start[2] && gz < w.end[2];
    const int gy = w.ctl[1] + y;
    const bool row_in = gy >= w.start[1] && gy < w.end[1];  // block-uniform

    // plane maxima on the float bits: every voxel value is +0 .. 1 or NaN (the
    // mean is clamped and +0.0f turns a -0 into +0), so unsigned order is float
    // order with NaN on top (torch.max: NaN wins) -- one v_max_u32 per step
    // instead of a NaN-aware float max (compares + select); +0 is neutral
    unsigned yzacc[JPL];
#pragma unroll
    for (int k = 0; k < JPL; ++k) yzacc[k] = 0u;

    // xy_direct (host: one x part, one z chunk, S <= 64, LPV <= 4 for every joint
    // slice): the block owns its row's xy cells, so the per-wave z maxima go to LDS
    // and leave as plain stores at the block's end -- no atomics (one per wave and x
    // step cost ~0.6 us per proposal, probe mode 6: non-returning atomics count in
    // vmcnt and the next taps wait on them)
    const bool defer = DXY && planes && xy_direct;
    if (defer) {
        for (int e = lane; e < 64 * JP; e += 64) lxy[wave * 64 * JP + e] = 0u;
    }
    int x_lo = xpart * SX / xsplit, x_hi = (xpart + 1) * SX / xsplit;
    if (!cubes) {
        // planes only: the x-planes outside the window are all 0, which changes none
        // of the maxima (pre-zeroed xy / xz planes, yzacc >= 0)
        // -- walk the window only
        if (w.skip || !row_in) {
            x_hi = x_lo;
        } else {
            x_lo = max(x_lo, w.start[0] - w.ctl[0]);
            x_hi = min(x_hi, w.end[0] - w.ctl[0]);
        }
    }
    for (int x = x_lo; x < x_hi; ++x) {
        const int gx = w.ctl[0] + x;
        const bool xin = !w.skip && gx >= w.start[0] && gx < w.end[0];
        const bool valid = xin && zin && row_in;
        // the clamped-mean input of fine voxel (gx, gy, gz): the V cameras' taps summed in the
        // reference's order (project_individual.py:278-283); outside the window or the cube: 0
        float acc[1][JPL];
#pragma unroll
        for (int k = 0; k < JPL; ++k) acc[0][k] = 0.0f;
        if (__builtin_amdgcn_ballot_w64(valid)) {
            const long long gn = valid ? ((long long)gx * s.fine[1] + gy) * s.fine[2] + gz : 0;
            float wxc = 0.f, wyc = 0.f, wzc = 0.f;  // OTF: fine voxel centre (compute_grid at fine resolution)
            if constexpr (OTF) {
                wxc = axis_coord(src.gs.start[0], src.gs.end[0], s.fine[0], valid ? gx : 0, src.gs.center[0]);
                wyc = axis_coord(src.gs.start[1], src.gs.end[1], s.fine[1], valid ? gy : 0, src.gs.center[1]);
                wzc = axis_coord(src.gs.start[2], src.gs.end[2], s.fine[2], valid ? gz : 0, src.gs.center[2]);
            }
            camera_sum<LPV, false, OTF, CASC, 1, JPL, (MODE >= 2 && MODE <= 4) ? MODE : 0, true>(
                acc, valid, gn, wxc, wyc, wzc, grs, lcam, rt, src.im, frame_cl, img, pix_bytes, qo, q, V, GV, W, H, sxs,
                sys);
        }
        float o[JPL];
        unsigned ou[JPL];
#pragma unroll
        for (int k = 0; k < JPL; ++k) {
            // clamp(0,1) of the mean; +0.0f turns a -0 into +0 (unsigned max order below)
            o[k] = valid ? clampf(acc[0][k] / fV, 0.0f, 1.0f) + 0.0f : 0.0f;
            ou[k] = zok ? __builtin_bit_cast(unsigned, o[k]) : 0u;  // beyond the cube: neutral
        }
        if constexpr (MODE == 1 || MODE == 4) {  // probe: keep the sums live, no planes
            if (offset && zok && (acc[0][0] + acc[0][1] + acc[0][2] + acc[0][3]) == -1.0f) offset[(size_t)p * 3] = o[0];
            continue;
        }
        if (cubes && zok) {
#pragma unroll
            for (int k = 0; k < JPL; ++k)
                if (JPL * q + k < J) cubes[((size_t)p * Jst + JPL * q + k) * S3 + ((size_t)x * SY + y) * SZ + zl] = o[k];
        }
        if (planes) {
#pragma unroll
            for (int k = 0; k < JPL; ++k) yzacc[k] = max(yzacc[k], ou[k]);
            // this wave's z-range maxima (all lanes: their slot's), four independent
            // VALU chains; lane L < JPL LPV then holds joint JPL (L % LPV) + L / LPV
            unsigned zm[JPL];
#pragma unroll
            for (int k = 0; k < JPL; ++k) zm[k] = slot_umax<LPV>(ou[k]);
            const int kk = lane / LPV;  // q == lane % LPV
            unsigned mv;
            if constexpr (JPL == 4) {
                mv = kk == 0 ? zm[0] : kk == 1 ? zm[1] : kk == 2 ? zm[2] : zm[3];
            } else {
                mv = zm[JPL - 1];
#pragma unroll
                for (int k = JPL - 2; k >= 0; --k) mv = kk == k ? zm[k] : mv;
            }
            if (defer) {
                if (lane < JP) lxy[(wave * 64 + x) * JP + JPL * q + kk] = mv;
            } else if (MODE != 6 && lane < JP && JPL * q + kk < J && mv != 0u) {
                // into the pre-zeroed plane (+0 cannot raise it)
                atomicMax(reinterpret_cast<unsigned *>(xy_pl) + ((size_t)(JPL * q + kk) * SX + x) * SY + y, mv);
            }
            if (zok) {
#pragma unroll
                for (int k = 0; k < JPL; ++k) {
                    // +0 cannot raise the pre-zeroed plane: skip those atomics (most of the 64^3 cube)
                    const unsigned u = ou[k];
                    if (MODE == 8 && JPL * q + k < J && u != 0u)  // probe: plain stores instead (wrong maxima)
                        reinterpret_cast<unsigned *>(xz_pl)[((size_t)(JPL * q + k) * SX + x) * SZ + zl] = u;
                    else if (MODE != 5 && MODE != 8 && (MODE != 7 || (zl & 1) == 0) && JPL * q + k < J && u != 0u)
                        atomicMax(reinterpret_cast<unsigned *>(xz_pl) + ((size_t)(JPL * q + k) * SX + x) * SZ + zl, u);
                }
            }
        }
    }
    if (planes && zok) {
#pragma unroll
        for (int k = 0; k < JPL; ++k) {
            if (JPL * q + k >= J) continue;
            float *dst = yz_pl + ((size_t)(JPL * q + k) * SY + y) * SZ + zl;
            const unsigned u = yzacc[k];
            if (xsplit == 1) *dst = __builtin_bit_cast(float, u);
            else if (u != 0u) atomicMax(reinterpret_cast<unsigned *>(dst), u);  // pre-zeroed plane
        }
    }
    if (defer) {  // xy[j][x][y] = max over the block's waves (z ranges); the plane is pre-zeroed
        __syncthreads();
        // (only the walked x range and values above +0: a row's cells are SY floats
        // apart, and storing the zeros as well -- instead of the memset -- measured
        // slower: 5.45 -> 5.73 us per proposal)
        const int n = (x_hi - x_lo) * J;
        for (int e = threadIdx.x; e < n; e += 64 * LPV) {
            const int xi = x_lo + e / J, j = e - (e / J) * J;
            unsigned m = 0u;
#pragma unroll
            for (int wv = 0; wv < LPV; ++wv) m = max(m, lxy[(wv * 64 + xi) * JP + j]);
            if (MODE != 6 && m != 0u) xy_pl[((size_t)j * SX + xi) * SY + y] = __builtin_bit_cast(float, m);
        }
    }
}

template <int LPV, bool OTF, bool CASC, int MODE = 0>
__global__ __launch_bounds__(64 * LPV) void person_cl_kernel(const float *__restrict__ cl,
                                                             const float *__restrict__ fgrid, CoordSource src,
                                                             const float *__restrict__ props,
                                                             const int32_t *__restrict__ frame_of, fvp_person_spec s,
                                                             float *__restrict__ cubes, float *__restrict__ planes,
                                                             float *__restrict__ offset, int P, int V, int J, int Jst,
                                                             int H, int W, int xmap, int xsplit, int zsplit,
                                                             unsigned pix_bytes, int xy_direct) {
    person_cl_body<LPV, OTF, CASC, MODE, 4>(cl, fgrid, src, props, frame_of, s, cubes, planes, offset, P, V, J, Jst, H,
                                            W, xmap, xsplit, zsplit, pix_bytes, xy_direct);
}

// The same on fp16 channels-last pixels read in place (cached fine grid): 8 joints
// per lane, blocks of 64 z x LPV threads with LPV = 1 / 2 / 4 for J <= 8 / 16 / 32.
template <int LPV, bool CASC>
__global__ __launch_bounds__(64 * LPV) void person_cl_h8_kernel(const float *__restrict__ cl,
                                                                const float *__restrict__ fgrid, CoordSource src,
                                                                const float *__restrict__ props,
                                                                const int32_t *__restrict__ frame_of,
                                                                fvp_person_spec s, float *__restrict__ cubes,
                                                                float *__restrict__ planes, float *__restrict__ offset,
                                                                int P, int V, int J, int Jst, int H, int W, int xmap,
                                                                int xsplit, int zsplit, unsigned pix_bytes,
                                                                int xy_direct) {
    person_cl_body<LPV, false, CASC, 0, 8>(cl, fgrid, src, props, frame_of, s, cubes, planes, offset, P, V, J, Jst, H,
                                           W, xmap, xsplit, zsplit, pix_bytes, xy_direct);
}

// Small launches (per-frame calls) split each row's x walk over 2-4 blocks.
static int person_xsplit(int P, int SY) {
    const long long rows = (long long)P * SY;
    return rows >= 4096 ? 1 : rows >= 1024 ? 2 : 4;
}

// heatmaps: planar [B][V][J][H][W] (cp == 0: re-laid out into the workspace
// first) or channels-last [B][V][H][W][cp] (read in place, no workspace).
// More than kPersonSlice joints run in joint slices (layout + launch each).
constexpr int kPersonSlice = 32;

// Every host decision of a per-person call: what person_planes_any launches and
// what fvp_person_plan reports (one PersonLaunch per joint slice, in launch order).
struct PersonLaunch {
    int j0, Jc;          // the slice's first joint and joint count
    int lpv;             // lanes per voxel (the kernel's LPV; 64 * lpv threads per block)
    unsigned pix_bytes;  // bytes of one channels-last pixel as the kernel reads it
};
struct PersonPlan {
    int jpl;             // joints per lane: 4 (fp32 pixels), 8 (fp16 pixels)
    int otf, casc;       // coordinates projected on the fly; 16-camera cascade (V > 16)
    int xsplit, zsplit;  // blocks per row along x; 64-deep z chunks
    int xy_direct;       // xy maxima from LDS as plain stores (otherwise atomicMax)
    int layout;          // a layout pass per slice (planar input)
    int zeroed_planes;   // planes pre-zeroed by the call: 0 (no planes), 2 or 3 (x split: yz too)
    unsigned blocks;     // grid of every launch
    int n;               // launches
    PersonLaunch s[(FVP_MAX_JOINTS + kPersonSlice - 1) / kPersonSlice];
};

// The checks an entry point makes on its own arguments before the common ones.
static int person_entry_check(bool cl, bool cl_half, int cp, int J, bool hm_aligned) {
    if (cl_half) return (cp <= 0 || cp % 8 || cp < J || J > FVP_MAX_JOINTS || !hm_aligned) ? FVP_ERR_SHAPE : FVP_OK;
    if (cl) return cp <= 0 ? FVP_ERR_SHAPE : FVP_OK;
    return FVP_OK;
}

// The argument checks (all but the null-pointer and workspace checks) and the
// launch decisions of person_planes_any.  P <= 0 is FVP_OK with no launch.
static int person_plan(bool otf, int cp, bool cl_half, bool hm_aligned, int B, int V, int J, int H, int W,
                       const int32_t *bins, const int32_t *fine, int P, bool planes, PersonPlan &pl) {
    pl = PersonPlan{};
    if (P <= 0) return FVP_OK;
    if (B <= 0 || V <= 0 || V > FVP_MAX_VIEWS || J <= 0 || J > FVP_MAX_JOINTS || H < 2 || W < 2) return FVP_ERR_SHAPE;
    if (otf && V > 64) return FVP_ERR_SHAPE;  // camera records staged in LDS
    const int SX = bins[0], SY = bins[1], SZ = bins[2];
    if (SX <= 0 || SY <= 0 || SZ <= 0 || SX > 4096 || SY > 4096 || SZ > 4096 || fine[0] <= 1 || fine[1] <= 1 ||
        fine[2] <= 1)
        return FVP_ERR_SHAPE;
    if (planes && !(SX == SY && SY == SZ)) return FVP_ERR_SHAPE;  // torch.cat of the planes needs a cubic volume
    // packed fine grid addressed with 32-bit byte offsets
    if (!otf && (long long)fine[0] * fine[1] * fine[2] * FVP_GRID_SLOTS(V) * 8 > 0xfffff000LL) return FVP_ERR_SHAPE;
    if (cl_half) {  // fp16 pixels, cp in fp16 elements (as fvp_voxelize_cl_f16); cached fine grid only
        if (otf || cp <= 0 || cp % 8 || cp < J || !hm_aligned || (unsigned long long)H * W * cp * 2 > 0x7fffffffull)
            return FVP_ERR_SHAPE;
    } else if (cp) {
        const int jl = ((J - 1) / kPersonSlice) * kPersonSlice;
        if (cp % 4 || cp < jl + 4 * lanes_per_voxel(J - jl) || (size_t)H * W * cp * 4 > 0x7fffffffull)
            return FVP_ERR_SHAPE;
    }
    pl.jpl = cl_half ? 8 : 4;
    pl.otf = otf ? 1 : 0;
    pl.casc = V > 16 ? 1 : 0;
    pl.xsplit = person_xsplit(P, SY);
    pl.zsplit = (SZ + 63) / 64;
    // xy maxima stored by their row's block without atomics (person_cl_kernel
    // xy_direct): one x part, one z chunk, S <= 64 and every joint slice at <= 4
    // lanes per voxel
    pl.xy_direct = (planes && pl.xsplit == 1 && SZ <= 64 && SX <= 64 && (J <= 16 || cl_half)) ? 1 : 0;
    pl.layout = (!cl_half && !cp) ? 1 : 0;
    // xy, xz (and yz when x is split) hold maxima over non-negative floats: from +0
    pl.zeroed_planes = planes ? (pl.xsplit > 1 ? 3 : 2) : 0;
    pl.blocks = (unsigned)((long long)P * SY * pl.xsplit * pl.zsplit);
    for (int j0 = 0; j0 < J; j0 += kPersonSlice) {
        PersonLaunch &l = pl.s[pl.n++];
        l.j0 = j0;
        l.Jc = J - j0 < kPersonSlice ? J - j0 : kPersonSlice;
        l.lpv = cl_half ? lanes_per_voxel_h(l.Jc) : lanes_per_voxel(l.Jc);
        l.pix_bytes = cl_half ? 2u * (unsigned)cp : 4u * (unsigned)(cp ? cp : 4 * l.lpv);
    }
    return FVP_OK;
}

template <int LPV, bool OTF, bool CASC, int JPL = 4>
static void launch_person_cl(const float *cl, const CoordSource &src, const float *props,
                             const int32_t *frame_of, const fvp_person_spec &s, float *cubes, float *planes,
                             float *offset, int P, int V, int J, int Jst, int H, int W, unsigned pix_bytes,
                             const PersonPlan &pl, hipStream_t st) {
    // one y-row per block: with the planes-only fast path for x-planes outside the
    // window, rows are the finer and better balanced unit -- measured (C3, 320
    // proposals): 1 row 6.24, 2 rows 6.85, 4 rows 7.4, 8 rows 8.8 us per proposal
    // (round 2); two rows per block again in round 4 (sequential: 6.04 vs 5.86; two
    // halves combining xz in LDS: 5.98 vs 5.45).  XCD-aware placement keeps a
    // proposal's rows on one XCD.  Small launches (per-frame calls) split each row's
    // x walk over 2-4 blocks (the yz maxima then go through atomics into a
    // pre-zeroed plane).  Cubes deeper than 64 run as 64-deep z chunks, one block
    // each (the xy and xz maxima combine across blocks through atomics; yz is per
    // (y, z)).
    const int xmap = 1, xsplit = pl.xsplit, zsplit = pl.zsplit, xy_direct = pl.xy_direct;
    const dim3 grid(pl.blocks);
    if constexpr (JPL == 8)
        hipLaunchKernelGGL((person_cl_h8_kernel<LPV, CASC>), grid, dim3(64 * LPV), 0, st, cl, src.grids, src, props,
                           frame_of, s, cubes, planes, offset, P, V, J, Jst, H, W, xmap, xsplit, zsplit, pix_bytes,
                           xy_direct);
    else
        hipLaunchKernelGGL((person_cl_kernel<LPV, OTF, CASC>), grid, dim3(64 * LPV), 0, st, cl, src.grids, src, props,
                           frame_of, s, cubes, planes, offset, P, V, J, Jst, H, W, xmap, xsplit, zsplit, pix_bytes,
                           xy_direct);
}

}  // namespace fvp

extern "C" int fvp_max_planes(const float *cubes, int P, int J, int S, float *planes, void *stream) {
    if (!cubes || !planes) return FVP_ERR_NULL;
    if (P <= 0) return FVP_OK;
    if (J <= 0 || S <= 0 || S > 4096) return FVP_ERR_SHAPE;
    if (S > 64) {
        const size_t n = (size_t)3 * P * J * S * S;
        hipLaunchKernelGGL(fvp::max_planes_generic_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                           (hipStream_t)stream, cubes, planes, P, J, S);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(fvp::max_planes_kernel, dim3(P * J), dim3(256), 0, (hipStream_t)stream, cubes, planes, P, J,
                       S);
    return (int)hipGetLastError();
}

extern "C" size_t fvp_person_workspace_bytes(int B, int V, int J, int H, int W) {
    if (B <= 0 || V <= 0 || J <= 0 || J > FVP_MAX_JOINTS || H <= 0 || W <= 0) return 0;
    return (size_t)B * fvp::cl_frame_bytes(V, J < 32 ? J : 32, H, W);  // one joint slice at a time
}

namespace fvp {

// +0.0 into the n floats of the planes a launch accumulates into: a grid-stride loop, one float
// per lane and step (consecutive lanes store consecutive floats; 4-byte alignment is all that is
// assumed of the planes).
__global__ __launch_bounds__(256) void zero_planes_kernel(float *__restrict__ p, size_t n) {
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) p[i] = 0.0f;
}

static int person_planes_any(const float *heatmaps, int cp, int B, int V, int J, int H, int W, const CoordSource &src,
                             const fvp_person_spec *spec, const float *proposals, const int32_t *frame_of, int P,
                             float *cubes, float *planes, float *offset, void *workspace, size_t workspace_bytes,
                             void *stream, bool cl_half = false) {
    if (!heatmaps || !spec || (!src.grids && !src.cams)) return FVP_ERR_NULL;
    if (P <= 0) return FVP_OK;
    if (!proposals) return FVP_ERR_NULL;
    PersonPlan pl;
    const int sc = person_plan(src.cams != nullptr, cp, cl_half, ((unsigned long long)heatmaps & 15ull) == 0, B, V, J,
                               H, W, spec->bins, spec->fine, P, planes != nullptr, pl);
    if (sc != FVP_OK) return sc;
    if (pl.layout) {
        const size_t need = (size_t)B * cl_frame_bytes(V, pl.s[0].Jc, H, W);
        if (!workspace || workspace_bytes < need) return FVP_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int SX = spec->bins[0], SY = spec->bins[1], SZ = spec->bins[2];
    if (pl.zeroed_planes) {
        const size_t n = pl.zeroed_planes * (size_t)P * J * SX * SY;
        // A workaround, under a stream capture only: the zeroing goes in as a kernel node like its
        // neighbours.  As a memset node, replays of a captured JLN after the first did not
        // reproduce the eager planes; why the runtime's memset node does that is supposed, not
        // established.  Eager launches keep the memset and pay one capture query.
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cap) != hipSuccess) {
            (void)hipGetLastError();
            cap = hipStreamCaptureStatusNone;
        }
        if (cap == hipStreamCaptureStatusActive) {
            const size_t want = (n + 4 * 256 - 1) / (4 * 256);  // ~4 floats per lane, at most 4,096 blocks
            const size_t blocks = want < 4096 ? want : 4096;
            hipLaunchKernelGGL(zero_planes_kernel, dim3((unsigned)blocks), dim3(256), 0, st, planes, n);
        } else {
            const hipError_t e = hipMemsetAsync(planes, 0, n * 4, st);
            if (e != hipSuccess) return (int)e;
        }
    }
    const size_t HW = (size_t)H * W, S2 = (size_t)SX * SY, S3 = S2 * SZ;
    using TT = std::true_type;
    using FF = std::false_type;
    for (int k = 0; k < pl.n; ++k) {
        const int j0 = pl.s[k].j0, Jc = pl.s[k].Jc;
        float *cb = cubes ? cubes + j0 * S3 : nullptr;
        float *pp = planes ? planes + j0 * S2 : nullptr;
        // the slice's pixels: fp16 / fp32 channels-last in place from channel j0 on, or the workspace
        const float *cl = cl_half ? reinterpret_cast<const float *>(reinterpret_cast<const _Float16 *>(heatmaps) + j0)
                          : cp    ? heatmaps + j0
                                  : reinterpret_cast<const float *>(workspace);
        auto go = [&](auto lpv, auto otf, auto casc, auto jpl) {
            constexpr int L = decltype(lpv)::value, JPL = decltype(jpl)::value;
            if constexpr (JPL == 4)
                if (pl.layout)
                    launch_layout<L, float>(heatmaps + j0 * HW, B, V, Jc, J, H, W,
                                            reinterpret_cast<float *>(workspace), st);
            launch_person_cl<L, decltype(otf)::value, decltype(casc)::value, JPL>(
                cl, src, proposals, frame_of, *spec, cb, pp, offset, P, V, Jc, J, H, W, pl.s[k].pix_bytes, pl, st);
        };
        auto flags = [&](auto lpv, auto jpl) {  // (fp16 pixels: cached fine grid only, person_plan)
            if constexpr (decltype(jpl)::value == 4)
                if (pl.otf) return pl.casc ? go(lpv, TT{}, TT{}, jpl) : go(lpv, TT{}, FF{}, jpl);
            return pl.casc ? go(lpv, FF{}, TT{}, jpl) : go(lpv, FF{}, FF{}, jpl);
        };
        auto lanes = [&](auto jpl) {  // (8 lanes per voxel: fp32 pixels only, lanes_per_voxel_h)
            const int lpv = pl.s[k].lpv;
            if (lpv == 1) return flags(std::integral_constant<int, 1>{}, jpl);
            if (lpv == 2) return flags(std::integral_constant<int, 2>{}, jpl);
            if constexpr (decltype(jpl)::value == 4)
                if (lpv == 8) return flags(std::integral_constant<int, 8>{}, jpl);
            return flags(std::integral_constant<int, 4>{}, jpl);
        };
        cl_half ? lanes(std::integral_constant<int, 8>{}) : lanes(std::integral_constant<int, 4>{});
    }
    return (int)hipGetLastError();
}

}  // namespace fvp

// What person_planes_any would do for these arguments (person_plan, the function
// the launcher itself calls): no device pointer, no HIP call.  (The struct checks of
// fvp_person_planes_cams -- image size, fine bins -- are not among its inputs.)
extern "C" int fvp_person_plan(int kind, int cp, int B, int V, int J, int H, int W, int SX, int SY, int SZ, int FX,
                               int FY, int FZ, int P, int want_cubes, int want_planes, int hm_aligned, long long *plan,
                               int cap, int *count) {
    if (!count || (cap > 0 && !plan)) return FVP_ERR_NULL;
    *count = 0;
    if (kind < 0 || kind > 3 || cap < 0) return FVP_ERR_SHAPE;
    (void)want_cubes;  // the cubes change nothing on the host (planes-only blocks walk less: a kernel decision)
    const bool cl = kind == 2, cl_half = kind == 3;
    int st = fvp::person_entry_check(cl, cl_half, cp, J, hm_aligned != 0);
    if (st != FVP_OK) return st;
    const int32_t bins[3] = {SX, SY, SZ}, fine[3] = {FX, FY, FZ};
    fvp::PersonPlan pl;
    st = fvp::person_plan(kind == 1, (cl || cl_half) ? cp : 0, cl_half, hm_aligned != 0, B, V, J, H, W, bins, fine, P,
                          want_planes != 0, pl);
    if (st != FVP_OK) return st;
    for (int k = 0; k < pl.n; ++k) {
        if (k < cap) {
            const fvp::PersonLaunch &l = pl.s[k];
            const long long r[FVP_PERSON_PLAN_FIELDS] = {l.j0, l.Jc, l.lpv, pl.jpl, pl.otf, pl.casc, pl.xsplit,
                                                         pl.zsplit, pl.xy_direct, pl.blocks, 64 * l.lpv, l.pix_bytes,
                                                         pl.layout, pl.zeroed_planes};
            for (int f = 0; f < FVP_PERSON_PLAN_FIELDS; ++f) plan[(size_t)k * FVP_PERSON_PLAN_FIELDS + f] = r[f];
        }
    }
    *count = pl.n;
    return FVP_OK;
}

extern "C" int fvp_person_planes(const float *heatmaps, int B, int V, int J, int H, int W, const float *fine_grid,
                                 const fvp_person_spec *spec, const float *proposals, const int32_t *frame_of, int P,
                                 float *cubes, float *planes, float *offset, void *workspace, size_t workspace_bytes,
                                 void *stream) {
    if (!fine_grid) return FVP_ERR_NULL;
    return fvp::person_planes_any(heatmaps, 0, B, V, J, H, W, fvp::CoordSource{fine_grid}, spec, proposals, frame_of, P,
                                  cubes, planes, offset, workspace, workspace_bytes, stream);
}

extern "C" int fvp_person_planes_cams(const float *heatmaps, int B, int V, int J, int H, int W, const float *cams,
                                      const float *resize_t, const fvp_grid_spec *fine_grid_spec,
                                      const fvp_image_spec *img, const fvp_person_spec *spec, const float *proposals,
                                      const int32_t *frame_of, int P, float *cubes, float *planes, float *offset,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    if (!cams || !resize_t || !fine_grid_spec || !img) return FVP_ERR_NULL;
    if (img->hm_w != W || img->hm_h != H) return FVP_ERR_SHAPE;
    for (int a = 0; a < 3; ++a)
        if (fine_grid_spec->bins[a] != spec->fine[a]) return FVP_ERR_SHAPE;
    const fvp::CoordSource src{nullptr, cams, resize_t, *fine_grid_spec, fvp::image_consts(*img), 0};
    return fvp::person_planes_any(heatmaps, 0, B, V, J, H, W, src, spec, proposals, frame_of, P, cubes, planes, offset,
                                  workspace, workspace_bytes, stream);
}

extern "C" int fvp_person_planes_cl(const float *heatmaps_cl, int cp, int B, int V, int J, int H, int W,
                                    const float *fine_grid, const fvp_person_spec *spec, const float *proposals,
                                    const int32_t *frame_of, int P, float *cubes, float *planes, float *offset,
                                    void *stream) {
    if (!fine_grid) return FVP_ERR_NULL;
    if (const int sc = fvp::person_entry_check(true, false, cp, J, true)) return sc;
    return fvp::person_planes_any(heatmaps_cl, cp, B, V, J, H, W, fvp::CoordSource{fine_grid}, spec, proposals,
                                  frame_of, P, cubes, planes, offset, nullptr, 0, stream);
}

extern "C" int fvp_person_planes_cl_f16(const void *heatmaps_cl, int cp, int B, int V, int J, int H, int W,
                                        const float *fine_grid, const fvp_person_spec *spec, const float *proposals,
                                        const int32_t *frame_of, int P, float *cubes, float *planes, float *offset,
                                        void *stream) {
    if (!heatmaps_cl || !fine_grid || !spec) return FVP_ERR_NULL;
    if (const int sc = fvp::person_entry_check(false, true, cp, J, ((unsigned long long)heatmaps_cl & 15ull) == 0))
        return sc;
    return fvp::person_planes_any(reinterpret_cast<const float *>(heatmaps_cl), cp, B, V, J, H, W,
                                  fvp::CoordSource{fine_grid}, spec, proposals, frame_of, P, cubes, planes, offset,
                                  nullptr, 0, stream, true);
}
