// mfx_xform_dev.h -- device pieces shared by the two splice + affine kernels, k_splice_affine (mfx_xform.hip: one tile of
// consecutive rows of one utterance per block) and k_sess_xform (mfx_sess_xform.hip: row groups of several sessions per
// block).  See DESIGN.md, "Splice + affine transform" and "Session transform".
//   xform_tiles / xform_steps / xform_ksteps   the operand geometry (host and device)
//   xform_tm                                   accumulator tiles a wave carries, rounded up to an instantiated count
//   xform_prefetch0 / xform_commit0            chunk 0 of the operands: global -> registers, registers -> LDS buffer 0
//   xform_bias                                 the accumulators' start: b
//   xform_chain                                the chunk loop: chunk c + 1 through registers while chunk c is consumed, the
//                                              ascending FMA chain of every accumulator (matrix pipe or vector ALUs)
//   xform_scatter                              accumulators -> the rows of one group of 16 in LDS, as they lie in memory
//   xform_compute                              the three above in turn, with the accumulators its own: what the kernels call
// Both kernels give a wave one row group of 16 rows (`za`: where the wave reads its group's spliced rows in LDS) and the output
// tiles slot + j slots, j < cnt; everything here is the same for them, so they deliver the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "mfx_dev.h"

namespace mfx {
namespace {

__host__ __device__ inline int xform_tiles(int out_dim) { return (out_dim + 15) >> 4; }
__host__ __device__ inline int xform_steps(int in_dim) { return (in_dim + 3) >> 2; }
// steps of 4 taps per LDS chunk: at most 2048 floats (8 KB, two 16-byte words per thread in flight) per buffer -- the
// two buffers leave room for 64 rows of the C2 shape (39 columns, 9 frames, 40 outputs) inside the LDS target
__host__ __device__ inline int xform_ksteps(int in_dim, int out_dim)
{
    const int k = 32 / xform_tiles(out_dim), s = xform_steps(in_dim);
    return k < s ? k : s;
}

// accumulator tiles a wave carries at tile_rows rows (tile_rows / 16 row groups) per block, rounded up to an instantiated count
inline int xform_tm(int out_dim, int tile_rows)
{
    const int slots = 4 / (tile_rows >> 4);
    const int t = (xform_tiles(out_dim) + slots - 1) / slots;
    return t <= 4 ? t : t <= 8 ? 8 : 16;
}

// the wave's share of a block: row group g, tiles slot + j slots for j < cnt (G = row groups of the block, 4, 2 or 1)
struct XformWave {
    int g, slot, slots, cnt;
};
template <int TM>
__device__ __forceinline__ XformWave xform_wave(int wave, int G, int NT)
{
    XformWave w;
    w.slots = 4 / G; // waves that share a group split the tiles
    w.g = wave & (G - 1);
    w.slot = wave / G;
    w.cnt = w.slot < NT ? min(TM, (NT - w.slot + w.slots - 1) / w.slots) : 0;
    return w;
}

// chunk 0 on its way (the caller stages its rows meanwhile), then into buffer 0
__device__ __forceinline__ void xform_prefetch0(const f32x4 *ops4, f32x4 (&pf)[2], int chunk4, int total4, int tid)
{
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int i = tid + 256 * q;
        if (i < min(chunk4, total4)) pf[q] = ops4[i];
    }
}
__device__ __forceinline__ void xform_commit0(float *s_b, const f32x4 (&pf)[2], int chunk4, int total4, int tid)
{
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int i = tid + 256 * q;
        if (i < min(chunk4, total4)) ((f32x4 *)s_b)[i] = pf[q];
    }
}

template <int TM>
__device__ __forceinline__ void xform_bias(const float *bias, const XformWave w, int li, f32x4 (&acc)[TM])
{
#pragma unroll
    for (int j = 0; j < TM; ++j) {
        const float b = j < w.cnt ? bias[16 * (w.slot + j * w.slots) + li] : 0.f;
        acc[j] = f32x4{b, b, b, b};
    }
}

// The chunk loop.  s_b: the two operand buffers (chunk 0 committed, a barrier behind it); za: the wave's rows in LDS -- matrix
// form: lane (li, lk) feeds row li of the group, tap 4 s + lk (za = rows + li Wd + lk); vector form: rows 4 lk + r, taps in
// turn (za = rows + 4 lk Wd).  Every thread of the block calls it (the barriers), busy or not.
template <bool VALU, int TM>
__device__ __forceinline__ void xform_chain(const f32x4 *ops4, f32x4 (&pf)[2], float *s_b, int chunk4, int total4, int nchunks, int steps,
                                            int KS, int NT, int in_dim, int Wd, const float *za, bool busy, const XformWave w, int tid,
                                            f32x4 (&acc)[TM])
{
    const int lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int slot = w.slot, slots = w.slots, cnt = w.cnt;
    for (int c = 0; c < nchunks; ++c) {
        const bool more = c + 1 < nchunks;
        const int n4 = more ? min(chunk4, total4 - (c + 1) * chunk4) : 0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int i = tid + 256 * q;
            if (i < n4) pf[q] = ops4[(c + 1) * chunk4 + i];
        }
        if (busy) {
            const float *buf = s_b + (c & 1) * chunk4 * 4 + slot * 64;
            const int s0 = c * KS, s1 = min(steps, s0 + KS);
            for (int s = s0; s < s1; ++s) {
                const float *b = buf + (s - s0) * NT * 64;
                if constexpr (VALU) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int i = 4 * s + k;
                        float z[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) z[r] = i < in_dim ? za[r * Wd + i] : 0.f;
#pragma unroll
                        for (int j = 0; j < TM; ++j) {
                            if (j < cnt) {
                                const float wt = b[j * slots * 64 + 16 * k + li];
#pragma unroll
                                for (int r = 0; r < 4; ++r) acc[j][r] = __builtin_fmaf(wt, z[r], acc[j][r]);
                            }
                        }
                    }
                } else {
                    const float a = 4 * s + lk < in_dim ? za[4 * s] : 0.f;
#pragma unroll
                    for (int j = 0; j < TM; ++j)
                        if (j < cnt) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[j * slots * 64 + lane], acc[j], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int i = tid + 256 * q;
            if (i < n4) ((f32x4 *)(s_b + ((c + 1) & 1) * chunk4 * 4))[i] = pf[q];
        }
        __syncthreads();
    }
}

// D[i][n]: lane holds rows i = 4 (lane >> 4) + r, output n = lane & 15, of its group's 16 rows.  s_grp: the group's rows in
// the output tile [.][od]; rows: how many of the 16 exist.
template <int TM>
__device__ __forceinline__ void xform_scatter(float *s_grp, int od, int rows, const XformWave w, int li, int lk, const f32x4 (&acc)[TM])
{
#pragma unroll
    for (int j = 0; j < TM; ++j) {
        const int o = 16 * (w.slot + j * w.slots) + li;
        if (j >= w.cnt || o >= od) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = 4 * lk + r;
            if (t < rows) s_grp[t * od + o] = acc[j][r];
        }
    }
}

// The wave's whole share of a block, with the accumulators its own: b, the chunk loop, the scatter into the group's rows of
// the output tile (s_grp, `rows` of them exist), and the barrier behind which the tile is complete.
template <bool VALU, int TM>
__device__ __forceinline__ void xform_compute(const f32x4 *ops4, const float *bias, f32x4 (&pf)[2], float *s_b, int chunk4, int total4,
                                              int nchunks, int steps, int KS, int NT, int in_dim, int Wd, const float *za, bool busy,
                                              const XformWave w, int tid, float *s_grp, int od, int rows)
{
    const int lane = tid & 63, li = lane & 15, lk = lane >> 4;
    f32x4 acc[TM];
    xform_bias<TM>(bias, w, li, acc);
    xform_chain<VALU, TM>(ops4, pf, s_b, chunk4, total4, nchunks, steps, KS, NT, in_dim, Wd, za, busy, w, tid, acc);
    if (busy) xform_scatter<TM>(s_grp, od, rows, w, li, lk, acc);
    __syncthreads();
}

} // namespace
} // namespace mfx
