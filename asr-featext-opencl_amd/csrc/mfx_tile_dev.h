// mfx_tile_dev.h -- device pieces shared by the kernels behind the front ends (mfx_tail / mfx_plp / mfx_traps / mfx_xform):
//   div_small, div_magic   floor(i / d) of a tile index as a multiply-high
//   tile_store_rows        a finished tile from LDS to its output rows, 16-byte words where the layout allows
//   delta_tile             the delta stage of one tile, typed for float (k_delta) or float4 (k_delta4) elements
//   PlainGroups            the row groups of [0, n_rows): the plain counterpart of RunGroups (mfx_dev.h)
#pragma once
#include <hip/hip_runtime.h>

#include "mfx_delta_dev.h"
#include "mfx_dev.h"
#include "mfx_kernels.h"

namespace mfx {
namespace {

// floor(i / d) for i < 2^16 as a multiply-high; magic = div_magic(d) = 0xffffffff / d + 1, which wraps to 0 at d = 1: a
// one-column configuration (ceps_len 1 without c0, one filter without a DCT) takes i itself.  div_small2: the
// caller knows d >= 2.
__device__ __forceinline__ uint32_t div_magic(int d) { return 0xffffffffu / (uint32_t)d + 1; }
__device__ __forceinline__ int div_small2(int i, uint32_t magic) { return (int)__umulhi((uint32_t)i, magic); }
__device__ __forceinline__ int div_small(int i, int d, uint32_t magic) { return d == 1 ? i : div_small2(i, magic); }

// The tile s_out [rows][cols], assembled in LDS as it lies in memory, to rows row0 .. row0 + rows - 1 of `out` at `pitch`
// floats: consecutive threads on consecutive words, 16-byte words where the row width, the pitch and the pointer allow,
// floats otherwise.  256 threads.
__device__ __forceinline__ void tile_store_rows(const float *s_out, int cols, int rows, float *out, int64_t row0, int pitch, int tid)
{
    float *obase = out + row0 * pitch;
    if ((cols & 3) == 0 && (pitch & 3) == 0 && ((uintptr_t)out & 15) == 0) {
        const int c4 = cols >> 2;
        const uint32_t magic = div_magic(c4);
        const int n = rows * c4;
        for (int i = tid; i < n; i += 256) {
            const int rr = div_small(i, c4, magic);
            const int q = i - rr * c4;
            *(float4 *)(obase + rr * (int64_t)pitch + 4 * q) = *(const float4 *)(s_out + rr * cols + 4 * q);
        }
    } else {
        const uint32_t magic = div_magic(cols);
        const int n = rows * cols;
        for (int i = tid; i < n; i += 256) {
            const int rr = div_small(i, cols, magic);
            const int c = i - rr * cols;
            obase[rr * (int64_t)pitch + c] = s_out[i];
        }
    }
}

// ---- the delta tile: element helpers for float and float4 (the same arithmetic per component: delta_quot)
__device__ __forceinline__ float delta_fma_diff(float l, float a, float b, float num) { return __builtin_fmaf(l, a - b, num); }
__device__ __forceinline__ float4 delta_fma_diff(float l, float4 a, float4 b, float4 num)
{
    return make_float4(__builtin_fmaf(l, a.x - b.x, num.x), __builtin_fmaf(l, a.y - b.y, num.y), __builtin_fmaf(l, a.z - b.z, num.z),
                       __builtin_fmaf(l, a.w - b.w, num.w));
}
__device__ __forceinline__ float delta_quot_e(float num, float d, float inv) { return delta_quot(num, d, inv); }
__device__ __forceinline__ float4 delta_quot_e(float4 num, float d, float inv)
{
    return make_float4(delta_quot(num.x, d, inv), delta_quot(num.y, d, inv), delta_quot(num.z, d, inv), delta_quot(num.w, d, inv));
}
// regression of order L around element i of rows of cw elements: ascending-l FMA chain, then the quotient
template <class E>
__device__ __forceinline__ E delta_regress(const E *s, int i, int L, int cw, float d, float inv)
{
    E num{};
    for (int l = 1; l <= L; ++l) num = delta_fma_diff((float)l, s[i + (L + l) * cw], s[i + (L - l) * cw], num);
    return delta_quot_e(num, d, inv);
}
__device__ __forceinline__ void delta_denominator(int L, float &d, float &inv)
{
    float den = 0.f;
    for (int l = 1; l <= L; ++l) den += (float)(l * l);
    d = 2 * den;
    inv = 1.0f / d;
}

// Delta stage of one tile of ROWS output rows (deltacpu.cpp:16-29; edges: the clamped row accessor of Segment).  E = float:
// any shape; FAST16 (cols <= 16): a row is 16 consecutive work items -- no integer division by a run-time column count,
// 13..16 consecutive floats per row piece -- otherwise the generic index split.  E = float4: a work item is 4 consecutive
// columns, every load / LDS access / store a 16-byte word; requires cols % 4 == 0, l1 > 0, src_pitch % 4 == 0, out_pitch ==
// cols * groups and 16-byte aligned src / out.  LDS: s_pad [ROWS + 2 D][cw] | s_d [ROWS + 2 l2][cw] | s_dd [ROWS][cw].
template <class E, bool FAST16, int ROWS>
__device__ __forceinline__ void delta_tile(const DeltaParams &p, E *smem)
{
    constexpr bool VEC = sizeof(E) == sizeof(float4);
    static_assert(!(VEC && FAST16), "16-column rows are float rows");
    const Segment sg = p.inline_seg ? p.seg0 : p.segs[blockIdx.y];
    const int r0 = blockIdx.x * ROWS;
    if (r0 >= sg.n_out) return;
    const int rows = min(ROWS, sg.n_out - r0);
    const int l1 = p.l1, l2 = p.l2, D = l1 + l2;
    const int cols = VEC ? p.cols >> 2 : p.cols; // in elements
    const int cw = FAST16 ? 16 : cols;           // row width in work items and in LDS
    const int tid = threadIdx.x;
    E *s_pad = smem;
    E *s_d = s_pad + (ROWS + 2 * D) * cw;
    E *s_dd = s_d + (ROWS + 2 * l2) * cw;
    const uint32_t magic_c = div_magic(cols > 0 ? cols : 1);
    auto split = [&](int i, int &rr, int &c) {
        if (FAST16) {
            rr = i >> 4;
            c = i & 15;
        } else {
            rr = div_small2(i, magic_c); // (not FAST16: more than 16 columns, at least 5 words of 4)
            c = i - rr * cols;
        }
    };

    if (VEC || l1 > 0) {
        const int n_pad = (rows + 2 * D) * cw;
        for (int i = tid; i < n_pad; i += 256) {
            int rr, c;
            split(i, rr, c);
            int sr = r0 + rr + sg.shift;
            sr = max(sg.lo, min(sg.hi, sr));
            s_pad[i] = (VEC || c < cols) ? ((const E *)(p.src + (sg.src_row0 + sr) * (int64_t)p.src_pitch))[c] : E{};
        }
        __syncthreads();
        float d1, inv1;
        delta_denominator(l1, d1, inv1);
        const int n_d = (rows + 2 * l2) * cw;
        for (int i = tid; i < n_d; i += 256) s_d[i] = delta_regress(s_pad, i, l1, cw, d1, inv1);
        __syncthreads();
    }
    if (l2 > 0) {
        float d2, inv2;
        delta_denominator(l2, d2, inv2);
        const int n_dd = rows * cw;
        for (int i = tid; i < n_dd; i += 256) s_dd[i] = delta_regress(s_d, i, l2, cw, d2, inv2);
        __syncthreads();
    }
    // The tile's output rows are one contiguous block of rows * width elements: write it with consecutive threads on
    // consecutive addresses (whole cache lines), statics included.
    const int groups = l2 > 0 ? 3 : (VEC || l1 > 0) ? 2 : 1;
    const int width = VEC || p.out_pitch == cols * groups ? cols * groups : 0;
    const int stat_row = sg.static_off - sg.shift; // row of s_pad that holds the static part of output row 0
    if (VEC || (width > 0 && l1 > 0)) {
        E *obase = (E *)(p.out + (sg.out_row0 + r0) * (int64_t)p.out_pitch);
        const uint32_t magic = div_magic(width);
        const int n_o = rows * width;
        for (int i = tid; i < n_o; i += 256) {
            const int rr = div_small2(i, magic); // (two or three column groups: width >= 2)
            const int cc = i - rr * width;
            E v;
            if (cc < cols)
                v = s_pad[(rr + stat_row) * cw + cc];
            else if (cc < 2 * cols)
                v = s_d[(rr + l2) * cw + cc - cols];
            else
                v = s_dd[rr * cw + cc - 2 * cols];
            obase[i] = v;
        }
        return;
    }
    if constexpr (!VEC) { // generic fallback (row pitch wider than the feature row, or statics only): scalar stores
        const int n_o = rows * cw;
        for (int i = tid; i < n_o; i += 256) {
            int rr, c;
            split(i, rr, c);
            if (c >= cols) continue;
            float *orow = p.out + (sg.out_row0 + r0 + rr) * (int64_t)p.out_pitch;
            orow[c] = p.src[(sg.src_row0 + r0 + rr + sg.static_off) * (int64_t)p.src_pitch + c];
            if (l1 > 0) {
                orow[cols + c] = s_d[i + l2 * cw];
                if (l2 > 0) orow[2 * cols + c] = s_dd[i];
            }
        }
    }
}

// ---- wave-per-row-group kernels (k_melcep): their row groups and the staging of the mel plan
// Groups of G rows of [0, n_rows), numbered through: this wave takes the groups `first`, `first + stride`, ...; while
// valid(), rows row0 .. row0 + count - 1 (count <= G) are its current group.  (RunGroups, mfx_dev.h, is the same interface
// over a table's clipped row runs.)
template <int G>
struct PlainGroups {
    int64_t n_rows, grp, stride;
    int64_t row0 = 0;
    int count = 0;
    __device__ __forceinline__ PlainGroups(int64_t n_rows_, int64_t first, int64_t stride_) : n_rows(n_rows_), grp(first), stride(stride_) { set(); }
    __device__ __forceinline__ bool valid() const { return grp * G < n_rows; }
    __device__ __forceinline__ void advance()
    {
        grp += stride;
        set();
    }
    __device__ __forceinline__ void set()
    {
        row0 = grp * G;
        count = (int)(n_rows - row0 < G ? n_rows - row0 : G);
    }
};

} // namespace
} // namespace mfx
