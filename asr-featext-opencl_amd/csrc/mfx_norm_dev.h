// mfx_norm_dev.h -- device code the normaliser kernels share (mfx_tail.hip: k_norm_stats, k_norm_seg; mfx_speakers.hip:
// k_spk_sums, k_spk_finish): the per-column totals of a run of rows, and the statistics from such totals.  One definition, so
// that a speaker's pooled statistics are built from the very doubles an utterance's own statistics are built from.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mfx_kernels.h"

namespace mfx {

// mean and multiplier from the totals of n rows (normalizercpu.cpp:40-58); N: int, or double where n may pass 2^31
template <class N>
__device__ __forceinline__ void norm_finish_to(float *st, int cols, int norm_type, int c, N n, double S, double S2, float mn,
                                               float mx)
{
    const float mean = (float)(S / n);
    float mult = 1.f;
    if (norm_type == 2)
        mult = (float)sqrt((n - 1) / (S2 - S * (S / n)));
    else if (norm_type == 3)
        mult = 1.f / fmaxf(fabsf(mn - mean), fabsf(mx - mean));
    st[c] = mean;
    st[cols + c] = mult;
}

// columns rounded up to a power of two: 2^lg threads per row of threads, 256 >> lg rows per pass (cols <= 256)
__device__ __forceinline__ int norm_lg(int cols)
{
    int lg = 0;
    while ((1 << lg) < cols) ++lg;
    return lg;
}

// Totals of rows [r0, r1) of `cols` columns by the first 256 threads of the block: thread tid is (row class rr = tid >> lg,
// column c = tid & (2^lg - 1)); it adds its rows r0 + rr, r0 + rr + rpp, ... in ascending order, in double (the sum of
// squares takes the float32 product v * v, normalizercpu.cpp:44), and the row classes are folded through LDS by halving.
// load(r, c): the value at row r, column c.  On return (behind a barrier) thread (0, c), c < cols, finds the totals in
// s_sum[tid], s_sum2[tid], s_min[tid], s_max[tid].  Every thread of the block must call it.  WIDE: the block has more than
// 256 threads (the others only take part in the barriers).
template <bool WIDE, class Load>
__device__ __forceinline__ void norm_rows_totals(Load load, int r0, int r1, int cols, int lg, int tid, double *s_sum, double *s_sum2,
                                                 float *s_min, float *s_max)
{
    const int Cp = 1 << lg, rpp = 256 >> lg;
    const int rr = tid >> lg, c = tid & (Cp - 1);
    double sum = 0, sum2 = 0;
    float mn = 3.402823466e+38f, mx = -3.402823466e+38f;
    if (c < cols && (!WIDE || tid < 256))
        for (int r = r0 + rr; r < r1; r += rpp) {
            const float v = load(r, c);
            sum += v;
            sum2 += (double)(v * v);
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
    if (!WIDE || tid < 256) {
        s_sum[tid] = sum;
        s_sum2[tid] = sum2;
        s_min[tid] = mn;
        s_max[tid] = mx;
    }
    __syncthreads();
    for (int s = rpp >> 1; s > 0; s >>= 1) {
        if (rr < s) { // (rr < s <= rpp / 2: threads of the first 256 only)
            const int o = tid + (s << lg);
            s_sum[tid] += s_sum[o];
            s_sum2[tid] += s_sum2[o];
            s_min[tid] = fminf(s_min[tid], s_min[o]);
            s_max[tid] = fmaxf(s_max[tid], s_max[o]);
        }
        __syncthreads();
    }
}

} // namespace mfx
