// mfx_onorm_dev.h -- device code of the online (causal) normaliser that the batch kernels (mfx_onorm.hip: k_onorm_totals,
// k_onorm_offsets, k_onorm_apply) and the session kernel (k_onorm_sess) share: the links of the double chains and the
// statistics of one row.  One definition, so that a session's rows are the bits of the batch's.  include/mfx.h,
// mfx_batch_set_online_norm, is the definition; every double operation here is rounded on its own (the device build
// contracts a * b + c unless told otherwise, hence the pragma in every body).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mfx_kernels.h"

namespace mfx {

// what the statistics of a row need beside its window sums
struct OnormStat {
    int32_t cvn;           // 0: CMN, else CVN
    int32_t prior_frames;  // F
    int64_t prior_count;   // p (0: no prior)
};

// the q of a row's value: the float32 product as a double (k_norm_stats' rule)
__device__ __forceinline__ double onorm_sq(float v)
{
#pragma clang fp contract(off)
    const float q = v * v;
    return (double)q;
}

// one link of a chain: a + (double)v, and the sum of two chain values
__device__ __forceinline__ double onorm_add(double a, double b)
{
#pragma clang fp contract(off)
    return a + b;
}

__device__ __forceinline__ double onorm_sub(double a, double b)
{
#pragma clang fp contract(off)
    return a - b;
}

// Row t of a stream at one column: v its raw value, (Sw, Qw) the window sums of v and q over the n rows of the window,
// (ps, pq) the prior's sums of that column (read only when prior_count > 0).  Returns the normalised value.
__device__ __forceinline__ float onorm_row(float v, double Sw, double Qw, int64_t n, const OnormStat &s, double ps, double pq)
{
#pragma clang fp contract(off)
    int64_t k = 0;
    if (s.prior_count > 0 && (int64_t)s.prior_frames > n) k = min(s.prior_count, (int64_t)s.prior_frames - n);
    if (k > 0) {
        const double r = (double)k / (double)s.prior_count;
        const double a = ps * r, b = pq * r;
        Sw = Sw + a;
        Qw = Qw + b;
    }
    const double nn = (double)(n + k);
    const double m = Sw / nn;
    const float mean = (float)m;
    const float c = v - mean;
    if (!s.cvn) return c;
    const double sm = Sw * m;
    const double d = Qw - sm;
    float mult = 1.0f;
    if (nn >= 2.0 && d > 0.0) {
        const double num = nn - 1.0;
        const double ratio = num / d;
        mult = (float)sqrt(ratio);
    }
    return c * mult;
}

} // namespace mfx
