// mfx_onorm_dev.h -- device code of the online (causal) normaliser that the batch kernels (mfx_onorm.hip: k_onorm_totals,
// k_onorm_offsets, k_onorm_apply) and the session kernel (k_onorm_sess) share: the links of the double chains and the
// statistics of one row; and what the sliding-window normaliser's kernel (mfx_slide.hip: k_slide_apply) takes from them: the
// links, the tiles' LDS image, its own row (slide_row).  One definition, so that a session's rows are the bits of the batch's.  include/mfx.h,
// mfx_batch_set_online_norm, is the definition; every double operation here is rounded on its own (the device build
// contracts a * b + c unless told otherwise, hence the pragma in every body).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mfx_kernels.h"

namespace mfx {

// A block of the batch kernels (k_onorm_totals, k_onorm_apply, k_slide_apply) serves G = max(1, 256 / Wn) chunks: thread tid
// is (tile g = tid / Wn, column j = tid % Wn), so that a 39-column row still fills the block's lanes.
__device__ __forceinline__ int onorm_tiles(int Wn) { return Wn >= 256 ? 1 : 256 / Wn; }

// The block's G tiles between HBM and their LDS image [kOnormChunk][G * Wn]: row r of ALL the tiles is one run of G * Wn
// floats, so the column walk of thread tid touches word r * G * Wn + tid -- the lanes of a wave on consecutive words at every
// width (no bank conflict, no padding needed) -- and the loops below walk the same words in order: HBM is read and written in
// whole row pieces of Wn floats.  Tile g holds rows [row0[g], row0[g] + rows[g]) of the source; the load leaves zeros behind
// a tile's last row.  Word i is (row r = i / GW, tile, column c): i / GW and rem / Wn for i < 2^16 as multiply-highs (Wn == 1
// would wrap the constant to 0: the shift form).  256 threads; the caller puts the barriers around them.
struct OnormTileIndex {
    int Wn, GW;
    uint32_t magic_gw, magic;
    __device__ __forceinline__ OnormTileIndex(int wn, int G)
        : Wn(wn), GW(G * wn), magic_gw(0xffffffffu / (uint32_t)(G * wn) + 1), magic(wn > 1 ? 0xffffffffu / (uint32_t)wn + 1 : 0)
    {
    }
    __device__ __forceinline__ void split(int i, int &r, int &gg, int &c) const
    {
        r = (int)__umulhi((uint32_t)i, magic_gw);
        const int rem = i - r * GW;
        gg = Wn > 1 ? (int)__umulhi((uint32_t)rem, magic) : rem;
        c = rem - gg * Wn;
    }
};

// (four loads are in flight before the first LDS write waits for them)
__device__ __forceinline__ void onorm_tiles_load(const OnormTileIndex &ix, const float *src, int src_pitch, const int64_t *row0,
                                                 const int32_t *rows, float *tile, int tid)
{
    const int words = kOnormChunk * ix.GW;
    for (int i0 = tid; i0 < words; i0 += 4 * 256) {
        float a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + k * 256;
            a[k] = 0.f;
            if (i < words) {
                int r, gg, c;
                ix.split(i, r, gg, c);
                if (r < rows[gg]) a[k] = src[(row0[gg] + r) * (int64_t)src_pitch + c];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k * 256 < words) tile[i0 + k * 256] = a[k];
    }
}

__device__ __forceinline__ void onorm_tiles_store(const OnormTileIndex &ix, float *out, int out_pitch, const int64_t *row0,
                                                  const int32_t *rows, const float *tile, int tid)
{
    const int words = kOnormChunk * ix.GW;
    for (int i = tid; i < words; i += 256) {
        int r, gg, c;
        ix.split(i, r, gg, c);
        if (r < rows[gg]) out[(row0[gg] + r) * (int64_t)out_pitch + c] = tile[i];
    }
}

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

// The sliding-window normaliser's row (include/mfx.h, mfx_batch_set_sliding_norm; k_slide_apply): v the raw value, (Sw, Qw)
// the sums of v and q over the n >= 1 rows of the window.  Kaldi's population variance and floor, no prior.
__device__ __forceinline__ float slide_row(float v, double Sw, double Qw, int n, int norm_vars)
{
#pragma clang fp contract(off)
    const double nn = (double)n;
    const double m = Sw / nn;
    const float mean = (float)m;
    const float c = v - mean;
    if (!norm_vars) return c;
    if (n == 1) return 0.0f;
    const double e2 = Qw / nn;
    const double mm = m * m;
    double var = e2 - mm;
    if (var < 1e-10) var = 1e-10;
    const double sd = sqrt(var);
    const double inv = 1.0 / sd;
    return c * (float)inv;
}

} // namespace mfx
