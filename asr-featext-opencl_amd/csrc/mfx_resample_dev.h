// mfx_resample_dev.h -- device pieces shared by the two sample-rate converters, k_resample (mfx_resample.hip: tiles of whole
// utterances of a batch) and k_sess_resample (mfx_sess_resample.hip: tiles of the pieces of a push, their input staged from a
// session's carried tail and the caller's array).  See DESIGN.md, "Sample-rate conversion" and "Session sample-rate
// conversion".
//   lo16 / hi16       the two samples of a 32-bit word, as floats
//   to_pcm            accumulator -> int16: rintf, clamp
//   convert_items     the outputs of a tile dealt to work items, every output's whole ascending FMA chain in one thread
//   convert_tile      convert_items at the rate's R
// Both kernels stage a tile's input span in LDS as floats, one plane per channel (`s_x`, `xf` floats per plane, position
// `base_n` of the utterance / stream at index 0), and call convert_tile on it: the one FMA chain, so they deliver the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "mfx_kernels.h"

#include <type_traits>

namespace mfx {
namespace {

typedef float rs_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float lo16(uint32_t w) { return (float)(int16_t)(w & 0xffffu); }
__device__ __forceinline__ float hi16(uint32_t w) { return (float)((int32_t)w >> 16); }

__device__ __forceinline__ int16_t to_pcm(float acc)
{
    return (int16_t)(int)fminf(fmaxf(rintf(acc), -32768.f), 32767.f);
}

template <int CH, int R, bool LDS_TAPS>
__device__ __forceinline__ void convert_items(const ResRate &r, const ResTile &t, const float *taps, int tap_stride, const float *s_x,
                                              int xf, int16_t *s_out, int nout, int64_t base_n)
{
    // (LDS_TAPS: the table pointer keeps its LDS address space through the call, so the tap reads are ds_read, not flat loads)
    using TapPtr = typename std::conditional<LDS_TAPS, const __attribute__((address_space(3))) float *, const float *>::type;
    const int NI = r.items, P = r.P;
    const int step = (int)(((int64_t)NI * r.M) / r.L); // input samples between the same-phase outputs of an item (exact for R > 1)
    for (int w = threadIdx.x; w < NI && w < nout; w += 256) {
        const int64_t jm = (t.j0 + w) * (int64_t)r.M;
        const int64_t n = jm / r.L;
        const int phi = (int)(jm - n * r.L);
        const TapPtr h = (TapPtr)taps + phi * tap_stride;
        const int xb0 = (int)(n - r.Wh + 1 - base_n);
        const float *xp[R];
        float acc[CH][R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            xp[q] = s_x + (w + q * NI < nout ? xb0 + q * step : 0);
#pragma unroll
            for (int c = 0; c < CH; ++c) acc[c][q] = 0.f;
        }
#pragma unroll 4
        for (int k = 0; k < P; ++k) {
            const float hk = h[k];
#pragma unroll
            for (int q = 0; q < R; ++q)
#pragma unroll
                for (int c = 0; c < CH; ++c) acc[c][q] = __builtin_fmaf(hk, xp[q][c * xf + k], acc[c][q]);
        }
#pragma unroll
        for (int q = 0; q < R; ++q)
            if (w + q * NI < nout)
#pragma unroll
                for (int c = 0; c < CH; ++c) s_out[(w + q * NI) * CH + c] = to_pcm(acc[c][q]);
    }
}

template <int CH, bool LDS_TAPS>
__device__ __forceinline__ void convert_tile(const ResRate &r, const ResTile &t, const float *taps, int tap_stride, const float *s_x,
                                             int xf, int16_t *s_out, int nout, int64_t base_n)
{
    if (r.R == 4)
        convert_items<CH, 4, LDS_TAPS>(r, t, taps, tap_stride, s_x, xf, s_out, nout, base_n);
    else if (r.R == 2)
        convert_items<CH, 2, LDS_TAPS>(r, t, taps, tap_stride, s_x, xf, s_out, nout, base_n);
    else
        convert_items<CH, 1, LDS_TAPS>(r, t, taps, tap_stride, s_x, xf, s_out, nout, base_n);
}

} // namespace
} // namespace mfx
