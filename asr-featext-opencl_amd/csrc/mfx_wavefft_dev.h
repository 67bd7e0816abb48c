// mfx_wavefft_dev.h -- what the two FFT front ends whose frames live in LDS share (mfx_kaldi_dev.h: k_kaldi_front and
// k_kaldi_front_opts, M = 64 / 128 / 256; mfx_stft_fft.hip: k_stft_fft_mel, M = 512 / 1024):
//   wave_fft_half      a complex FFT of M points by one wave, in place in its LDS buffer: Stockham autosort, radix 4, and one last
//                      stage of radix 2 where M is no power of 4
//   real_split_power   bin k of the real frame's DFT from Z[k] and Z[M - k], and its power
//   mel_span_chain     one band's ascending FMA chain over its span of a power row
// The register front ends have an FFT core of their own (mfx_front_dev.h).
#pragma once
#include <hip/hip_runtime.h>

#include "mfx_dev.h"

namespace mfx {
namespace {

// One radix-4 Stockham stage over the M points of the wave's buffer, in place: sub-transform length LEN before the stage,
// stride ST = M / LEN.  A lane holds max(1, M / 256) of the M / 4 butterflies (below 256 points lanes from M / 4 on hold none);
// it reads the inputs of all of them into registers, the wave synchronises, then it writes: one buffer serves, and only the wave
// synchronises.  tw: W_M^k, k < M.
template <int M, int LEN>
__device__ __forceinline__ void wave_fft_stage4(float2 *buf, const float2 *tw, int lane)
{
    constexpr int ST = M / LEN, N1 = LEN / 4, NBF = M / 4, NB = NBF < 64 ? 1 : NBF / 64;
    constexpr bool GUARD = NBF < 64;
    float2 v[NB][4] = {};
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int idx = lane + 64 * b, pp = idx / ST, q = idx % ST;
        if (GUARD && idx >= NBF) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[b][r] = buf[q + ST * (pp + r * N1)];
    }
    wave_sync();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int idx = lane + 64 * b, pp = idx / ST, q = idx % ST;
        if (GUARD && idx >= NBF) continue;
        float2 o0, o1, o2, o3;
        dft4(v[b][0], v[b][1], v[b][2], v[b][3], o0, o1, o2, o3);
        float2 *y = buf + q + ST * (4 * pp);
        y[0] = o0;
        if (LEN == 4) { // (pp = 0: no twiddles)
            y[ST] = o1, y[2 * ST] = o2, y[3 * ST] = o3;
        } else {
            y[ST] = cmul(o1, tw[pp * ST]);
            y[2 * ST] = cmul(o2, tw[2 * pp * ST]);
            y[3 * ST] = cmul(o3, tw[3 * pp * ST]);
        }
    }
    wave_sync();
}

// the last stage of M = 128 and 512: radix 2 at sub-transform length 2 (no twiddles), M / 128 butterflies per lane
template <int M>
__device__ __forceinline__ void wave_fft_stage2_last(float2 *buf, int lane)
{
    constexpr int ST = M / 2, NB = M / 128;
    float2 v[NB][2];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int q = lane + 64 * b;
        v[b][0] = buf[q], v[b][1] = buf[q + ST];
    }
    wave_sync();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int q = lane + 64 * b;
        buf[q] = make_float2(v[b][0].x + v[b][1].x, v[b][0].y + v[b][1].y);
        buf[q + ST] = make_float2(v[b][0].x - v[b][1].x, v[b][0].y - v[b][1].y);
    }
    wave_sync();
}

// the stages at sub-transform lengths M, M / 4, ... down to 4, or to 8 and then the stage of radix 2
template <int M, int LEN = M>
__device__ __forceinline__ void wave_fft_half(float2 *buf, const float2 *tw, int lane)
{
    static_assert(M == 64 || M == 128 || M == 256 || M == 512 || M == 1024, "the lengths of the two front ends");
    if constexpr (LEN >= 4) {
        wave_fft_stage4<M, LEN>(buf, tw, lane);
        wave_fft_half<M, LEN / 4>(buf, tw, lane);
    } else if constexpr (LEN == 2) {
        wave_fft_stage2_last<M>(buf, lane);
    }
}

// The real split 2 X[k] = (Z[k] + conj Z[M - k]) + w (Z[k] - conj Z[M - k]), w = -i W_N^k, the factor 2 taken out by an exact
// 0.5f: |X[k]|^2 from zk = Z[k], zm = Z[(M - k) mod M].
__device__ __forceinline__ float real_split_power(float2 zk, float2 zm, float2 w)
{
    const float sr = zk.x + zm.x, si = zk.y - zm.y;
    const float dr = zk.x - zm.x, di = zk.y + zm.y;
    const float re = 0.5f * (sr + (w.x * dr - w.y * di));
    const float im = 0.5f * (si + (w.x * di + w.y * dr));
    return __builtin_fmaf(im, im, re * re);
}

// sum_j w[j] P[j], j < len, ascending, one FMA per weight
__device__ __forceinline__ float mel_span_chain(const float *w, const float *P, int len)
{
    float acc = 0.f;
    for (int j = 0; j < len; ++j) acc = __builtin_fmaf(w[j], P[j], acc);
    return acc;
}

} // namespace
} // namespace mfx
