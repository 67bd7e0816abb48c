// mfx_stft_dev.h -- device pieces the STFT log-mel kernels share (mfx_stft.hip: k_stft_mel, k_sess_stft_mel, the matrix form;
// mfx_stft_fft.hip: k_stft_fft_mel, the FFT form):
//   stft_bins, stft_p_pitch   bins of a DFT of N points; the row pitch of the power rows in LDS
//   stft_stage_span           the PCM span of a run of centred frames into LDS: reflected, converted, scaled
//   stft_mel_log              the Slaney mel chains and the log over power rows in LDS, one (frame, band) per thread
//   wave_max                  the largest value of a wave's lanes
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mfx_dev.h"
#include "mfx_kernels.h"
#include "mfx_tile_dev.h"

namespace mfx {
namespace {

__host__ __device__ inline int stft_bins(int N) { return N / 2 + 1; }
__host__ __device__ inline int stft_p_pitch(int N) { return stft_bins(N) | 1; } // odd: a column of P spreads over the banks

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Words [0, span) of s_x: samples base .. base + span - 1 of the utterance (or stream) of n samples whose sample 0 lies -- or
// would lie -- at element `off` of pcm, reflected at its ends, converted and scaled by 2^-15; words [span, all): zeros.  A
// reflected index that still leaves [0, n), or an element outside [0, elems) of pcm, is never read: the word is zero.
__device__ __forceinline__ void stft_stage_span(const int16_t *pcm, int64_t off, int64_t elems, int64_t n, int64_t base, int span, int all,
                                                float *s_x, int tid)
{
    for (int i = tid; i < all; i += 256) {
        float v = 0.f;
        if (i < span) {
            int64_t j = base + i;
            if (j < 0) j = -j;
            if (j >= n) j = 2 * (n - 1) - j;
            const int64_t e = off + j;
            if (j >= 0 && j < n && e >= 0 && e < elems) v = (float)pcm[e] * (1.0f / 32768.0f);
        }
        s_x[i] = v;
    }
}

// The mel chains and the log of `rows` frames whose power lies in s_P [rows][KP], one (frame, band) per thread and trip, to
// s_out [rows][M]; returns the thread's largest log value.  T: the parameters of any of the kernels.
template <class T>
__device__ __forceinline__ float stft_mel_log(const T &p, const float *s_P, int KP, int rows, float *s_out, int tid)
{
    float mx = -INFINITY;
    const int M = p.M, n = rows * M;
    const uint32_t magic = div_magic(M);
    for (int i = tid; i < n; i += 256) {
        const int t = div_small(i, M, magic);
        const int m = i - t * M;
        const int beg = p.mel_beg[m], len = p.mel_len[m];
        const float *w = p.mel_w + p.mel_off[m];
        const float *P = s_P + t * KP + beg;
        float acc = 0.f;
        for (int j = 0; j < len; ++j) acc = __builtin_fmaf(w[j], P[j], acc);
        const float v = fmaxf(acc, 1e-10f);
        float L;
        if (p.post == 2)
            L = logf(v);
        else
            L = v == 1e-10f ? -10.0f : log10f(v);
        s_out[i] = L;
        mx = fmaxf(mx, L);
    }
    return mx;
}

} // namespace
} // namespace mfx
