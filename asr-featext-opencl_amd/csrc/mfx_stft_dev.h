// mfx_stft_dev.h -- device pieces the STFT log-mel kernels share (mfx_stft.hip: k_stft_mel, k_sess_stft_mel, the matrix form;
// mfx_stft_fft.hip: k_stft_fft_mel, the FFT form):
//   stft_bins, stft_p_pitch   bins of a DFT of N points; the row pitch of the power rows in LDS
//   stft_stage_span           the PCM span of a run of centred frames into LDS: reflected, converted, scaled
//   stft_xo_floats            the overlay both block kernels stage their span in and assemble their rows in
//   stft_mel_log              the Slaney mel chains (mel_span_chain of mfx_wavefft_dev.h) and the log over power rows in LDS, one
//                             (frame, band) per thread
//   stft_finish_block         the tail of a block of the batch kernels: mel and log, the block's maximum, the rows out
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mfx_dev.h"
#include "mfx_kernels.h"
#include "mfx_tile_dev.h"
#include "mfx_wavefft_dev.h"

namespace mfx {

// the FFT form's side of launch_stft / stft_lds_bytes (mfx_stft_fft.hip): its block's LDS, and k_stft_fft_mel
size_t stft_fft_lds_bytes(int N, int S, int M, int tile_rows);
const void *stft_fft_kernel();

namespace {

__host__ __device__ inline int stft_bins(int N) { return N / 2 + 1; }
__host__ __device__ inline int stft_p_pitch(int N) { return stft_bins(N) | 1; } // odd: a column of P spreads over the banks

// floats of the staged span of R frames and `pad` words behind it (the matrix form: 4 words of zeros for the padded taps of
// the last frame; the FFT form: none) -- the finished rows [R][M] are assembled in the same words once the DFT is done
__host__ __device__ inline int stft_xo_floats(int N, int S, int M, int R, int pad)
{
    const int a = (R - 1) * S + N + pad, b = R * M;
    return ((a > b ? a : b) + 3) & ~3;
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
// s_out [rows][M]; returns the thread's largest log value.
__device__ __forceinline__ float stft_mel_log(const StftCore &p, const float *s_P, int KP, int rows, float *s_out, int tid)
{
    float mx = -INFINITY;
    const int M = p.M, n = rows * M;
    const uint32_t magic = div_magic(M);
    for (int i = tid; i < n; i += 256) {
        const int t = div_small(i, M, magic);
        const int m = i - t * M;
        const int beg = p.mel.beg[m], len = p.mel.len[m];
        const float acc = mel_span_chain(p.mel.w + p.mel.off[m], s_P + t * KP + beg, len);
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

// The tail of a block of k_stft_mel / k_stft_fft_mel once the power of its `rows` frames lies in s_P (every thread calls this,
// behind a block barrier): mel and log into s_out, the block's largest log value into *blk_max_slot through s_red [4], the rows
// to the chunk's place in core.out.
__device__ __forceinline__ void stft_finish_block(const StftCore &core, const float *s_P, int KP, int rows, float *s_out, float *s_red,
                                                  float *blk_max_slot, const StftChunk &ck, int tid)
{
    float mx = stft_mel_log(core, s_P, KP, rows, s_out, tid);
    mx = wave_max(mx);
    if ((tid & 63) == 0) s_red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) *blk_max_slot = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));

    tile_store_rows(s_out, core.M, rows, core.out, ck.out_row, core.out_pitch, tid);
}

} // namespace
} // namespace mfx
