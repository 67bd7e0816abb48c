// mfx_stft_fft.hip -- k_stft_fft_mel: the STFT log-mel front end (MFX_METHOD_STFT_LOGMEL) at DFT lengths 1024 and 2048, where
// the matrix form of mfx_stft.hip (N^2 / 2 multiply-adds per frame, N^2 floats of basis) is no option, and its launcher.  See
// DESIGN.md, "STFT log-mel, FFT form".
//
// Frames, samples, power, mel, log and post are those of mfx_stft.hip; window and DFT are
//   z[j]   = x[j] * w[j]                                   (one float32 product, w the caller's N floats)
//   X[k]   = sum_j z[j] e^(-2 pi i j k / N), k < K1        (a float32 FFT, not pinned to a summation order)
//
// A block of 4 waves takes R = 16, 8 or 4 consecutive frames of one utterance (StftChunk, as k_stft_mel).  Their PCM span, (R -
// 1) S + N floats, is staged once in LDS (stft_stage_span); the window and the twiddles W_M^k (M = N / 2) are kept once per
// block in LDS.  Wave w takes frames w, w + 4, ... of the chunk, one after the other, in its own buffer of M complex points:
//   - the frame as M complex points (z[2 n], z[2 n + 1]);
//   - a complex FFT of M points, Stockham autosort, radix 4 (M = 1024: five stages; M = 512: four, then one of radix 2):
//     wave_fft_half of mfx_wavefft_dev.h, which the Kaldi front end shares.  A stage reads all of its inputs into registers
//     before it writes any output, so ONE buffer serves (k_front_wave's loop needs two), and only the wave synchronises;
//   - the real split 2 X[k] = (Z[k] + conj Z[M - k]) - i W_N^k (Z[k] - conj Z[M - k]) (real_split_power of the same header),
//     its table read from memory (one coalesced 8-byte read per bin), and the power into s_P [frame][KP].
// The float32 operations a frame sees are those of this one instruction stream: they depend on N alone, not on the tile, the
// wave, the frame's place in its block, or the batch.  After a block barrier the mel chains and the log run one (frame, band)
// per thread (stft_mel_log) into the span's words -- every wave has left the span by then --, the block's largest log value
// goes to its slot of blk_max, and the rows leave through tile_store_rows.  k_stft_post follows unchanged for WHISPER.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_dev.h"
#include "mfx_stft_dev.h"
#include "mfx_tile_dev.h"
#include "mfx_wavefft_dev.h"

namespace mfx {

namespace {

// LDS, all of it dynamic (stft_fft_lds_bytes is the whole of what a block asks for):
//   s_x [max((R - 1) S + N, R M)] (later s_out [R][M]) | window [N] | W_M^k [M] complex | FFT buffers [4][M] complex | s_P [R][KP]
//   | s_red [4]
template <int M>
__device__ __forceinline__ void stft_fft_block(const StftParams &p, float *smem)
{
    constexpr int N = 2 * M, KP = (M + 1) | 1;
    const StftChunk ck = p.chunks[blockIdx.x];
    const int R = p.tile_rows, S = p.core.S, nb = p.core.M;
    const int rows = ck.n_frames;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *s_x = smem;
    float *s_w = s_x + stft_xo_floats(N, S, nb, R, 0);
    const float2 *s_tw = (const float2 *)(s_w + N);
    float2 *s_f = (float2 *)(s_w + 2 * N) + wave * M;
    float *s_P = s_w + 6 * N;
    float *s_red = s_P + R * KP; // the waves' maxima

    {   // the span of frames t0 .. t0 + rows - 1, reflected at the ends of the utterance; the window and the twiddles
        const int span = (rows - 1) * S + N;
        stft_stage_span(p.pcm, ck.utt_off, INT64_MAX, ck.utt_len, (int64_t)ck.t0 * S - N / 2, span, span, s_x, tid);
        for (int i = tid; i < 2 * N; i += 256) s_w[i] = p.core.operands[i];
    }
    __syncthreads();

    const float2 *cs = (const float2 *)(p.core.operands + 2 * N); // -i W_N^k, k <= M
    for (int f = wave; f < rows; f += 4) {
        const float *xs = s_x + f * S;
#pragma unroll
        for (int b = 0; b < M / 64; ++b) {
            const int n = lane + 64 * b;
            const float2 w = ((const float2 *)s_w)[n];
            s_f[n] = make_float2(xs[2 * n] * w.x, xs[2 * n + 1] * w.y);
        }
        wave_sync();
        wave_fft_half<M>(s_f, s_tw, lane);
        float *P = s_P + f * KP;
#pragma unroll
        for (int b = 0; b <= M / 64; ++b) { // (bin M: lane 0 of the last trip)
            const int k = lane + 64 * b;
            if (k > M) break;
            P[k] = real_split_power(s_f[k & (M - 1)], s_f[(M - k) & (M - 1)], cs[k]);
        }
        wave_sync(); // (the next frame takes the buffer)
    }
    __syncthreads(); // every wave has left the span: the rows may take its words

    stft_finish_block(p.core, s_P, KP, rows, s_x, s_red, p.blk_max + (p.chunk_first + blockIdx.x), ck, tid);
}

__global__ void __launch_bounds__(256) k_stft_fft_mel(StftParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (p.core.N == 1024)
        stft_fft_block<512>(p, smem);
    else
        stft_fft_block<1024>(p, smem);
}

} // namespace

size_t stft_fft_lds_bytes(int N, int S, int M, int tile_rows)
{
    const size_t f = (size_t)stft_xo_floats(N, S, M, tile_rows, 0) + (size_t)2 * N /* window, twiddles */ + (size_t)4 * N /* FFT buffers */ +
                     (size_t)tile_rows * stft_p_pitch(N) + 4 /* s_red */;
    return f * sizeof(float);
}

const void *stft_fft_kernel() { return (const void *)k_stft_fft_mel; }

} // namespace mfx
