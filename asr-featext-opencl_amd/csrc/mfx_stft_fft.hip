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
//   - a complex FFT of M points, Stockham autosort, radix 4 (M = 1024: five stages; M = 512: four, then one of radix 2).  A
//     stage reads all of its inputs into registers before it writes any output, so ONE buffer serves (k_front_wave's loop
//     needs two), and only the wave synchronises (wave_sync);
//   - the real split 2 X[k] = (Z[k] + conj Z[M - k]) - i W_N^k (Z[k] - conj Z[M - k]), its table read from memory (one
//     coalesced 8-byte read per bin), the factor 2 taken out by an exact 0.5f, and the power into s_P [frame][KP].
// The float32 operations a frame sees are those of this one instruction stream: they depend on N alone, not on the tile, the
// wave, the frame's place in its block, or the batch.  After a block barrier the mel chains and the log run one (frame, band)
// per thread (stft_mel_log) into the span's words -- every wave has left the span by then --, the block's largest log value
// goes to its slot of blk_max, and the rows leave through tile_store_rows.  k_stft_post follows unchanged for WHISPER.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_dev.h"
#include "mfx_stft_dev.h"
#include "mfx_tile_dev.h"

namespace mfx {

namespace {

// One radix-4 Stockham stage over the M points of the wave's buffer, in place: sub-transform length LEN before the stage,
// stride ST = M / LEN; every lane reads the inputs of its M / 256 butterflies, the wave synchronises, then it writes.
// tw: W_M^k, k < M.
template <int M, int LEN>
__device__ __forceinline__ void stft_fft_stage4(float2 *buf, const float2 *tw, int lane)
{
    constexpr int ST = M / LEN, N1 = LEN / 4, NB = M / 256;
    float2 v[NB][4];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int idx = lane + 64 * b, pp = idx / ST, q = idx % ST;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[b][r] = buf[q + ST * (pp + r * N1)];
    }
    wave_sync();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int idx = lane + 64 * b, pp = idx / ST, q = idx % ST;
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

// the last stage of M = 512: radix 2 at sub-transform length 2 (no twiddles)
template <int M>
__device__ __forceinline__ void stft_fft_stage2_last(float2 *buf, int lane)
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

template <int M>
__device__ __forceinline__ void stft_fft_half(float2 *buf, const float2 *tw, int lane)
{
    static_assert(M == 512 || M == 1024, "the two lengths of the FFT form");
    stft_fft_stage4<M, M>(buf, tw, lane);
    stft_fft_stage4<M, M / 4>(buf, tw, lane);
    stft_fft_stage4<M, M / 16>(buf, tw, lane);
    stft_fft_stage4<M, M / 64>(buf, tw, lane);
    if constexpr (M == 1024)
        stft_fft_stage4<M, 4>(buf, tw, lane);
    else
        stft_fft_stage2_last<M>(buf, lane);
}

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
        stft_fft_half<M>(s_f, s_tw, lane);
        float *P = s_P + f * KP;
#pragma unroll
        for (int b = 0; b <= M / 64; ++b) { // (bin M: lane 0 of the last trip)
            const int k = lane + 64 * b;
            if (k > M) break;
            const float2 zk = s_f[k & (M - 1)], zm = s_f[(M - k) & (M - 1)];
            const float sr = zk.x + zm.x, si = zk.y - zm.y;
            const float dr = zk.x - zm.x, di = zk.y + zm.y;
            const float2 w = cs[k];
            const float re = 0.5f * (sr + (w.x * dr - w.y * di));
            const float im = 0.5f * (si + (w.x * di + w.y * dr));
            P[k] = __builtin_fmaf(im, im, re * re);
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
