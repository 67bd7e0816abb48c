// mfx_kaldi_dev.h -- the block body of the Kaldi front end, shared by k_kaldi_front (mfx_kaldi.hip) and k_kaldi_front_opts
// (mfx_kaldi_opts.hip: the build for kaldi_flags of mfx_create_kaldi != 0).  mfx_kaldi.hip describes the structure; the wave FFT,
// the real split and the mel chain are those of mfx_wavefft_dev.h, which the STFT FFT form shares.
#pragma once
#include <hip/hip_runtime.h>

#include "mfx_dev.h"
#include "mfx_kernels.h"
#include "mfx_tile_dev.h"
#include "mfx_wavefft_dev.h"

namespace mfx {

namespace {

constexpr int kKaldiRows = 16; // frames of a chunk at most (kChunkFrames of the planner)

__host__ __device__ inline int kaldi_p_pitch(int N) { return (N / 2) | 1; } // odd: a column of P spreads over the banks
// floats of the staged span of 16 frames; the log mel rows [16][M] are assembled in the same words once the DFTs are done
__host__ __device__ inline int kaldi_xo_floats(int W, int S, int M)
{
    const int a = (kKaldiRows - 1) * S + W, b = kKaldiRows * M;
    return ((a > b ? a : b) + 3) & ~3;
}
__host__ __device__ inline int kaldi_c_floats(int C) { return (kKaldiRows * C + 3) & ~3; }
__host__ __device__ inline int kaldi_meta_words(int M) { return (3 * M + 3) & ~3; }

// LDS, all of it dynamic (kaldi_lds_bytes is the whole of what a block asks for):
//   s_x [max(15 S + W, 16 M)] (later the log mel rows [16][M]) | s_c [16][C] | window [N] | W_MH^k [MH] complex | -i W_N^k [MH]
//   complex | FFT buffers [4][MH] complex | mel weights [N] | mel spans [3][M] | s_P [16][KP]
// OPTS: the build for kaldi_flags != 0 (include/mfx.h, "Options").  The span is gathered through the utterance's mirror, the
// frame's log-energy waits in the pad word of its s_P row (index MH: no bin lies there), and the energy column and the HTK order
// are placed where s_x / s_c are filled -- fbank rows are M + 1 floats wide then.  Without OPTS the code is what it was.
template <int MH, bool OPTS>
__device__ __forceinline__ void kaldi_block(const KaldiParams &p, float *smem)
{
    constexpr int N = 2 * MH, KP = MH | 1;
    const Chunk ck = p.chunks[blockIdx.x];
    const int64_t rows_left = p.row_limit - ck.out_row;
    const int nf = ck.n_frames < kKaldiRows ? ck.n_frames : kKaldiRows;
    const int rows = (int)(rows_left < nf ? (rows_left < 0 ? 0 : rows_left) : nf);
    if (rows <= 0) return;
    const int W = p.W, S = p.S, nb = p.M, C = p.C;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int flags = OPTS ? p.flags : 0;
    const bool energy = OPTS && (flags & kKaldiUseEnergy), htk = OPTS && (flags & kKaldiHtkCompat);
    const int cols = OPTS ? kaldi_static_cols(nb, C, flags) : (C > 0 ? C : nb);
    const int xp = OPTS && C == 0 ? cols : nb; // floats of a log mel row in s_x
    float *s_x = smem;
    float *s_c = s_x + kaldi_xo_floats(W, S, xp);
    float *s_w = s_c + kaldi_c_floats(C);
    const float2 *s_tw = (const float2 *)(s_w + N);
    const float2 *s_sp = (const float2 *)(s_w + 2 * N);
    float2 *s_f = (float2 *)(s_w + 3 * N) + wave * MH;
    float *s_mw = s_w + 7 * N;
    int32_t *s_meta = (int32_t *)(s_mw + N);
    float *s_P = s_mw + N + kaldi_meta_words(nb);

    {   // the span of frames 0 .. rows - 1 of the chunk: nothing before its first sample, nothing behind its last
        const int span = (rows - 1) * S + W;
        if (OPTS && (flags & kKaldiNoSnipEdges)) { // centred frames: the utterance mirrored at both ends, never a neighbour
            // (launch_kaldi refuses a launch without bounds; plan_batch numbers `pad` inside them and gives no chunk to an empty
            // utterance: the two returns keep a block from reading outside the table, they are not a path a plan can take)
            if (!p.utt_bounds || ck.pad < 0 || ck.pad >= p.n_utt) return;
            const int64_t uo = p.utt_bounds[2 * (int64_t)ck.pad], un = p.utt_bounds[2 * (int64_t)ck.pad + 1];
            if (un <= 0) return;
            const int64_t s0 = ck.pcm_off - uo;
            for (int i = tid; i < span; i += 256) {
                int64_t s = s0 + i;
                if (s < 0 || s >= un) s = kaldi_reflect(s, un); // (only the chunks at an utterance's ends get here)
                const int64_t e = uo + s;
                s_x[i] = (e >= 0 && e < p.pcm_total) ? (float)p.pcm[e] : 0.f;
            }
        } else {
#pragma unroll 4
            for (int i = tid; i < span; i += 256) {
                const int64_t e = ck.pcm_off + i;
                s_x[i] = (e >= 0 && e < p.pcm_total) ? (float)p.pcm[e] : 0.f;
            }
        }
#pragma unroll
        for (int i = tid; i < 3 * N; i += 256) s_w[i] = p.operands[i];
        const int nw = p.mel_w_floats < N ? p.mel_w_floats : N;
        for (int i = tid; i < nw; i += 256) s_mw[i] = p.mel.w[i];
        for (int i = tid; i < nb; i += 256) s_meta[i] = p.mel.beg[i], s_meta[nb + i] = p.mel.len[i], s_meta[2 * nb + i] = p.mel.off[i];
    }
    __syncthreads();

    const float c = p.preemph, fW = (float)W;
    for (int f = wave; f < rows; f += 4) {
        const float *xs = s_x + f * S;
        float mean = 0.f;
        if (p.remove_dc) { // the exact sum: int32 holds 512 samples of 16 bits
            int s = 0;
            for (int i = lane; i < W; i += 64) s += (int)xs[i];
            mean = (float)wave_sum_i32(s) / fW;
        }
        float en = 0.f;
#pragma unroll
        for (int b = 0; b < MH / 64; ++b) {
            const int n = lane + 64 * b, i0 = 2 * n, i1 = i0 + 1;
            float2 z = make_float2(0.f, 0.f);
            if (i0 < W) {
                const float d0 = xs[i0] - mean;
                const float dp = i0 == 0 ? d0 : xs[i0 - 1] - mean; // (the frame's first sample stands for its predecessor)
                z.x = __builtin_fmaf(-c, dp, d0) * s_w[i0];
                if (i1 < W) z.y = __builtin_fmaf(-c, d0, xs[i1] - mean) * s_w[i1];
                if (energy) { // the lane's chain, taps ascending: d before pre-emphasis (raw), or z
                    if (flags & kKaldiEnergyWindowed) {
                        en = __builtin_fmaf(z.x, z.x, en);
                        en = __builtin_fmaf(z.y, z.y, en);
                    } else {
                        en = __builtin_fmaf(d0, d0, en);
                        if (i1 < W) {
                            const float d1 = xs[i1] - mean;
                            en = __builtin_fmaf(d1, d1, en);
                        }
                    }
                }
            }
            s_f[n] = z;
        }
        if (energy) {
            const float le = fmaxf(logf(fmaxf(wave_sum_f32(en), 0x1p-23f)), p.energy_log_floor);
            if (lane == 0) s_P[f * KP + MH] = le;
        }
        wave_sync();
        wave_fft_half<MH>(s_f, s_tw, lane);
        float *P = s_P + f * KP;
#pragma unroll
        for (int b = 0; b < MH / 64; ++b) {
            const int k = lane + 64 * b;
            const float pw = real_split_power(s_f[k], s_f[(MH - k) & (MH - 1)], s_sp[k]);
            P[k] = p.use_power ? pw : sqrtf(pw);
        }
        wave_sync(); // (the next frame takes the buffer)
    }
    __syncthreads(); // every wave has left the span: the log mel rows may take its words

    {   // mel chains and the log, one (frame, band) per thread and trip
        const int n = rows * nb;
        const uint32_t magic = div_magic(nb);
        for (int i = tid; i < n; i += 256) {
            const int t = div_small(i, nb, magic);
            const int m = i - t * nb;
            const float acc = mel_span_chain(s_mw + s_meta[2 * nb + m], s_P + t * KP + s_meta[m], s_meta[nb + m]);
            if (OPTS) // (fbank with the energy column: it leads the bands, or under HTK follows them)
                s_x[t * xp + m + (xp > nb && !htk ? 1 : 0)] = logf(fmaxf(acc, 0x1p-23f));
            else
                s_x[i] = logf(fmaxf(acc, 0x1p-23f));
        }
        if (OPTS && xp > nb)
            for (int t = tid; t < rows; t += 256) s_x[t * xp + (htk ? nb : 0)] = s_P[t * KP + MH];
    }
    const float *s_out = s_x;
    if (C > 0) { // cepstra, one (frame, i) per thread and trip; dct_t [M][C]: a wave's reads of one band are consecutive
        __syncthreads();
        const int n = rows * C;
        const uint32_t magic = div_magic(C);
        for (int i = tid; i < n; i += 256) {
            const int t = div_small(i, C, magic);
            const int ci = i - t * C;
            const float *L = s_x + t * nb;
            float acc = 0.f;
#pragma unroll 4
            for (int m = 0; m < nb; ++m) acc = __builtin_fmaf(p.dct_t[m * C + ci], L[m], acc);
            if (OPTS) { // column 0 is the energy or c0; HTK: it goes last (c0 times sqrt 2 in double), the others move up
                if (ci == 0) acc = energy ? s_P[t * KP + MH] : htk ? (float)((double)acc * 1.4142135623730951) : acc;
                s_c[t * C + (htk ? (ci == 0 ? C - 1 : ci - 1) : ci)] = acc;
            } else {
                s_c[i] = acc;
            }
        }
        s_out = s_c;
    }
    __syncthreads();
    tile_store_rows(s_out, cols, rows, p.feat, ck.out_row, p.feat_pitch, tid);
}

// two kernels in two translation units, so that a handle without options runs the code, the registers and the three blocks per CU it always had
template <bool OPTS>
__device__ __forceinline__ void kaldi_front(const KaldiParams &p, float *smem)
{
    if (p.N == 512)
        kaldi_block<256, OPTS>(p, smem);
    else if (p.N == 256)
        kaldi_block<128, OPTS>(p, smem);
    else
        kaldi_block<64, OPTS>(p, smem);
}

} // namespace

// the launch of k_kaldi_front_opts (mfx_kaldi_opts.hip), for launch_kaldi, which has checked the arguments and sized the LDS
hipError_t launch_kaldi_opts(const KaldiParams &p, size_t lds, hipStream_t stream);

} // namespace mfx
