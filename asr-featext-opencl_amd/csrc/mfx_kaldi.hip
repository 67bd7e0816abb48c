// mfx_kaldi.hip -- k_kaldi_front: the Kaldi-compatible fbank / MFCC front end (MFX_METHOD_KALDI; include/mfx.h states the
// definition, DESIGN.md section 5 "Kaldi front end" the structure), and its launcher.  The block body is mfx_kaldi_dev.h, which
// mfx_kaldi_opts.hip builds once more as k_kaldi_front_opts for handles with kaldi_flags of mfx_create_kaldi != 0.
//
// A block of 4 waves takes one Chunk: at most kChunkFrames = 16 consecutive frames of one utterance (or of a session's slot).
// Their PCM span, (rows - 1) S + W samples, is staged once in LDS as floats (exact: int16); the window (zero padded to N), the
// twiddles W_M^k (M = N / 2) and the real split's factors -i W_N^k are kept once per block in LDS.  No sample outside the span
// is read: a frame's first sample stands for its predecessor.  Wave w takes frames w, w + 4, ... of the chunk, one after the
// other, in its own buffer of M complex points:
//   - the exact integer sum of the frame's W samples by a wave reduction (shuffles), mean = (float)s / (float)W;
//   - d = x - mean, e[i] = fmaf(-c, d[i - 1], d[i]), z = e * w as M complex points (z[2 n], z[2 n + 1]), zero from tap W on;
//   - a complex FFT of M = 64, 128 or 256 points, Stockham autosort, radix 4 (M = 128: three stages, then one of radix 2):
//     wave_fft_half of mfx_wavefft_dev.h, the stages k_stft_fft_mel runs, here with one butterfly per lane, lanes beyond M / 4
//     idle.  A stage reads all of its inputs into registers before it writes any output, so one buffer serves, and only the
//     wave synchronises;
//   - the real split (real_split_power of the same header) for bins k < M (the Nyquist bin has no mel weight) and the power, or
//     its root, into s_P [frame][KP].
// The float32 operations a frame sees are those of this one instruction stream: they depend on N alone, not on the chunk, the
// wave, the frame's place in its block, the batch or the entry.  After a block barrier the mel chains and the log run one
// (frame, band) per thread into the span's words -- every wave has left the span by then --, the cepstra one (frame, i) per
// thread, and the rows leave through tile_store_rows.  The mel table (at most N weights: a bin lies in two bands at most) and
// its spans are staged in LDS with the window: a chain's reads are LDS reads, not dependent trips to L2.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_dev.h"
#include "mfx_launch.h"
#include "mfx_tile_dev.h"
#include "mfx_kaldi_dev.h"

namespace mfx {

namespace {

__global__ void __launch_bounds__(256) k_kaldi_front(KaldiParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    kaldi_front<false>(p, smem);
}

} // namespace

size_t kaldi_lds_bytes(int W, int S, int M, int C, int flags)
{
    const int N = kaldi_fft_size(W);
    // (fbank with the energy column assembles rows of M + 1 floats in the span's words)
    const size_t f = (size_t)kaldi_xo_floats(W, S, C > 0 ? M : kaldi_static_cols(M, C, flags)) + kaldi_c_floats(C) + (size_t)3 * N /* window, twiddles, split */ +
                     (size_t)4 * N /* FFT buffers: 4 waves of N / 2 complex points */ + (size_t)N + kaldi_meta_words(M) /* mel table */ +
                     (size_t)kKaldiRows * kaldi_p_pitch(N);
    return f * sizeof(float);
}

hipError_t launch_kaldi(const KaldiParams &p, hipStream_t stream)
{
    if (p.n_chunks <= 0) return hipSuccess;
    if (!kaldi_shape_ok(p.W, p.S, p.M, p.C) || p.N != kaldi_fft_size(p.W) || !p.pcm || !p.chunks || !p.operands || !p.mel.w || !p.mel.beg ||
        !p.mel.len || !p.mel.off || p.mel_w_floats < 1 || p.mel_w_floats > p.N || (p.C > 0 && !p.dct_t) || !p.feat || !kaldi_flags_ok(p.flags) ||
        p.feat_pitch < kaldi_static_cols(p.M, p.C, p.flags) || ((p.flags & kKaldiNoSnipEdges) && (!p.utt_bounds || p.n_utt <= 0)))
        return hipErrorInvalidValue;
    const size_t lds = kaldi_lds_bytes(p.W, p.S, p.M, p.C, p.flags);
    if (lds > kLdsMax) return hipErrorInvalidValue;
    if (p.flags != 0) return launch_kaldi_opts(p, lds, stream);
    const void *fn = (const void *)k_kaldi_front;
    if (hipError_t e = allow_dynamic_lds(fn, lds); e != hipSuccess) return e;
    KaldiParams q = p;
    return launch_kernel(fn, dim3(p.n_chunks), dim3(256), lds, stream, q);
}

} // namespace mfx
