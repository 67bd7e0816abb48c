// mfx_stft.hip -- k_stft_mel and k_stft_post: the exact-length STFT log-mel front end (MFX_METHOD_STFT_LOGMEL) and their
// launchers.  See DESIGN.md, "STFT log-mel".
//
// Per utterance of n samples (N = DFT length, S = hop, M = bands, K1 = N / 2 + 1 bins): T = 0 when n <= N / 2, else n div S
// centred frames; frame t, tap j reads sample t S + j - N / 2, reflected at the ends of the utterance.
//   x[j]      = (float)pcm * 2^-15
//   re[k]     = 0, then for j = 0 .. N - 1 ascending: fmaf(x[j], Ck[k][j], .)        (im[k] likewise with Sk: the UNFOLDED form)
//   P[k]      = fmaf(im, im, re * re)
//   mel[m]    = 0, then over the row's non-zero span ascending: fmaf(Wm[m][k], P[k], .)
//   L         = log10(max(mel, 1e-10f)), -10.0f at the floor itself (LN: the natural log)
//   WHISPER   : L = max(L, mx - 8.0f), out = (L + 4.0f) * 0.25f, mx the utterance's largest L          (k_stft_post)
//
// k_stft_mel: a block of 4 waves takes R = 64, 32 or 16 consecutive frames of one utterance (StftChunk).  Their PCM span,
// (R - 1) S + N floats, is staged once in LDS, reflected, converted and scaled: frame t is then the contiguous run at t S
// and no frame is ever copied (k_splice_affine's staging with the row pitch Wd replaced by the hop).  The basis comes as
// v_mfma_f32_16x16x4_f32 lane operands [pass][step of 4 taps][tile of 16 outputs][64 lanes] and is streamed through two
// LDS buffers of kStftKSteps steps, chunk c + 1 travelling through registers while chunk c is consumed.  Wave w owns the 16
// frames 16 w .. 16 w + 15 and ALL output tiles of the pass: the A operand of a step is read once and serves every tile.
// Tiles come in pairs -- tile 2 q holds the cos rows, tile 2 q + 1 the sin rows of bins 16 q .. 16 q + 15 -- so re[k] and
// im[k] of a frame meet in the same lane and register of sibling accumulators and the power is formed in place.  A pass
// carries at most kStftTB bin tiles (26 accumulator tiles, 104 registers); a DFT with more bins (N > 414) takes a second
// pass over the taps for the rest -- every output still has ONE uncut chain, inside one pass.  Taps past N (N is padded to
// a multiple of 4) meet zero operands and finite staged words.  P goes to LDS, the mel chains and the log run one (frame,
// band) per thread, and the rows leave with consecutive lanes on consecutive words (tile_store_rows).  The block's largest
// log value goes to its slot of blk_max.
// k_stft_post (WHISPER only): the block of a chunk takes the maximum over the slots of its utterance's chunks -- a float
// maximum does not depend on the order, no atomics -- and clamps and maps its own rows in place.
// k_sess_stft_mel (the session entries, LOG10 / LN): the same DFT loop and mel stage (stft_dft_power below, stft_mel_log of
// mfx_stft_dev.h -- which k_stft_fft_mel, the FFT form of mfx_stft_fft.hip, shares with the span staging: one
// chain per value, tap for tap) over groups of at most 16 frames of DIFFERENT sessions per block; see its own comment.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_dev.h"
#include "mfx_launch.h"
#include "mfx_stft_dev.h"
#include "mfx_tile_dev.h"

namespace mfx {

namespace {

__host__ __device__ inline int stft_steps(int N) { return (N + 3) >> 2; }
// floats of one LDS operand buffer
__host__ __device__ inline int stft_buf_floats(int N) { return kStftKSteps * 2 * stft_pass_tiles(N) * 64; }
constexpr int kStftPad = 4; // words of zeros behind a staged span: the padded taps of its last frame
__host__ __device__ inline int stft_span_floats(int N, int S, int R) { return (R - 1) * S + N + kStftPad; } // the span and its pad
constexpr int kStftPf = (kStftKSteps * 2 * kStftTB * 16 + 255) / 256; // 16-byte words a thread carries for the next chunk

// The DFT and the power of a wave's 16 frames, shared by k_stft_mel and k_sess_stft_mel: every pass over the taps, the basis
// operands streamed through the two LDS buffers s_b for all waves of the block (every thread calls this: it synchronises the
// block, the first time once the callers' spans are staged).  Lane (li, lk) of a busy wave feeds frame li, tap 4 s + lk from
// za[4 s]; the power of the wave's frames r < wave_rows goes to s_Pw [16][KP].
__device__ __forceinline__ void stft_dft_power(const float *operands, int N, float *s_b, const float *za, bool busy, int wave_rows, float *s_Pw,
                                               int tid)
{
    const int K1 = stft_bins(N), KP = stft_p_pitch(N), NBT = stft_bin_tiles(N), TBp = stft_pass_tiles(N), steps = stft_steps(N);
    const int lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    for (int b0 = 0; b0 < NBT; b0 += TBp) {
        const int cnt = min(TBp, NBT - b0);       // bin tiles of this pass
        const int pt = 2 * TBp;                   // tiles of a pass as the table holds them (the last pass: zeros beyond cnt)
        const int chunk4 = kStftKSteps * pt * 16; // 16-byte words of a chunk
        const int total4 = steps * pt * 16;
        const int nchunks = (steps + kStftKSteps - 1) / kStftKSteps;
        const f32x4 *ops4 = (const f32x4 *)operands + (int64_t)(b0 / TBp) * total4;

        f32x4 pf[kStftPf] = {};
#pragma unroll
        for (int q = 0; q < kStftPf; ++q) {
            const int i = tid + 256 * q;
            if (i < min(chunk4, total4)) pf[q] = ops4[i];
        }
        __syncthreads(); // (the previous pass has left the buffers; the first pass: nothing reads them yet)
#pragma unroll
        for (int q = 0; q < kStftPf; ++q) {
            const int i = tid + 256 * q;
            if (i < min(chunk4, total4)) ((f32x4 *)s_b)[i] = pf[q];
        }
        __syncthreads(); // (also: the spans are staged)

        f32x4 acc[2 * kStftTB];
#pragma unroll
        for (int j = 0; j < 2 * kStftTB; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int c = 0; c < nchunks; ++c) {
            const bool more = c + 1 < nchunks;
            const int n4 = more ? min(chunk4, total4 - (c + 1) * chunk4) : 0;
#pragma unroll
            for (int q = 0; q < kStftPf; ++q) {
                const int i = tid + 256 * q;
                if (i < n4) pf[q] = ops4[(c + 1) * chunk4 + i];
            }
            if (busy) {
                const float *buf = s_b + (c & 1) * chunk4 * 4;
                const int s0 = c * kStftKSteps, s1 = min(steps, s0 + kStftKSteps);
                for (int s = s0; s < s1; ++s) {
                    const float *b = buf + (s - s0) * pt * 64 + lane;
                    const float a = za[4 * s];
#pragma unroll
                    for (int j = 0; j < kStftTB; ++j) {
                        if (j < cnt) {
                            acc[2 * j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[(2 * j) * 64], acc[2 * j], 0, 0, 0);
                            acc[2 * j + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[(2 * j + 1) * 64], acc[2 * j + 1], 0, 0, 0);
                        }
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < kStftPf; ++q) {
                const int i = tid + 256 * q;
                if (i < n4) ((f32x4 *)(s_b + ((c + 1) & 1) * chunk4 * 4))[i] = pf[q];
            }
            __syncthreads();
        }

        // D[i][n]: the lane holds frames i = 4 (lane >> 4) + r, bin n = lane & 15 of the tile -- re and im side by side
        if (busy) {
#pragma unroll
            for (int j = 0; j < kStftTB; ++j) {
                const int k = 16 * (b0 + j) + li;
                if (j >= cnt || k >= K1) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int t = 4 * lk + r;
                    const float re = acc[2 * j][r], im = acc[2 * j + 1][r];
                    if (t < wave_rows) s_Pw[t * KP + k] = __builtin_fmaf(im, im, re * re);
                }
            }
        }
    }
}

// LDS, all of it dynamic (stft_lds_bytes is the whole of what a block asks for):
//   operand buffers [2][KS][2 TBp][64] | s_x [(R - 1) S + N + 4] (later s_out [R][M]) | s_P [R][KP] | s_red [4]
__global__ void __launch_bounds__(256) k_stft_mel(StftParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const StftChunk ck = p.chunks[blockIdx.x];
    const int R = p.tile_rows, N = p.core.N, S = p.core.S, M = p.core.M;
    const int rows = ck.n_frames;
    const int KP = stft_p_pitch(N);
    const int tid = threadIdx.x;
    float *s_b = smem;
    float *s_x = s_b + 2 * stft_buf_floats(N);
    float *s_P = s_x + stft_xo_floats(N, S, M, R, kStftPad);
    float *s_red = s_P + R * KP; // the waves' maxima

    {   // the span of frames t0 .. t0 + rows - 1, reflected at the ends of the utterance; zeros behind it
        const int span = (rows - 1) * S + N, all = stft_span_floats(N, S, R);
        stft_stage_span(p.pcm, ck.utt_off, INT64_MAX, ck.utt_len, (int64_t)ck.t0 * S - N / 2, span, all, s_x, tid);
    }

    const int lane = tid & 63, g = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const bool busy = 16 * g < rows && 16 * g < R;
    const float *za = s_x + (16 * g + li) * S + lk; // lane (li, lk) feeds frame 16 g + li, tap 4 s + lk
    stft_dft_power(p.core.operands, N, s_b, za, busy, rows - 16 * g, s_P + 16 * g * KP, tid);
    __syncthreads();

    stft_finish_block(p.core, s_P, KP, rows, s_x, s_red, p.blk_max + (p.chunk_first + blockIdx.x), ck, tid);
}

__global__ void __launch_bounds__(256) k_stft_post(StftParams p)
{
    __shared__ float s_red[4];
    const StftChunk ck = p.chunks[blockIdx.x];
    const int tid = threadIdx.x;
    float mx = -INFINITY;
    for (int c = tid; c < ck.utt_chunks; c += 256) mx = fmaxf(mx, p.blk_max[ck.utt_chunk0 + c]);
    mx = wave_max(mx);
    if ((tid & 63) == 0) s_red[tid >> 6] = mx;
    __syncthreads();
    const float lo = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3])) - 8.0f;
    const int M = p.core.M, n = ck.n_frames * M;
    const uint32_t magic = div_magic(M);
    float *obase = p.core.out + ck.out_row * (int64_t)p.core.out_pitch;
    for (int i = tid; i < n; i += 256) {
        const int t = div_small(i, M, magic);
        float *o = obase + t * (int64_t)p.core.out_pitch + (i - t * M);
        *o = (fmaxf(*o, lo) + 4.0f) * 0.25f;
    }
}

// k_sess_stft_mel: the same chains over the rows one push of the session entries delivers, for many sessions at once
// ("Session log-mel").  A push is many sessions with about ten frames each, so a block does not take R consecutive
// frames of one utterance: it takes up to G = 4, 2 or 1 GROUPS (StftChunk: at most 16 consecutive frames of one session),
// wave g owning group g, stages each group's own span, 15 S + N (+ 4) floats, from the session's current slot with the
// reflections of the STREAM, and streams the basis through the two operand buffers once for all of them.
// LDS: operand buffers [2][KS][2 TBp][64] | s_x [G][15 S + N + 4] (later s_out [G][16][M]) | s_P [16 G][KP]
__global__ void __launch_bounds__(256) k_sess_stft_mel(SessStftParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int G = p.G, N = p.core.N, S = p.core.S, M = p.core.M;
    const int g0 = blockIdx.x * G, ng = min(G, p.n_groups - g0);
    const int KP = stft_p_pitch(N), xo = stft_xo_floats(N, S, M, 16, kStftPad);
    const int tid = threadIdx.x;
    float *s_b = smem;
    float *s_x = s_b + 2 * stft_buf_floats(N);
    float *s_P = s_x + G * xo;

    for (int q = 0; q < ng; ++q) { // the span of the group's frames, reflected at the ends of the stream; zeros behind it
        const StftChunk ck = p.groups[g0 + q]; // (utt_off: where stream sample 0 would lie in the slot array)
        const int rows = min(ck.n_frames, 16);
        const int span = (rows - 1) * S + N, all = stft_span_floats(N, S, 16);
        stft_stage_span(p.pcm, ck.utt_off, p.pcm_elems, ck.utt_len, (int64_t)ck.t0 * S - N / 2, span, all, s_x + q * xo, tid);
    }

    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const bool busy = wave < ng;
    const int g = busy ? wave : 0;
    const float *za = s_x + g * xo + li * S + lk; // lane (li, lk) feeds frame li of the wave's group, tap 4 s + lk
    stft_dft_power(p.core.operands, N, s_b, za, busy, busy ? min(p.groups[g0 + g].n_frames, 16) : 0, s_P + 16 * g * KP, tid);
    __syncthreads();

    for (int q = 0; q < ng; ++q) stft_mel_log(p.core, s_P + 16 * q * KP, KP, min(p.groups[g0 + q].n_frames, 16), s_x + q * xo, tid);
    __syncthreads();
    for (int q = 0; q < ng; ++q) {
        const StftChunk ck = p.groups[g0 + q];
        tile_store_rows(s_x + q * xo, M, min(ck.n_frames, 16), p.core.out, ck.out_row, p.core.out_pitch, tid);
    }
}

// a core any kernel of the method can run on: a shape inside the limits, every table and the rows in place
bool stft_core_ok(const StftCore &c)
{
    return stft_shape_ok(c.N, c.S, c.M) && c.out_pitch >= c.M && c.operands && c.mel.w && c.mel.beg && c.mel.len && c.mel.off && c.out;
}

size_t stft_matrix_lds_bytes(int N, int S, int M, int tile_rows)
{
    const size_t f = (size_t)2 * stft_buf_floats(N) + (size_t)stft_xo_floats(N, S, M, tile_rows, kStftPad) +
                     (size_t)tile_rows * stft_p_pitch(N) + 4 /* s_red */;
    return f * sizeof(float);
}

} // namespace

size_t stft_lds_bytes(int N, int S, int M, int tile_rows)
{
    return stft_form(N) == StftForm::Fft ? stft_fft_lds_bytes(N, S, M, tile_rows) : stft_matrix_lds_bytes(N, S, M, tile_rows);
}

static int stft_top_tile(int N) { return stft_form(N) == StftForm::Fft ? 16 : 64; } // the largest of the form's three tiles: 64 / 32 / 16, 16 / 8 / 4

int stft_tile_rows(int N, int S, int M)
{
    if (!stft_shape_ok(N, S, M)) return 0;
    for (int r = stft_top_tile(N); r >= stft_top_tile(N) / 4; r /= 2)
        if (stft_lds_bytes(N, S, M, r) <= kLdsMax) return r;
    return 0;
}

static bool stft_params_ok(const StftParams &p) // what launch_stft and launch_stft_post take
{
    const int top = stft_top_tile(p.core.N), R = p.tile_rows;
    return stft_core_ok(p.core) && p.pcm && p.chunks && p.blk_max && (R == top || R == top / 2 || R == top / 4) &&
           stft_lds_bytes(p.core.N, p.core.S, p.core.M, R) <= kLdsMax;
}

hipError_t launch_stft(const StftParams &p, hipStream_t stream)
{
    if (p.n_chunks <= 0) return hipSuccess;
    if (!stft_params_ok(p)) return hipErrorInvalidValue;
    const size_t lds = stft_lds_bytes(p.core.N, p.core.S, p.core.M, p.tile_rows);
    const void *fn = stft_form(p.core.N) == StftForm::Fft ? stft_fft_kernel() : (const void *)k_stft_mel;
    if (hipError_t e = allow_dynamic_lds(fn, lds); e != hipSuccess) return e;
    StftParams q = p;
    return launch_kernel(fn, dim3(p.n_chunks), dim3(256), lds, stream, q);
}

size_t sess_stft_lds_bytes(int N, int S, int M, int G)
{
    const size_t f = (size_t)2 * stft_buf_floats(N) + (size_t)G * stft_xo_floats(N, S, M, 16, kStftPad) + (size_t)16 * G * stft_p_pitch(N);
    return f * sizeof(float);
}

int sess_stft_groups(int N, int S, int M)
{
    if (stft_form(N) != StftForm::Matrix || !stft_shape_ok(N, S, M)) return 0;
    for (int g : {4, 2, 1})
        if (sess_stft_lds_bytes(N, S, M, g) <= kLdsMax) return g;
    return 0;
}

hipError_t launch_sess_stft(const SessStftParams &p, hipStream_t stream)
{
    if (p.n_groups <= 0) return hipSuccess;
    if (!stft_core_ok(p.core) || !p.pcm || p.pcm_elems <= 0 || !p.groups) return hipErrorInvalidValue;
    const int G = sess_stft_groups(p.core.N, p.core.S, p.core.M);
    if (G == 0 || p.G != G) return hipErrorInvalidValue; // (another form, or the caller sized its lists for another packing)
    const size_t lds = sess_stft_lds_bytes(p.core.N, p.core.S, p.core.M, G);
    const void *fn = (const void *)k_sess_stft_mel;
    if (hipError_t e = allow_dynamic_lds(fn, lds); e != hipSuccess) return e;
    SessStftParams q = p;
    return launch_kernel(fn, dim3((p.n_groups + G - 1) / G), dim3(256), lds, stream, q);
}

hipError_t launch_stft_post(const StftParams &p, hipStream_t stream)
{
    if (p.n_chunks <= 0) return hipSuccess;
    if (!stft_params_ok(p)) return hipErrorInvalidValue;
    StftParams q = p;
    return launch_kernel((const void *)k_stft_post, dim3(p.n_chunks), dim3(256), 0, stream, q);
}

} // namespace mfx
