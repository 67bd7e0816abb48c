// mfx_tables.h -- host-side construction of the constant tables the HIP kernels consume.
//
// The tables are *data* of the feature extractor, defined by the reference's CPU back end; they
// are built once per handle (the mel table again on every set_alpha change) in the reference's
// float32 expression order and uploaded to HBM.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mfx {

// Smallest power of two >= v (reference: ceil2, mfcccpu.cpp:10-20).
uint32_t ceil_pow2(uint32_t v);

// Frames that fit in `samples` samples: floor((samples - (W - S)) / S), integer arithmetic.
// Equals ParamBase::estimated_window_count (parambase.cpp:16-19) wherever that float32
// expression is exact (samples < 2^24).
int64_t frame_count(int64_t samples, int window_size, int shift);

// One push of one session of the session entries ("Session entries"): a stream that has received n samples per
// channel and delivered rows [0, E) takes `length` more.  T(n) = max(0, frame_count(n)); E = max(0, T - D) while the
// stream is open, T once a push is final.  The previous slot carries the samples from the first frame not yet computed,
// [T * S, n), and the static rows of frames [f0, T), f0 = max(0, E - D); the push computes frames [T_old, T_new) behind
// them and delivers rows [E_old, E_new) through the delta Segment (n_out, shift, lo, hi, static_off), rows relative to
// frame f0.  Returns n_out; n and E are advanced (both 0 after a final push: the session is fresh).
struct SessionStep {
    int64_t carry_samples; // samples per channel carried in
    int32_t carry_rows;    // static rows carried in
    int32_t new_frames;    // frames the push computes
    int32_t n_out, shift, lo, hi, static_off;
};
int32_t session_step(int window_size, int shift, int D, int64_t &n, int64_t &E, int64_t length, bool final_push, SessionStep &st);

// The session transform's step ("Session transform"): a session whose rows y[0, Ey) are complete (Ey is the E of
// session_step) and which has delivered transformed rows [0, Ex) completes n_y more rows.  Ex = max(0, Ey - right) while the
// stream is open, Ey once a push is final.  The previous y slot carries rows [c0, Ey), c0 = max(0, Ex - left) -- at most left +
// right of them -- and the push writes the n_y new rows behind them: row 0 of the current slot is y[c0].  The push delivers
// rows [Ex_old, Ex_new) through k_splice_affine's accessor src[src_row0 + clamp(r - left + c, lo, hi)], r relative to Ex_old:
// src_row0 = Ex_old - c0 is the slot row of y[Ex_old], lo = -src_row0 (y[c0]: reached only when c0 = 0, the true start of the
// stream) and hi = Ey_new - 1 - Ex_old (reached only by a final push).  Returns n_out; Ey and Ex are advanced (both 0 after a
// final push).
struct SessionXformStep {
    int32_t n_out;      // rows delivered
    int32_t carry_rows; // rows y carried in
    int32_t src_row0, lo, hi;
};
int32_t session_xform_step(int left, int right, int64_t &Ey, int64_t &Ex, int32_t n_y, bool final_push, SessionXformStep &st);

// The work list of k_sess_xform for one push: piece i delivers n_out[i] rows with transform xf[i].  Every piece is cut into
// row groups of at most 16 rows; the groups are sorted by transform (stable: pieces keep their order inside a transform) and
// packed into blocks of at most G consecutive groups of one transform.
struct SessXfCut {
    int32_t piece, r0, rows; // the group: rows [r0, r0 + rows) of the piece
};
struct SessXfPack {
    int32_t g0, ng, xf;      // the block: groups [g0, g0 + ng), their transform
};
void pack_sess_xform_groups(const int32_t *n_out, const int32_t *xf, int n, int G, std::vector<SessXfCut> &groups, std::vector<SessXfPack> &blocks);

// The reference's float32 version, bit-for-bit (used by the streaming state machine).
int estimated_window_count_f32(int samples, int window_size, int shift);

struct MelTable {
    std::vector<float> weights;   // [2][fft_size]: row 0 even-numbered filters, row 1 odd-numbered
    std::vector<int32_t> beg;     // [num_banks + 2] first bin of filter i (= rounded centre i)
};

// Triangular mel filterbank with optional VTLN bilinear warp (reference: MfccCpu::refresh_filters,
// mfcccpu.cpp:24-60).  Filter m covers bins [beg[m], beg[m+2]) of weights[m % 2].
void build_mel_table(int num_banks, int fft_size, float sample_rate, float low_freq, float high_freq,
                     float alpha, MelTable &out);

// DCT-II with sinusoidal lifter, c0 (if wanted) as the LAST column
// (reference: mfcccpu.cpp:118-136).  Row-major [num_banks][dct_len].
void build_dct_matrix(int num_banks, int ceps_len, bool want_c0, float lift_coef, std::vector<float> &out);

// PLP tables (PLP), evaluated in double and rounded once to float:
//   eql  [num_banks]: equal-loudness weight e_m = (q / (q + 1.6e5))^2 (q + 1.44e6) / (q + 9.61e6), q = f_m^2, f_m the
//        (warped) centre of filter m in Hz
//   idft [lpc_order + 1][num_banks + 2]: r_i = sum_m idft[i][m] A_m, idft[i][m] = w_m cos(pi i m / (N - 1)) / (2 (N - 1)),
//        N = num_banks + 2, w_m = 1 at both ends, 2 elsewhere
void build_plp_tables(int num_banks, float sample_rate, float low_freq, float high_freq, float alpha, int lpc_order,
                      std::vector<float> &eql, std::vector<float> &idft);
// lifter weights w_1 .. w_C of the PLP cepstra: the float32 expression of build_dct_matrix
void build_plp_lifter(int ceps_len, float lift_coef, std::vector<float> &out);

// TRAPS (TRAPS): basis [K][L] of the trajectory transform, evaluated in double and rounded once to float:
//   B[k][j] = (0.54 - 0.46 cos(2 pi j / (L - 1))) sqrt(2 / L) cos(pi k (j + 1/2) / L)
// i.e. a Hamming window over the L frames times the DCT-II in build_dct_matrix's convention (k = 0: the windowed mean,
// scaled like the c0 column).
void build_traps_basis(int traps_len, int traps_dct_len, std::vector<float> &out);
// k_traps on the matrix pipe (v_mfma_f32_16x16x4_f32): B operands for every tile of 16 coefficients and every step of 4
// taps, out[(tile * steps + s) * 64 + lane] = B[16 tile + (lane & 15)][4 s + (lane >> 4)], zero beyond the basis.
// tiles = ceil(K / 16), steps = ceil(L / 4).
void build_traps_mfma_operands(const std::vector<float> &basis, int traps_len, int traps_dct_len, int &tiles, int &steps,
                               std::vector<float> &out);
// k_traps on the vector ALUs: the basis transposed, [L][kp], kp = K padded to 4, 16 or 32 accumulators (zero beyond K)
void build_traps_valu_operands(const std::vector<float> &basis, int traps_len, int traps_dct_len, int &kp, std::vector<float> &out);

// k_splice_affine ("Splice + affine transform"): one transform's matrix A, row-major [out_dim][in_dim], as the
// kernel streams it -- for every step of 4 taps and every tile of 16 outputs the 64 lanes' operands of
// v_mfma_f32_16x16x4_f32: out[(s * tiles + tile) * 64 + lane] = A[16 tile + (lane & 15)][4 s + (lane >> 4)], zero beyond
// the matrix.  tiles = ceil(out_dim / 16), steps = ceil(in_dim / 4).  `out` must hold steps * tiles * 64 floats.
void build_xform_operands(const float *A, int out_dim, int in_dim, int &tiles, int &steps, float *out);

// Per-utterance warp factors of a planned batch (mfx_batch_set_alphas) -> what the row-run kernels read.  Utterance u holds
// the rows [sum of frames[0 .. u), + frames[u]).
//   tables: the distinct factors, compared bit for bit, in order of first appearance
//   off   : [tables + 1] table a owns runs [off[a], off[a + 1])
//   runs  : [n][2] (first row, rows); a table's runs ascend; utterances without frames leave none, neighbours (with nothing
//           but frameless utterances between them) of the same factor are one run
void build_alpha_runs(const float *alphas, const int64_t *frames, int n_utt, std::vector<float> &tables, std::vector<int32_t> &off,
                      std::vector<int64_t> &runs);
// the same lists with every run clipped to the rows [row0, row0 + rows), as the kernels clip them; empty runs dropped
void clip_alpha_runs(int64_t row0, int64_t rows, std::vector<int32_t> &off, std::vector<int64_t> &runs);

// Speakers of a planned batch (mfx_batch_set_speakers) -> the lists k_spk_finish walks.  utt_spk[u] in [0, n_spk) is the speaker of
// utterance u (false when one is outside: nothing is written then); frames[u] its row count.
//   off  : [n_spk + 1] speaker s owns list[off[s] .. off[s + 1])
//   list : its utterances in ascending utterance index; utterances without frames are left out
bool build_speaker_lists(const int32_t *utt_spk, const int64_t *frames, int n_utt, int n_spk, std::vector<int32_t> &off,
                         std::vector<int32_t> &list);

// The online normaliser (mfx_batch_set_online_norm) on host memory, exactly as include/mfx.h defines it: rows [T][pitch],
// columns [0, Wn) -> out [T][Wn].  kind: 1 CMN, 2 CVN.  False -- and nothing written -- on an argument outside the limits.
bool host_online_norm(const float *rows, int64_t T, int pitch, int Wn, int kind, int window, int prior_frames, int64_t prior_count,
                      const double *prior_acc, float *out);

// The sliding-window normaliser (mfx_batch_set_sliding_norm): the window [ws, we) of row t of an utterance of T rows, Kaldi's
// SlidingWindowCmn rule as include/mfx.h restates it.  One definition for the host restatement and k_slide_apply.
// 0 <= t < T, window >= 1, 0 <= min_window: then 0 <= ws <= t < we <= T.
#if defined(__HIP__)
#define MFX_HOST_DEVICE __host__ __device__
#else
#define MFX_HOST_DEVICE
#endif
// (I: int64_t on the host; int in the kernel: T + window must fit, and its utterances hold fewer than 2^31 - 4096 rows)
template <class I>
MFX_HOST_DEVICE inline void slide_window(I T, int window, int min_window, bool center, I t, I &ws, I &we)
{
    if (center) {
        ws = t - window / 2;
        we = ws + window;
    } else {
        ws = t - window;
        we = t + 1;
    }
    if (ws < 0) {
        we -= ws;
        ws = 0;
    }
    if (!center) we = t + 1 > (I)min_window ? t + 1 : (I)min_window;
    if (we > T) {
        ws -= we - T;
        we = T;
        if (ws < 0) ws = 0;
    }
}
#undef MFX_HOST_DEVICE
// The definition on host memory: rows [T][pitch], columns [0, W) -> out [T][out_pitch].  False -- and nothing written -- on an
// argument outside the limits of include/mfx.h.
bool host_sliding_norm(const float *rows, int64_t T, int W, int pitch, int window, int min_window, int center, int norm_vars, float *out,
                       int out_pitch);

// Utterance tilings ("Utterance tilings"): the rows of every utterance of a planned batch cut into items of `rows`
// consecutive rows (the last one of an utterance may be shorter), numbered through the batch in utterance order.
//   item0    : [n_utt + 1] first item of every utterance (a frameless utterance owns none)
//   item_utt : [items] the utterance of every item; may be null (the speakers' chunks: their kernels take the utterance from the grid)
// False -- and nothing written -- on n_utt < 0, rows < 1, a negative frame count or more than 0x7ffffff0 items.
bool build_utt_tiling(const int64_t *frames, int n_utt, int rows, std::vector<int32_t> &item0, std::vector<int32_t> *item_utt);
// The item sizes the kernels are compiled for: one definition each, for the host that builds a tiling and the kernel that
// walks it (the launchers refuse a tiling of another size).  The pitch track's tile_frames is the one run-time size.
constexpr int kVadTileRows = 64;     // k_vad_flags, k_vad_scan, k_vad_select: a wave's ballot is a tile's mask
constexpr int kNormChunkRows = 4096; // a run of rows longer than this is summed in chunks, combined in ascending order (normaliser, speakers, VAD)
constexpr int kOnormChunk = 32;      // rows of a chunk of the online normaliser's prefix sums (the window is a multiple of it)
constexpr int kPitchFeatRows = 256;  // rows per tile of k_pitch_feats = threads per block

// Pitch track (mfx_batch_set_pitch; DESIGN.md, "Pitch track").  pitch_shape: the limits of include/mfx.h on the seven
// parameters (window as resolved: never 0); fills K = lag_max - lag_min + 1 states and the resolved jump J.  False outside them.
struct PitchShape {
    int window, lag_min, lag_max, K, J;
};
bool pitch_shape(int window, int lag_min, int lag_max, float ballast, float lag_cost, float penalty, int max_jump, PitchShape &s);
// wt[k] = (float)(1 - lag_cost * l / lag_max), lg[k] = (float)ln(l), l = lag_min + k: double, rounded once
void build_pitch_tables(const PitchShape &s, float lag_cost, std::vector<float> &wt, std::vector<float> &lg);
// k_pitch_nccf's tiles: the utterance tiling at pitch_tile_frames frames (at most 64, fewer while the tile's PCM span would
// pass kPitchSpanMax staged samples).
// pitch_span_pad: int16 slots left empty behind every `shift` staged samples, so that the frames of a tile start on
// different LDS banks; pitch_span_slots: the slots the span of `frames` frames takes with them.
constexpr int kPitchSpanMax = 24576;
int pitch_span_pad(int shift);
int pitch_span_slots(int window, int lag_max, int shift, int frames);
int pitch_tile_frames(int window, int lag_max, int shift);
// The definition of include/mfx.h on host memory, for ONE utterance of n samples per channel and T frames at `shift`:
// pitch [T][2] = (lag, rho), index [T], nccf [T][K]; any of them may be null.  False -- and nothing written -- on an argument
// outside the limits.
bool host_pitch(const int16_t *pcm, int64_t n, int channels, int64_t T, int shift, int window, int lag_min, int lag_max, float ballast,
                float lag_cost, float penalty, int max_jump, float *pitch, int32_t *index, float *nccf);

// Pitch features (mfx_batch_set_pitch_feats; DESIGN.md, "Pitch features").  pitch_feat_shape: the limits of include/mfx.h on
// the eight parameters; fills the resolved column bits (0 -> POV | NORM_LOG_PITCH | DELTA), their number F and
// den = 2 sum of l^2 over l = 1 .. D.  False outside them.  k_pitch_feats' tiles are the utterance tiling at kPitchFeatRows.
struct PitchFeatShape {
    int columns, F, left, right, D;
    double den;
};
bool pitch_feat_shape(int columns, int left, int right, int delta_window, float pov_scale, float pov_offset, float pitch_scale,
                      float delta_scale, PitchFeatShape &s);
// The definition of include/mfx.h on host memory, for ONE utterance of T rows: pitch [T][2] = (lag, rho) -> feats [T][F].
// False -- and nothing written -- on an argument outside the limits.
bool host_pitch_feats(const float *pitch, int64_t T, float sample_rate, int columns, int left, int right, int delta_window,
                      float pov_scale, float pov_offset, float pitch_scale, float delta_scale, float *feats);

// Dense padded tensor output (mfx_batch_set_tensor; DESIGN.md, "Tensor output").  Layouts and element types are the MFX_TENSOR_*
// and MFX_DTYPE_* values of include/mfx.h.
#ifndef MFX_TENSOR_TILE_ROWS // (a dev build may pass -DMFX_TENSOR_TILE_ROWS=128 to measure the other size)
#define MFX_TENSOR_TILE_ROWS 64
#endif
constexpr int kTensorTileRows = MFX_TENSOR_TILE_ROWS; // rows t of one utterance per block of k_tensor_pack: 64 or 128
constexpr int kTensorTimeMajor = 0, kTensorChannelMajor = 1;
constexpr int kDtypeF32 = 0, kDtypeF16 = 1, kDtypeBf16 = 2;
constexpr int kTensorPadMax = 1 << 24; // largest t_pad
inline int tensor_elem_bytes(int dtype) { return dtype == kDtypeF32 ? 4 : 2; }
// LDS bytes of a block of k_tensor_pack: the CHANNEL_MAJOR image of kTensorTileRows rows at the odd pitch Wo | 1 dwords
// (TIME_MAJOR uses none)
inline size_t tensor_lds_bytes(int Wo) { return (size_t)kTensorTileRows * (size_t)(Wo | 1) * sizeof(float); }
// bytes of the tensor [B][Tp][Wo]; -1 on a negative size, an unknown dtype, Tp > kTensorPadMax or a product beyond int64
int64_t tensor_bytes(int64_t B, int64_t Wo, int64_t Tp, int dtype);
// float32 -> IEEE binary16 / bfloat16 bits, roundTiesToEven in integer arithmetic: overflow to inf, subnormals produced, the sign
// of zero kept, a NaN stays a NaN (quiet, the payload's top bits)
uint16_t f32_to_f16_bits(uint32_t u);
uint16_t f32_to_bf16_bits(uint32_t u);
// The definition of include/mfx.h on host memory: rows [.][Wo] with utterance u's rows from out_rows[u] on, lengths[u] = L_u
// (any value >= 0: cut at Tp) -> the tensor at `out`, tensor_bytes of it, every element written.  False -- and nothing written
// -- on an argument outside the limits.
bool tensor_pack_host(const float *rows, const int64_t *out_rows, const int32_t *lengths, int64_t B, int Wo, int64_t Tp, int layout,
                      int dtype, float pad, void *out);

// exp(-2*pi*i*k/n) for k in [0, count), evaluated in double and rounded once to float.
void build_twiddles(int n, int count, std::vector<float> &re_im_interleaved);

// Split twiddles -i W_WS^k = (wi, -wr), k <= WS / 2, of the real-input split (every front end; k_front512 stages the first
// 128).  WS = fft_size, or 512 in the zero-stuffed forms (256 / 128 / 64 points on k_front512), which run the 512-POINT
// transform and its split: the kernel stages W_512^k for k < 128 whatever fft_size is.  (Until round 4 this table had
// fft_size / 2 + 1 entries: at 128 and 64 points the kernel read 63 / 95 entries past its end.  The split's difference
// term is rounding noise there, so fresh -- zero -- memory hid it; stale memory with large values did not: found by
// tools/fuzz_all.py, seed 3 case 17.)
void build_split_twiddles(int fft_size, bool stuffed, std::vector<float> &out);

// k_front_reg (fft_size >= 1024): per-pass twiddle tables laid out [k][butterfly] so that the lanes of one LDS read touch
// consecutive words.  M = fft_size / 2, R1 = 8 at 1024 points, else 16.  Pass 1 (radix R1 over M points): W_M^(pp k),
// pp < M / R1; pass 2 (radix R1 over M / R1 points): W_M^(pp k R1), pp < M / R1^2; k = 1 .. R1 - 1 in both.  Same values as
// build_twiddles(M, M).
void build_reg_pass_twiddles(int fft_size, std::vector<float> &out);

// k_front512 / k_front1024: out[l * 16 + k] = W_256^(l k), l, k < 16.
void build_pass256_twiddles(std::vector<float> &out);

// Window layouts of the register front ends.  `padded`: the window zero-padded to fft_size taps.  Every layout carries the
// output scale 0.5 / fft_size (1/2 of the real split, 1 / fft_size of mfcccpu.cpp:203): a power of two, so scaling the taps
// instead of the magnitudes changes no bit of the result and saves a multiply per bin.
//
// k_front512, and k_front1024 with a window of at most 512 samples: out[l * 16 + m] = (w[2 n], w[2 n + 1]) * scale,
// n = l + 16 m.  Zero-stuffed forms (fft_size < 512): packed sample n = (x[n / step], 0) where step = 256 / fft_size
// divides n, else (0, 0), so out[l * 16 + m] = (w[n / step] * scale, 0) or zero.
void build_window_pairs(const std::vector<float> &padded, int fft_size, bool stuffed, std::vector<float> &out);

// Phase O of k_front1024 (window <= 512 samples): (taps of pair n) x W_512^n as the real 2 x 2 form
//   re = A x0 + B x1,  im = C x0 + D x1,   (A, B, C, D) = (t0 c, -t1 s, t0 s, t1 c),  W_512^n = c + i s
// out[l * 16 + m] = (A, B, C, D) of n = l + 16 m.
void build_front1024_phase_o(const std::vector<float> &padded, int fft_size, std::vector<float> &out);

// k_front1024, window longer than 512 samples: the taps of all 32 rows of sample pairs, taps[l * 32 + m] = (w[2 n],
// w[2 n + 1]) * scale, n = l + 16 m, m < 32, and the twiddles of the first 16 rows, tw[l * 16 + m] = W_512^n, m < 16; the
// kernel folds the frame's halves itself.
void build_front1024_long_window(const std::vector<float> &padded, int fft_size, std::vector<float> &taps, std::vector<float> &tw);

// Sample-rate conversion ("Sample-rate conversion"): in_hz -> out_hz by the rational factor L / M, L = out_hz / g,
// M = in_hz / g, g = gcd.  Filter: Hann-windowed sinc, c = rolloff min(1, L / M), Wh = ceil(zeros / c), P = 2 Wh taps per
// phase.  zeros == 0 means 6, rolloff == 0 means 0.99.  resample_shape returns 0, or a negative number naming the limit that
// refuses the pair: -1 a rate outside 1000 .. 768000 Hz, -2 zeros outside 1 .. 64, -3 rolloff outside (0, 1], -4 L > 4096,
// -5 P > 4096, -6 L P > 2^20.
struct ResampleShape {
    int32_t L = 1, M = 1, P = 0, Wh = 0;
    double c = 0; // cutoff as a fraction of the input Nyquist band
};
int resample_shape(int32_t in_hz, int32_t out_hz, int32_t zeros, float rolloff, ResampleShape &s);
// taps [L][P]: h[phi][k] = c sinc(c t) (1 + cos(pi t / Wh)) / 2 for |t| < Wh, else 0, t = (k - Wh + 1) - phi / L;
// evaluated in double, rounded once to float.  No per-phase renormalisation.
void build_resample_taps(const ResampleShape &s, float *taps);
// ceil(samples L / M) in int64 arithmetic (samples >= 0 and samples L < 2^63; in_hz == out_hz: samples)
int64_t resampled_length(int64_t samples, int32_t in_hz, int32_t out_hz);
// the converted PCM's layout: utterance u holds resampled_length(lengths[u]) samples per channel from offsets[u]; starts are
// even and ascend in utterance order with nothing between utterances but the one pad sample behind an odd length.  Returns
// the total (even), or -1 on a negative length or a rate outside the limits.
int64_t resample_layout(int32_t n_utt, const int64_t *lengths, const int32_t *rates_hz, int32_t out_hz, int64_t *offsets,
                        int64_t *out_lengths);

// What the two converters (k_resample, k_sess_resample) are told about one input rate: its table and its tile geometry.
struct ResRate {
    int64_t taps_off;   // first float of the rate's table [L][P] inside the launch's taps
    int32_t L, M, P, Wh;
    int32_t R;          // same-phase outputs a work item carries (1, 2 or 4)
    int32_t items;      // work items of a full tile; a multiple of L when R > 1: outputs w + r items, r < R, share a phase
    int32_t tile_out;   // R * items, even
    int32_t in_lds;     // the table is staged in LDS (row stride P + 1), else read through the caches
};
// The three parts of a converter launch's LDS, each the maximum over the rates it serves
struct ResLds {
    int32_t taps_floats; // floats of the table part (0: no rate stages its table)
    int32_t x_floats;    // floats per channel of the staged input span (a multiple of 8)
    int32_t out_elems;   // int16 elements of the output staging (even)
};
constexpr int kResCopyTile = 4096; // samples per channel of a tile of a same-rate utterance / pass-through piece
inline size_t resample_lds_bytes(int channels, const ResLds &l)
{
    return ((size_t)l.taps_floats + (size_t)(channels == 2 ? 2 : 1) * l.x_floats) * sizeof(float) + (size_t)l.out_elems * sizeof(int16_t);
}
// Tile geometry of one rate (fills R, items, tile_out, in_lds from L, M, P), and the LDS floats per channel its span needs
void resample_geometry(int channels, ResRate &r);
int resample_span_floats(const ResRate &r);
// Everything a plan or a session set derives from its input rates, in the order given: tables (concatenated; four zeros when no
// rate converts, so that the buffer is never empty), geometry, the LDS maxima, and for the sessions the carry slot's samples
// per channel (max over rates of 2 Wh + M div L + 2, a multiple of 8) and the smallest tile.  A rate equal to out_hz has no
// table: tile_out == 0 marks the copy; check_same_rate says whether resample_shape judges zeros and rolloff for it too
// (mfx_sessions_set_rates does, mfx_batch_plan_rates does not).  Returns 0, or the index into kResampleWhy of the refusal.
struct ResRateSet {
    std::vector<ResRate> rates;
    std::vector<float> taps;
    ResLds lds;
    int32_t carry_cap, tile_min;
};
extern const char *const kResampleWhy[7];
int build_resample_rates(int channels, int32_t out_hz, const int32_t *in_hz, int n_rates, int32_t zeros, float rolloff, bool check_same_rate,
                         ResRateSet &set);

// One push of one session under a session rate ("Session sample-rate conversion"): a stream that has received N
// input samples per channel and holds converted samples [0, J) takes `length` more.  J = max(0, ceil((N - Wh) L / M)) while the
// stream is open -- the outputs whose last tap n + Wh has arrived -- and ceil(N L / M) once a push is final; a pass-through
// rate (L == M) has J = N and carries nothing.  The previous carry slot holds input samples [c0_old, N_old), c0 = max(0, (J M)
// div L - Wh + 1) (the first sample output J reads); the push converts outputs [J_old, J_new) from them and the new samples
// and leaves [c0_new, N_new) in the current slot: at most 2 Wh - 1 samples, nothing after a final push.  Returns J_new - J_old;
// N and J are advanced (both 0 after a final push: the session is fresh).
struct SessionResampleStep {
    int64_t c0_old, c0_new; // first input sample the previous / the current carry slot holds
    int32_t carry_in, carry_out; // samples per channel carried in and out
};
int64_t session_resample_step(int32_t L, int32_t M, int32_t Wh, int64_t &N, int64_t &J, int64_t length, bool final_push,
                              SessionResampleStep &st);

// STFT log-mel front end ("STFT log-mel"; N = DFT length, even; K1 = N / 2 + 1 bins).
// The DFT lengths the method takes and the kernel form each one gets -- THE rule, host and device: even lengths 32 .. 512 run on
// the matrix pipe (k_stft_mel, k_sess_stft_mel), 1024 and 2048 as a float32 FFT (k_stft_fft_mel, batch entries only)
enum class StftForm { None, Matrix, Fft };
constexpr StftForm stft_form(int N) { return N >= 32 && N <= 512 && !(N & 1) ? StftForm::Matrix : N == 1024 || N == 2048 ? StftForm::Fft : StftForm::None; }
// the limits of a shape: a DFT length of either form, hop 1 .. N, 1 .. 128 bands
constexpr bool stft_shape_ok(int N, int S, int M) { return stft_form(N) != StftForm::None && S >= 1 && S <= N && M >= 1 && M <= 128; }
constexpr int kStftTB = 13; // bin tiles (16 bins: a cos and a sin accumulator tile) a wave carries through one pass over the taps
constexpr int stft_bin_tiles(int N) { return (N / 2 + 1 + 15) >> 4; }
// bin tiles of a pass of the matrix form: as many as the DFT has, at most kStftTB (the operand table is laid out for it)
constexpr int stft_pass_tiles(int N) { return stft_bin_tiles(N) < kStftTB ? stft_bin_tiles(N) : kStftTB; }
// frames of an utterance of `samples` samples: 0 up to N / 2 samples (the reflection needs one more), else samples div S
int64_t stft_frame_count(int64_t samples, int N, int S);
// basis [2][K1][N]: Ck[k][j] = w[j] cos(2 pi ((k j) mod N) / N), Sk[k][j] = -w[j] sin(same), in double from the float32
// window, rounded once
void build_stft_basis(int N, const float *window, float *cos_sin);
// Slaney mel table (librosa filters.mel(htk=False, norm="slaney")), in double, rounded once: weights [M][K1]; beg / len: the
// non-zero span of every row (len 0: a band narrower than a bin that holds none)
void build_slaney_mel(int M, int N, float sample_rate, float low_freq, float high_freq, float *weights, int32_t *beg, int32_t *len);
// the basis as k_stft_mel streams it: passes of `tb` bin tiles (16 bins: tile 2 q of a pass the cos rows, tile 2 q + 1 the
// sin rows); out[((pass * steps + s) * 2 tb + tile) * 64 + lane] = row(16 bin tile + (lane & 15))[4 s + (lane >> 4)], zero
// beyond the bins and the taps.  steps = ceil(N / 4), passes = ceil(ceil(K1 / 16) / tb).
void build_stft_operands(const float *cos_sin, int N, int tb, std::vector<float> &out);
// FFT form (N = 1024 / 2048, M = N / 2; DESIGN.md, "STFT log-mel, FFT form"), in double, rounded once:
// twid [M] complex: W_M^k = e^(-2 pi i k / M), the twiddles of the half-length complex FFT; split [M + 1] complex: -i W_N^k, the
// real split's factors (2 X[k] = (Z[k] + conj Z[M - k]) + split[k] (Z[k] - conj Z[M - k]))
void build_stft_fft_tables(int N, float *twid, float *split);
// What the FFT kernels of two methods take as their operands, in double, rounded once: the window's W taps zero padded to N | W_M^k, k
// < M = N / 2, complex | the first n_split factors -i W_N^k, complex: 2 N + 2 n_split floats
void build_fft_operands(int W, int N, int n_split, const float *window, std::vector<float> &out);
// k_stft_fft_mel's (W = N, every bin k <= M): window [N] | twid [2 M] | split [2 (M + 1)], 3 N + 2 floats
void build_stft_fft_operands(int N, const float *window, std::vector<float> &out);
// what mfx_set_window uploads for a handle of `form`: the basis of `window` in stft_pass_tiles(N)-tile passes
// (build_stft_basis, build_stft_operands), or the FFT form's operands
void build_stft_form_operands(StftForm form, int N, const float *window, std::vector<float> &out);
// A dense mel table [M][row_width] whose rows' non-zero spans stand in meta [0, M) (first bin) and [M, 2 M) (bins), as the kernels
// read it (MelSpans): the spans back to back in `w` (one zero when every row is empty: the buffer is never empty) and every row's
// first weight in meta [2 M, 3 M)
void pack_mel_spans(const float *dense, int M, int row_width, std::vector<float> &w, std::vector<int32_t> &meta);
// the Slaney table packed so; meta [3][M]: first bin, bins, first weight of every row
void build_slaney_spans(int M, int N, float sample_rate, float low_freq, float high_freq, std::vector<float> &w, std::vector<int32_t> &meta);

// Kaldi front end (MFX_METHOD_KALDI; include/mfx.h states the definition; DESIGN.md section 5, "Kaldi front end").
// The DFT length of a window of W samples: the next power of two, 128 at least
constexpr int kaldi_fft_size(int W) { return W <= 128 ? 128 : W <= 256 ? 256 : 512; }
// the limits of a shape: window 65 .. 512, shift 1 .. W, 1 .. 128 bands, 0 .. M cepstra (0: the log mel energies)
constexpr bool kaldi_shape_ok(int W, int S, int M, int C) { return W >= 65 && W <= 512 && S >= 1 && S <= W && M >= 1 && M <= 128 && C >= 0 && C <= M; }
// high_freq as the table takes it: absolute when > 0, else Kaldi's offset from Nyquist; false unless 0 <= low < high <= Nyquist
bool kaldi_freqs_ok(float sample_rate, float low_freq, float high_freq, double *high_abs = nullptr);
// Kaldi's mel table, in double, rounded once: mel(f) = 1127 ln(1 + f / 700), M + 2 points equally spaced in mel between low and
// high (absolute), f_k = k sample_rate / N for the bins k < N / 2 (the Nyquist bin has no weight).  weights [M][N / 2]; beg /
// len: the non-zero span of every band (len 0: none)
void build_kaldi_mel(int M, int N, float sample_rate, float low_freq, double high_abs, float *weights, int32_t *beg, int32_t *len);
// the table as k_kaldi_front reads it: spans back to back and meta [3][M], as build_slaney_spans lays them out
void build_kaldi_spans(int M, int N, float sample_rate, float low_freq, double high_abs, std::vector<float> &w, std::vector<int32_t> &meta);
// G [C][M] = (float)(l[i] D[i][m]): Kaldi's DCT (row 0 sqrt(1 / M), row i sqrt(2 / M) cos(pi / M (m + 1/2) i)) times its lifter
// l[i] = 1 + Q / 2 sin(pi i / Q) (1 at Q = 0), in double, rounded once
void build_kaldi_dct(int M, int C, float lifter, float *G);
// k_kaldi_front's operands (build_fft_operands, the bins k < N / 2): 3 N floats
void build_kaldi_operands(int W, int N, const float *window, std::vector<float> &out);
// kaldi_flags of mfx_create_kaldi as the code reads them (MFX_KALDI_* of include/mfx.h)
constexpr int kKaldiNoSnipEdges = 1, kKaldiUseEnergy = 2, kKaldiEnergyWindowed = 4, kKaldiHtkCompat = 8, kKaldiFlagsAll = 15;
// a flag word the method serves: known bits only, the windowed energy only with the energy column
constexpr bool kaldi_flags_ok(int flags) { return (flags & ~kKaldiFlagsAll) == 0 && (!(flags & kKaldiEnergyWindowed) || (flags & kKaldiUseEnergy)); }
// static columns of a row: M + 1 for fbank with the energy column, else C or M
constexpr int kaldi_static_cols(int M, int C, int flags) { return C > 0 ? C : M + ((flags & kKaldiUseEnergy) ? 1 : 0); }
// frames of an utterance of n samples: snip_edges = true is frame_count's rule; false (n + S div 2) div S, centred on the hops
int64_t kaldi_frame_count(int64_t samples, int W, int S, int flags);
// Kaldi's mirror of sample index s into an utterance of n >= 1 samples (feature-window.cc: while s < 0 or s >= n: s = -s - 1 or
// 2 n - 1 - s) in closed form: the symmetric reflection of period 2 n.  The kernel and the host restatement share it
constexpr int64_t kaldi_reflect(int64_t s, int64_t n)
{
    int64_t m = s % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}
// idx [W]: the utterance sample of every tap of frame t < kaldi_frame_count(samples) (samples >= 1 then)
void kaldi_frame_samples(int64_t samples, int W, int S, int flags, int64_t t, int64_t *idx);
// sample index relative to the utterance of tap 0 of frame t under snip_edges = false (may be negative: kaldi_reflect maps it)
constexpr int64_t kaldi_centred_start(int64_t t, int W, int S) { return t * S + S / 2 - W / 2; }

// One push of one session of an STFT log-mel handle ("Session log-mel"): a stream that has received n samples and
// delivered rows [0, E) takes `length` more.  While the stream is open E = 0 up to n = N / 2, else min(n div S, (n - N / 2)
// div S + 1): the frames whose taps have all arrived without a right reflection, and that no later sample can take out of
// T(n) = stft_frame_count; E = T(n) once a push is final.  The previous slot holds samples [c0_old, n_old), c0 = max(0, E S -
// N / 2) (the first tap of frame E); the push computes frames [E_old, E_new) from them and the new samples and leaves
// [c0_new, n_new) for the next slot: fewer than N + S samples, nothing after a final push.  Returns E_new - E_old; n and E are
// advanced (both 0 after a final push: the session is fresh).
struct SessionStftStep {
    int64_t c0_old, c0_new;      // first stream sample the previous / the current slot hands on
    int32_t carry_in, carry_out; // samples carried in and out
};
int32_t session_stft_step(int N, int S, int64_t &n, int64_t &E, int64_t length, bool final_push, SessionStftStep &st);
// the most rows one push of `max_samples` samples can deliver: its own, and what a final push adds, N / (2 S) + 1
inline int64_t session_stft_rows_max(int N, int S, int64_t max_samples) { return max_samples / S + N / (2 * S) + 2; }

// The work list of k_sess_stft_mel for one push: piece i delivers n_out[i] rows and is cut into groups of at most 16
// consecutive frames, pieces in their order; block b of the launch takes groups [G b, G b + G).
struct SessStftCut {
    int32_t piece, r0, rows; // the group: rows [r0, r0 + rows) of the piece
};
void cut_sess_stft_groups(const int32_t *n_out, int n, std::vector<SessStftCut> &groups);

} // namespace mfx

namespace mfx {

// Lane plan of the mel stage: the filters are dealt to the `lanes` lanes that share a frame -- 16 (k_front512, k_front1024),
// 32 (k_front2048: the two halves of a wave walk the same filters of their own frames) or 64 (k_front_reg, k_front_wave,
// k_melcep, k_plp) -- a round of `lanes` filters at a time, longest first so that a round's padding is small.  Lane j's
// weights for round r start at w[j * row_stride + sum(L[0..r))], cover bins [start[r][j], start[r][j] + L[r]) in ascending
// order (the reference's summation order, mfcccpu.cpp:192-220) and are zero outside the filter's own span.
struct MelPlan {
    int lanes = 0, rounds = 0;
    int row_stride = 0;            // floats; a multiple of 4 with row_stride / 4 odd (LDS banks)
    int L[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // bins per lane in round r (x8)
    std::vector<float> w;          // [lanes][row_stride]
    std::vector<int32_t> start;    // [rounds][lanes] first bin read
    std::vector<int32_t> fid;      // [rounds][lanes] filter, -1 = idle lane
};
// false when the plan does not fit the kernels' limits (lanes not 16 / 32 / 64, more than 8 rounds, or a padded span that
// would read past `max_read_bin`)
// align: starts are multiples of it (2: two bins per 8-byte read of one magnitude array; 4: the de-interleaved even / odd
// arrays of k_front1024, two bins of each per 8-byte read)
bool build_mel_plan(const MelTable &t, int num_banks, int fft_size, int max_read_bin, int lanes, int align, MelPlan &out);

// B operands of the DCT on the matrix pipe (v_mfma_f32_16x16x4_f32), for every tile of 16 output columns and every
// K step of 4 mel bands: out[(tile * ksteps + j) * 64 + lane] = dct[4 j + (lane >> 4)][16 tile + (lane & 15)],
// zero beyond the matrix.  ksteps = ceil(num_banks / 4), tiles = ceil(dct_len / 16).
void build_dct_mfma_operands(const std::vector<float> &dct, int num_banks, int dct_len, int &tiles, int &ksteps,
                             std::vector<float> &out);

// B operands of the DCT on v_mfma_f32_4x4x1_16b_f32 (k_front2048): 64 output columns per tile, four bands per 16-byte load,
// out[((tile * ks + j4) * 64 + lane) * 4 + u] = dct[4 j4 + u][64 tile + lane], ks = ceil(num_banks / 4), zero beyond the matrix.
void build_dct_mfma_operands4(const std::vector<float> &dct, int num_banks, int dct_len, std::vector<float> &out);

// k_front2048 with at most 40 output columns and a multiple of 32 bands: the 64-column tile of the 4x4x1 form would be
// 37 - 50 % empty.  The 16 blocks of an instruction are dealt to (column group, band part) instead: pass A = 8 groups of 4
// columns x 2 band halves (columns 0..31), pass B = 2 groups x 8 band eighths (columns 32..39); the parts are summed across
// the wave afterwards.  mode 0: not applicable, 1: pass A alone (dct_len <= 32), 2: A + B.
//   out = [nb / 8 groups of pass A][64][4] then [nb / 32 groups of pass B][64][4]:
//   A: out[(g * 64 + lane) * 4 + u] = dct[(lane >> 5) * nb / 2 + 4 g + u][lane & 31]
//   B: out[((nb / 8 + g) * 64 + lane) * 4 + u] = dct[(lane >> 3) * nb / 8 + 4 g + u][32 + (lane & 7)]
int dct_split_mode(int num_banks, int dct_len);
void build_dct_mfma_operands4_split(const std::vector<float> &dct, int num_banks, int dct_len, std::vector<float> &out);

// Transposed, padded DCT matrix for the 512-point kernel: [cols][stride], stride / 4 odd,
// row c = column c of the [num_banks][dct_len] matrix followed by zeros.
void build_dct_transposed(const std::vector<float> &dct, int num_banks, int dct_len, int &stride, int &nb_pad,
                          std::vector<float> &out);

} // namespace mfx
