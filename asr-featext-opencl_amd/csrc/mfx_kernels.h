// mfx_kernels.h -- launch interface of the gfx950 kernels (implemented in mfx_front512.hip, mfx_front_generic.hip, mfx_front2048.hip, mfx_tail.hip, mfx_plp.hip, mfx_traps.hip, mfx_xform.hip, mfx_sess_xform.hip, mfx_sess_resample.hip, mfx_sessions.hip, mfx_resample.hip, mfx_speakers.hip, mfx_vad.hip, mfx_onorm.hip, mfx_slide.hip, mfx_stft.hip, mfx_stft_fft.hip, mfx_kaldi.hip, mfx_kaldi_opts.hip, mfx_pitch.hip, mfx_pitchfeat.hip, mfx_tensor.hip: one translation unit per kernel family).
//
// Kernel inventory and the reference stage each one replaces:
//   spectrum512 / fused512   segmenter.cl kernelSegmentWindow + AppleFFT fft0 + mfcc.cl kernelTranspose
//                            (+ mfcc.cl kernelFilter + the DCT slot when fused)
//   spectrum_generic         same three stages for any power-of-two FFT length
//   melcep                   mfcc.cl kernelFilter + DCT slot (mfccopencl.cpp:315-358) from a stored spectrum
//   plp                      PLP cepstra from a stored spectrum (no reference kernel: the reference names the method only)
//   traps                    TRAPS temporal patterns from stored log mel rows (no reference kernel: the reference names the method only)
//   splice_affine            frame splicing + affine transform of finished rows (no reference analogue: the last stage of a front end)
//   sess_gather              carry state of the session entries: PCM tail + new samples + carried static rows into the current slot
//                            (no reference analogue: the reference re-frames 2 D frames of context per block, segmentercpu.cpp:69-73)
//   resample                 per-utterance sample-rate conversion of the batch entries' PCM (no reference analogue: the reference takes
//                            its files at the one rate its model was trained at)
//   sess_resample            per-session sample-rate conversion in front of a push of the session entries: the chain of resample on
//                            an input span staged from the session's carried input tail and the caller's array (no reference analogue)
//   vad_*                    energy voice-activity decision + voiced-frame selection of finished rows (no reference analogue: the
//                            reference hands every frame to its consumer)
//   pitch_*                  pitch track beside the rows of a batch run: NCCF of the PCM + Viterbi path (no reference analogue)
//   pitch_feats / pitch_paste  Kaldi's pitch features from that track, and their paste into the rows (no reference analogue)
//   onorm_*                  online (causal, sliding-window) CMN / CVN of the batch and session entries (no reference analogue: its
//                            NormalizerCPU keeps one block's statistics)
//   slide_apply              sliding-window CMN / CVN of the batch entries (apply-cmvn-sliding) on onorm's prefix chains (no
//                            reference analogue)
//   stft_mel / stft_post     the STFT log-mel front end: exact-length DFT of centred frames on the matrix pipe, power, Slaney mel, log;
//                            the clamp by the utterance's maximum and the map (no reference analogue: a neural recogniser's input)
//   stft_fft_mel             the same front end at DFT lengths 1024 / 2048: window product, a float32 FFT per wave and frame (half-length
//                            complex Stockham FFT in LDS + real split), then stft_mel's power, mel and log; stft_post follows unchanged
//                            (one launcher surface and one block tail for both; stft_form(N) of mfx_tables.h says which a length gets)
//   sess_stft_mel            the same front end over the frames one push of the session entries completes, groups of 16 frames of
//                            different sessions sharing a block's pass over the basis (no reference analogue)
//   kaldi_front              the Kaldi-compatible fbank / MFCC front end: per-frame DC removal, pre-emphasis, window, a float32 FFT per
//                            wave and frame, power, Kaldi's mel table, log, DCT + lifter with c0 first (no reference analogue)
//   tensor_pack              the finished rows of a batch run as a dense padded tensor, time- or channel-major, float32 / half / bfloat16
//                            (no reference analogue: a neural model's input)
//   delta                    delta.cl kernelDelta x2 + the staging copies of mfccopencl.cpp:360-387
//   norm_stats / norm_apply  norm.cl kernelSum + kernelFinalizeSum / kernelNormalize
// What is attached to a planned batch (vad_*, onorm_*, slide_apply, pitch_*, pitch_feats) walks its rows by one work list, UttTiling below.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mfx_tables.h" // (the item sizes of the utterance tilings: kVadTileRows, kNormChunkRows, kOnormChunk, kPitchFeatRows)

namespace mfx {

// A run of consecutive frames of one utterance (or of the streaming carry buffer).
struct Chunk {
    int64_t pcm_off;  // sample index (per channel) of the first sample of the chunk's first frame
    int64_t out_row;  // destination row of the chunk's first frame
    int32_t n_frames;
    int32_t pad;      // 0, except on a Kaldi handle with snip_edges = false: the chunk's utterance (KaldiParams::utt_bounds), and
                      // pcm_off is then the unreflected start, which may lie in front of the utterance
};

// One independent series of feature rows (an utterance, or the current streaming block) for the
// delta and normalisation kernels.
struct Segment {
    int64_t src_row0;   // first row of the series inside the static-feature buffer
    int64_t out_row0;   // first output row
    int32_t n_out;      // rows to produce
    int32_t shift;      // padded[i] = src[clamp(i + shift, lo, hi)] (rows relative to src_row0)
    int32_t lo, hi;
    int32_t static_off; // static part of output row r is src row r + static_off
    int32_t pad;        // normalisation: rows the statistics cover (0 = all n_out rows)
};

// An utterance tiling ("Utterance tilings"; build_utt_tiling, mfx_tables.h): items of `rows` consecutive rows of one
// utterance, numbered through the batch in utterance order.  Every per-item array of a kernel is indexed absolutely, so that a
// run over an utterance range fills its part and leaves the rest.  utt_item (mfx_dev.h) decodes an item.
struct UttTiling {
    const int32_t *utt_item0; // [n_utt + 1] first item of every utterance (a frameless utterance owns none)
    const int32_t *item_utt;  // [items] the utterance of every item
    int32_t first, count;     // the items of this run's utterance range
    int32_t rows;             // rows per item: the constant the kernel was compiled for, or the launcher refuses
};

// One tile of the delta stage fused into the 512-point kernel: <= 64 consecutive output rows of one
// utterance, all of them inside the owning block's row range.
struct DeltaTile {
    int64_t out_row0;   // first output row (absolute) = first row of the statics scratch the tile owns
    int64_t seg_row0;   // first row of the tile's utterance (statics scratch and output use the same rows)
    int32_t n_rows;
    int32_t r0;         // out_row0 - seg_row0
    int32_t shift, lo, hi, static_off; // the utterance's Segment fields (padded[i] = src[clamp(i + shift, lo, hi)])
    int32_t dep_lo, dep_hi; // block-local chunk indices whose statics the tile reads (inclusive)
};

// LDS floats of one delta tile staged `tr` output rows at a time (delta_tile16<.., TR>): the statics with their 2 (l1 + l2)
// context rows and the deltas with their 2 l2, as 16-float rows; the output rows at up to 48 floats; 8 floats for the
// tile's position inside a 16-byte group.  One formula for the kernels and the host.
__host__ __device__ inline int delta_tile_lds_floats(int tr, int l1, int l2)
{
    return ((tr + 2 * (l1 + l2)) + (tr + 2 * l2)) * 16 + tr * 48 + 8;
}
// Tile sharing in the fused k_front512: a front-end wave that has run out of frames works a tile off as sub-tiles of
// kDeltaShareRows rows in its own frame slots (kDeltaShareFloats of LDS).  Orders whose sub-tile does not fit there do not
// share: the delta wave alone walks the tiles.
constexpr int kDeltaShareRows = 16;
constexpr int kDeltaShareFloats = 4 * 512;
__host__ __device__ inline bool delta_share_fits(int l1, int l2)
{
    return delta_tile_lds_floats(kDeltaShareRows, l1, l2) <= kDeltaShareFloats;
}
// The claim word of a block's tile list, in LDS: head | tail << 16, both biased by one -- tiles [head - 1, tail - 1] of the list
// are unclaimed, and the list is exhausted when head > tail.  The delta wave claims ascending from head, helpers descending
// from tail, each by one compare-exchange: no tile twice, none skipped.  (Host restatement for the planner's bound and tests.)
constexpr int kClaimMaxTiles = 0xfffe;
__host__ __device__ inline uint32_t claim_init(int n_tiles) { return 1u | ((uint32_t)n_tiles << 16); }
__host__ __device__ inline bool claim_empty(uint32_t w) { return (w & 0xffffu) > (w >> 16); }
__host__ __device__ inline int claim_head_tile(uint32_t w) { return (int)(w & 0xffffu) - 1; }
__host__ __device__ inline int claim_tail_tile(uint32_t w) { return (int)(w >> 16) - 1; }
__host__ __device__ inline uint32_t claim_take_head(uint32_t w) { return w + 1u; }
__host__ __device__ inline uint32_t claim_take_tail(uint32_t w) { return w - 0x10000u; }

// A mel lane plan (mfx::MelPlan, mfx_tables.h) as a kernel takes it: the filters dealt to the `lanes` lanes of a frame in
// `rounds` rounds, round r padded to L[r] bins; lane j's weights for all rounds are one row of w.
struct MelPlanArg {
    const float *w;               // [lanes][row_stride]
    const int32_t *start, *fid;   // [rounds][lanes] first bin read / filter index or -1
    int32_t L[8];
    int32_t rounds, row_stride;   // (last: k_front512 reads them and the two DCT sizes behind mel16 in one scalar load)
};
// The 64-lane plans of k_melcep / k_plp, one per table of a sweep, all padded to the same row stride
struct MelTablesArg {
    const float *w;               // [n_tables][64][row_stride]
    const int32_t *start, *fid;   // [n_tables][rounds][64]
    const int32_t *L;             // [n_tables][8] bins per lane and round (device memory)
    int32_t rounds, row_stride;
};

struct FrontParams {
    const int16_t *pcm;
    int64_t pcm_total;        // int16 elements readable behind `pcm` (all channels)
    const Chunk *chunks;
    int32_t n_chunks;
    int32_t channels;         // 1 or 2 (generic kernels only)
    int32_t pair_ok;          // mono, even shift, even window length, even chunk offsets: 2 samples per 32-bit load
    int64_t row_limit;        // frames whose destination row is >= row_limit are skipped
    int32_t window_size;      // W
    int32_t shift;            // S
    int32_t fft_size;         // W2
    // outputs: exactly one of {spec, feat} is used by a launch
    float *spec;              // [rows][spec_pitch] magnitudes |X[k]|/W2, k = 0..W2/2
    int32_t spec_pitch;
    float *feat;              // [rows][feat_pitch], static features written at columns [0, cols)
    int32_t feat_pitch;
    // tables (device pointers)
    const float *window;      // [W2] zero padded                      (generic)
    const float *winpair;     // [16][16][2] window laid out per lane  (512 fast path, k_front1024 phase E)
    const float *win1024o;    // [16][16][4] window x W_512^m as (A, B, C, D) per sample pair (k_front1024 phase O)
    const float *twid_pass;   // [16][16][2] W_256^(l*k)               (512 fast path)
    const float *twid_half;   // [W2/2][2]   W_{W2/2}^k, k < W2/2       (generic Stockham, radix 4 needs 3k)
    const float *twid_reg;    // k_front_reg: pass tables [R1-1][M/R1][2] then [R1-1][M/R1^2][2] (W2 >= 1024)
    const float *twid_split;  // [W2/2+1][2] -i * W_{W2}^k             (real split)
    const float *mel_w;       // [2][W2]
    const int32_t *mel_beg;   // [nb+2]
    const float *dct;         // [nb][dct_len] or nullptr when ceps_len == 0
    // the lane plans (rounds = row_stride = 0: the handle has none that fits the kernel)
    MelPlanArg mel16;             // 512 fast path and k_front1024: the 16 lanes of a frame
    int32_t dct_stride, nb_pad;   // (directly behind mel16: see MelPlanArg)
    const float *dct_t;           // [cols][dct_stride] transposed DCT matrix, rows zero padded to nb_pad
    int32_t dct_mode;             // 0: DCT from the LDS mel scratch; 1: on the matrix pipe, v_mfma_f32_16x16x4_f32 per
                                  //    4 frames (cols <= 16, num_banks <= 40; matrix from `dct`, held in registers)
    MelPlanArg mel64;             // wave-per-frame kernels (k_front_reg / k_front_wave fused): the 64 lanes of the frame's wave
    MelPlanArg mel32;             // k_front2048: the 32 lanes of each of a wave's two frames
    // DCT on the matrix pipe: B operands [dct_tiles][dct_ksteps][64] (build_dct_mfma_operands), read from L1 / L2
    const float *dct_b;
    const float *dct_b4;          // 4x4x1 form: [ceil(dct_len / 64)][dct_ksteps][64][4] (k_front2048, build_dct_mfma_operands4)
    int32_t stuff;                // k_front512: 0, or 512 / fft_size = 2, 4, 8: 256 / 128 / 64-point transforms in the zero-stuffed form
    const float *dct_b4s;         // k_front2048: the split form (build_dct_mfma_operands4_split) or nullptr
    int32_t dct_split;            // dct_split_mode(): 0 none, 1 pass A (<= 32 columns), 2 passes A + B (<= 40 columns)
    int32_t dct_tiles, dct_ksteps;
    int32_t num_banks;
    int32_t dct_len;
    int32_t cols;             // dct_len, or num_banks when ceps_len == 0
    float scale;              // 1/W2 (0.5/W2 where the split's 1/2 is folded in)
    // fused delta stage (512 fast path, launch_front512_delta): block b walks the chunks
    // [blk_chunk_off[b], blk_chunk_off[b+1]) of `chunks` in order (its own rows plus <= D halo rows either
    // side, statics to the compact scratch `feat`, pitch 16) while its last wave turns finished statics
    // into whole [static | d | dd] rows of `out` for the tiles [blk_tile_off[b], blk_tile_off[b+1]).
    const int32_t *blk_chunk_off;
    const int32_t *blk_tile_off;
    const DeltaTile *tiles;
    float *out;
    int32_t out_pitch;
    int32_t dl1, dl2;
    int32_t n_blocks;
    int32_t done_words;       // LDS words of the per-block "chunk finished" bitmap
    int32_t dshare;           // tile sharing: 0 the delta wave alone, 1 idle front-end waves help from the list's tail,
                              // 2 helpers take every tile (the delta wave claims none).  (In what was padding in front of
                              // err_flag: the argument block of every front-end kernel keeps its size and offsets.)
    int32_t *err_flag;        // set nonzero if a delta or helper wave gave up waiting (never expected)
};

struct MelcepParams {
    const float *spec;
    int32_t spec_pitch;
    int64_t n_rows;
    float *feat;
    int32_t feat_pitch;
    int32_t fft_size;
    const float *mel_w;
    const int32_t *mel_beg;
    const float *dct;
    int32_t num_banks, dct_len, cols;
    MelTablesArg mel;             // the 64-lane plan of every table
    int32_t mag_floats;           // LDS floats of a wave's magnitude buffer: >= spec_pitch and > the plans' last read, x4
    const float *dct_b4;          // DCT operands of the 4x4x1 form (build_dct_mfma_operands4) or nullptr
    int32_t dct_ksteps;
    // VTLN sweep: n_tables (>= 1) warped filterbanks over the same spectrum in one launch; table a is
    // mel_w + a * mel_w_stride / mel_beg + a * mel_beg_stride and writes feat + a * feat_table_stride
    int32_t n_tables;
    int32_t mel_beg_stride;
    int64_t mel_w_stride;
    int64_t feat_table_stride;
};

// k_plp (mfx_plp.hip): stored magnitudes -> power -> mel filterbank -> equal loudness + cube root -> autocorrelation ->
// Levinson-Durbin -> LPC cepstrum -> lifter (PLP).  Same spectrum rows, 64-lane mel plan and sweep layout as
// MelcepParams; statics of width cols = ceps_len (+ 1 with c0 as the last column).
struct PlpParams {
    const float *spec;
    int32_t spec_pitch;
    int64_t n_rows;
    float *feat;
    int32_t feat_pitch;
    int32_t fft_size;
    int32_t num_banks;
    int32_t lpc_order;            // p, 1 .. kPlpMaxOrder
    int32_t ceps_len;             // C >= 1
    int32_t want_c0;
    int32_t cols;                 // ceps_len + (want_c0 ? 1 : 0)
    MelTablesArg mel;
    int32_t mag_floats;
    const float *eql;             // [n_tables][num_banks] equal-loudness weights e_m (centres move with alpha)
    const float *idft;            // [lpc_order + 1][num_banks + 2] cosine basis of the autocorrelation (mfx_host_plp_tables)
    const float *lift;            // [ceps_len] lifter weights w_1 .. w_C
    float *r_out;                 // nullptr, or [n_rows][lpc_order + 1] autocorrelations (table 0 only; mfx_debug_read 7)
    int32_t n_tables;
    int64_t feat_table_stride;
};
constexpr int kPlpMaxOrder = 32;

// Row-run form of k_melcep / k_plp (k_melcep_runs / k_plp_runs: per-utterance warp factors of the batch entries,
// DESIGN.md, "Per-utterance warp factors").  Table a = blockIdx.y serves the runs [off[a], off[a + 1]) of `runs`; a run is
// (first row, row count) in absolute rows, ascending and disjoint within a table, and is clipped to the window
// [row0, row0 + rows) by the kernel.  spec and feat of the accompanying parameters address ABSOLUTE rows (there is one
// output: n_rows and feat_table_stride are not used, PlpParams::r_out must be null).
struct RowRuns {
    const int64_t *runs;  // [n_runs][2]: first row, rows
    const int32_t *off;   // [n_tables + 1]
    int64_t row0, rows;   // the window: rows of the spectrum slab
};

// k_traps (mfx_traps.hip): log mel rows -> per band the Hamming-windowed DCT-II of the L frames around every frame
// (TRAPS).  One Segment per utterance: rows src_row0 + clamp(t - (L - 1) / 2 + j, lo, hi) are read, rows
// out_row0 + t, t < n_out, written (shift / static_off / pad are not used).  Statics land at columns m * K + k.
struct TrapsParams {
    const float *src;      // log mel energies, [rows][src_pitch], columns [0, num_banks)
    int32_t src_pitch;
    float *out;            // [rows][out_pitch], columns [0, num_banks * K) written
    int32_t out_pitch;
    const Segment *segs;
    int32_t n_segs;
    int32_t num_banks;     // M
    int32_t L, K;          // trajectory length (odd), coefficients kept
    int32_t valu;          // 0: matrix pipe, operands = build_traps_mfma_operands; 1: vector ALUs, build_traps_valu_operands
    const float *operands;
    int32_t tiles_per_seg_max; // in tiles of 64 rows, as DeltaParams
    int32_t tile_rows;     // set by the launcher: 64, 32 or 16 output rows per block
};

// k_splice_affine (mfx_xform.hip): finished feature rows -> spliced context window -> affine map ("Splice +
// affine transform").  One Segment per utterance: rows src_row0 + clamp(t - left + c, lo, hi), c <= left + right, are read,
// rows out_row0 + t, t < n_out, written (shift / static_off / pad are not used).  Segment s maps with transform seg_xf[s].
struct XformParams {
    const float *src;      // the rows y, [rows][src_pitch], columns [0, width)
    int32_t src_pitch;
    float *out;            // [rows][out_pitch], columns [0, out_dim) written
    int32_t out_pitch;
    const Segment *segs;
    int32_t n_segs;
    const int32_t *seg_xf; // [n_segs] transform of every segment, or nullptr: all 0
    int32_t width;         // Wd
    int32_t left, right;   // context frames, 0 .. 32 each; in_dim = (left + right + 1) * width <= 8192
    int32_t out_dim;       // 1 .. 256
    int32_t valu;          // 0: matrix pipe; 1: vector ALUs (the same operands, the same bits)
    const float *operands; // [n_xf][steps][tiles][64] (build_xform_operands per transform)
    const float *bias;     // [n_xf][tiles * 16], zero beyond out_dim
    int32_t tiles_per_seg_max; // in tiles of 64 rows, as DeltaParams
    int32_t tile_rows;     // set by the launcher: 64, 32 or 16 output rows per block
    int32_t ksteps;        // set by the launcher: steps of 4 taps per LDS chunk of the matrix
};

// k_sess_xform (mfx_sess_xform.hip): the same map over the rows one push of the session entries delivers ("Session
// transform").  The work list: row groups of at most 16 output rows of one session, sorted by transform, and blocks of up to
// tile_rows / 16 consecutive groups of ONE transform (pack_sess_xform_groups, mfx_tables.h).  Group rows r < rows: rows
// src_row0 + clamp(r0 + r - left + c, lo, hi), c <= left + right, are read, row out_row0 + r written.
struct SessXfGroup {
    int64_t src_row0;      // row of `src` that holds row 0 of the session's piece (the first row this push delivers)
    int64_t out_row0;      // output row of the group's first row
    int32_t r0, rows;      // first row of the group inside the piece; its rows (<= 16)
    int32_t lo, hi;        // the piece's clamp window, relative to src_row0
};
struct SessXfBlock {
    int32_t g0, ng;        // the block's groups: [g0, g0 + ng), ng <= tile_rows / 16
    int32_t xf, pad;       // their transform
};
struct SessXformParams {
    const float *src;      // the rows y, [rows][src_pitch], columns [0, width)
    int32_t src_pitch;
    float *out;            // [rows][out_pitch], columns [0, out_dim) written
    int32_t out_pitch;
    const SessXfGroup *groups;
    const SessXfBlock *blocks;
    int32_t n_blocks;
    int32_t width, left, right, out_dim, valu; // as XformParams
    const float *operands; // [n_xf][steps][tiles][64]
    const float *bias;     // [n_xf][tiles * 16]
    int32_t tile_rows;     // 16 G the work list was packed for (0: not checked); the launcher takes sess_xform_tile_rows
    int32_t ksteps;        // set by the launcher
};

// k_sess_gather (mfx_sessions.hip): one push of one session ("Session entries").  The session's CURRENT slot is
// written from three sources -- the PCM tail the previous slot carries, the caller's new samples, the static rows the
// previous slot carries -- and from nowhere else: previous and current slot are different slots of the ping-pong pair.
// PCM counts are int16 ELEMENTS (samples x channels).
struct SessDesc {
    int64_t carry_src;  // slot array: first element of the carried PCM tail (previous slot)
    int64_t pcm_dst;    // slot array: first element of the current slot's PCM part (a multiple of 8: 16-byte words)
    int64_t new_src;    // caller's array: first element of the new samples (any 2-byte alignment)
    int32_t carry_n;    // elements carried
    int32_t new_n;      // elements new
    int64_t row_src;    // statics: first carried row in the previous slot (absolute row, times src_pitch)
    int64_t row_dst;    // statics: first row of the current slot (absolute row, times SessGatherParams::stat_pitch)
    int32_t n_rows;     // rows carried
    int32_t src_pitch;  // floats per row the previous slot was written with
    int64_t y_src;      // finished rows y (session transform): first carried row in the previous y slot (absolute row)
    int64_t y_dst;      // first row of the current y slot
    int32_t y_rows;     // rows carried (0 without a session transform)
    int32_t pad;
};

struct SessGatherParams {
    const SessDesc *descs; // [n_descs]: blockIdx.y
    int32_t n_descs;
    int32_t narrow;        // nonzero: 2-byte loads throughout (the measurement's comparator; same bits)
    const int16_t *pcm;    // the caller's array, 4-byte aligned
    int64_t pcm_elems;     // its int16 elements
    int16_t *slot_pcm;     // both slot arrays (read: previous slots, written: current slots)
    int64_t slot_elems;
    float *slot_stat;      // both statics slot arrays
    int32_t stat_pitch;    // floats per row of the current slots
    int32_t cols;          // static columns
    int32_t items_max;     // set by the planner: the largest item count of any descriptor (sizes the grid)
    float *slot_y;         // both y slot arrays, [rows][y_width] (null without a session transform)
    int32_t y_width;       // Wd: floats per row of y
};

// k_resample (mfx_resample.hip): per-utterance sample-rate conversion, int16 -> int16 ("Sample-rate conversion").
// One ResRate (mfx_tables.h) per distinct input rate of the plan; one ResTile per run of at most tile_out output samples of one
// utterance.
struct ResTile {
    int64_t in_off;     // the utterance in the caller's array: first sample (per channel), any parity
    int64_t out_off;    // the utterance in the scratch: first sample (per channel), even
    int64_t n_in, n_out; // its samples per channel before and after
    int64_t j0;         // first output sample of the tile (a multiple of the rate's tile_out: even)
    int32_t rate;       // index into ResampleParams::rates; -1: same rate, the samples are copied
    int32_t pad;
};
struct ResampleParams {
    const int16_t *pcm; // the caller's array, 4-byte aligned
    int16_t *out;       // the scratch
    const ResTile *tiles;
    const ResRate *rates;
    const float *taps;
    int32_t n_tiles;
    int32_t channels;   // 1 or 2 (interleaved; each channel converted on its own)
    ResLds lds;         // the LDS parts: maxima over the plan's rates
};

// k_sess_resample (mfx_sess_resample.hip): the converter in front of a push of the session entries ("Session
// sample-rate conversion").  One SessResTile per run of at most tile_out outputs of ONE piece; positions are samples per
// channel of the session's STREAM.  The piece's input is stream samples [c0, n_new): [c0, n_old) in the session's previous
// carry slot, [n_old, n_new) in the caller's array; everything outside is zero (after n_new only a final push reads).  The
// piece's first tile also writes the new carry, samples [c1, n_new), to the session's current carry slot (move != 0).
struct SessResTile {
    int64_t in_off;     // caller's array: the piece's first new sample (per channel), any parity
    int64_t out_off;    // scratch: the piece's first converted sample (per channel), even
    int64_t carry_src;  // carry slots: first ELEMENT of the previous slot (a multiple of 8: 16-byte words)
    int64_t carry_dst;  // first element of the current slot
    int64_t c0, n_old, n_new, c1;
    int64_t j_old, j_new; // the piece converts outputs [j_old, j_new)
    int64_t j0;         // first output of the tile (j_old plus a multiple of the rate's tile_out)
    int32_t rate;       // index into SessResampleParams::rates; -1: pass-through, the new samples are copied
    int32_t move;       // nonzero: the tile writes the carry
};
struct SessResampleParams {
    const int16_t *pcm; // the caller's array, 4-byte aligned (may be null when no piece brings samples)
    int16_t *out;       // the scratch of converted pieces
    int16_t *carry;     // both carry slot arrays (read: previous slots, written: current slots)
    const SessResTile *tiles;
    const ResRate *rates;
    const float *taps;
    int32_t n_tiles;
    int32_t channels;
    ResLds lds;         // as in ResampleParams
};

struct DeltaParams {
    const float *src;      // static features, [rows][src_pitch]
    int32_t src_pitch;
    float *out;            // [rows][out_pitch]: [static | delta | acc]
    int32_t out_pitch;
    const Segment *segs;
    int32_t n_segs;
    int32_t cols;
    int32_t l1, l2;        // l2 == 0: first order only; l1 == 0: copy statics only
    int32_t tiles_per_seg_max;
    int32_t inline_seg;    // nonzero: ignore segs and use seg0 (single streaming block)
    Segment seg0;
};

struct NormParams {
    float *data;           // [rows][pitch], normalised in place at column offset col0
    int32_t pitch;
    int32_t col0;
    int32_t cols;
    const Segment *segs;   // uses out_row0 / n_out (rows to normalise) only
    int32_t n_segs;
    int32_t row_off;       // extra row offset added to out_row0
    int32_t norm_type;     // MFX_NORM_*
    float *stats;          // [n_segs][2][cols]: mean, scale (persist across calls for use_last_stats)
    int32_t inline_seg;    // nonzero: ignore segs and use seg0
    Segment seg0;
    int32_t max_rows;      // largest row count of any segment (sizes the grids)
    int32_t chunks;        // set by the launcher: row chunks per segment
    double *partial;       // [n_segs][chunks][4][cols] scratch, needed when max_rows > 4096 (norm_partial_doubles)
    int32_t groups;        // launch_norm_fused only: column groups col0 + g * cols normalised in ONE launch (0 / 1: one)
    int64_t group_stats_stride; // floats between the statistics of consecutive groups
};

// Per-speaker normalisation (mfx_batch_set_speakers; mfx_speakers.hip).  Wn = cols * groups normalised columns.
struct SpkTile {
    int64_t row0;          // first row of the tile (rows of ONE utterance)
    int32_t rows;
    int32_t spk;           // the utterance's speaker
};

struct SpkParams {
    float *data;           // [rows][pitch], normalised in place at columns 0 .. Wn - 1
    int32_t pitch;
    int32_t cols;          // columns of one group (<= 256): the statistics' thread mapping is per group
    int32_t groups;        // 1 (before the deltas), else the groups of the row
    int32_t norm_type;     // MFX_NORM_*
    int32_t mode;          // MFX_SPK_*
    const Segment *segs;   // [n_utt]: uses out_row0 / n_out (ALL rows of the utterance)
    int32_t n_utt;
    int32_t u0;            // set by the launcher: first utterance of the launch
    int32_t max_rows;      // largest row count of any utterance (sizes the grid)
    const int32_t *utt_chunk0; // [n_utt + 1] first chunk of every utterance: UttTiling::utt_item0 at kNormChunkRows
    double *partial;       // [chunks][4][Wn]: S, S2, min, max of every chunk
    const int32_t *spk_off;  // [n_spk + 1]
    const int32_t *spk_list; // utterances of every speaker, ascending, frameless ones left out
    int32_t n_spk;
    const int64_t *prior_count; // [n_spk] or null
    const double *prior_acc;    // [n_spk][4][Wn] or null
    int64_t *count;        // [n_spk]
    double *acc;           // [n_spk][4][Wn]
    float *stats;          // [n_spk][2][Wn]: mean, multiplier
    const SpkTile *tiles;
    int32_t n_tiles;
};

// Energy VAD + voiced-frame selection (mfx_batch_set_vad; mfx_vad.hip; DESIGN.md, "Voice activity and frame selection").
// Two utterance tilings: tiles of kVadTileRows rows, chunks of kNormChunkRows.
struct VadParams {
    const float *y;        // the rows the decision reads, [rows][y_pitch]
    int32_t y_pitch;
    int32_t column;        // 0 <= column < y_pitch
    const Segment *segs;   // [n_utt]: uses out_row0 / n_out
    int32_t n_utt;
    int32_t u0, u1;        // the utterance range of this run
    UttTiling tiles, chunks;
    float energy_threshold, energy_mean_scale, proportion_threshold;
    int32_t frames_context; // 0 .. 64
    int32_t mode;          // MFX_VAD_*: 0 flags only, 1 select inside every utterance's rows, 2 pack the batch
    double *partial;       // [chunks] sum of e over every chunk
    float *thr;            // [n_utt]
    int32_t *voiced;       // [n_utt]
    uint8_t *flags;        // [total_rows]
    uint64_t *mask;        // [tiles] bit r: row r of the tile is voiced
    int32_t *tile_base;    // [tiles] voiced rows of the utterance in front of the tile
    int64_t *packed_row0;  // [n_utt + 1] exclusive prefix of voiced (written by a run that reaches the last utterance)
    const float *rows;     // modes 1, 2: the finished rows, [total_rows][width], 16-byte aligned
    float *out;            // modes 1, 2: the caller's array, [total_rows][width]; never `rows`
    int32_t width;
};

// Pitch track (mfx_batch_set_pitch; mfx_pitch.hip; DESIGN.md, "Pitch track").  One utterance tiling at pitch_tile_frames
// frames, the one run-time item size; every per-row array is indexed by the plan's rows.
struct PitchParams {
    const int16_t *pcm;    // the array the front end reads (the converted scratch under a rates plan)
    int32_t channels;      // 1, or 2: one 32-bit word per sample, p = (L + R) >> 1
    const int64_t *utt;    // [n_utt][2]: first sample (per channel) and samples of every utterance
    const Segment *segs;   // [n_utt]: uses out_row0 / n_out
    UttTiling tiles;       // (rows: pitch_tile_frames)
    int32_t u0, u1;        // the utterance range of this run
    int32_t window, shift, lag_min, lag_max, K, J;
    int32_t span_pad;      // pitch_span_pad(shift)
    int32_t groups;        // pitch_groups(lag_min, lag_max): frames a wave of k_pitch_nccf takes at a time, 1 or 2
    float ballast, penalty;
    float c1;              // (float)(1 / (32768 (window + lag_max)))
    const float *wt, *lg;  // [K]
    float *nccf;           // [total_rows][K]: k_pitch_nccf leaves e(l_k) there on its way, then rho
    uint16_t *bp;          // [total_rows][K] back-pointers (the state k' itself)
    float *pitch;          // [total_rows][2] lag, rho
    int32_t *index;        // [total_rows]
};
bool pitch_params_ok(const PitchParams &p);
int pitch_groups(int lag_min, int lag_max);
size_t pitch_nccf_lds_bytes(const PitchParams &p);
// k_pitch_nccf over the tiles, then k_pitch_track over the utterances of the range
hipError_t launch_pitch(const PitchParams &p, hipStream_t stream);

// Pitch features (mfx_batch_set_pitch_feats; mfx_pitchfeat.hip; DESIGN.md, "Pitch features").  One utterance tiling at
// kPitchFeatRows; `pitch` and `feats` are indexed by the plan's rows.
constexpr int kPfPov = 1, kPfNorm = 2, kPfDelta = 4, kPfRaw = 8; // MFX_PF_* of include/mfx.h
struct PitchFeatParams {
    const float *pitch;    // [total_rows][2] lag, rho as k_pitch_track wrote them
    const Segment *segs;   // [n_utt]: uses out_row0 / n_out
    UttTiling tiles;
    int32_t columns, F;    // MFX_PF_* bits (resolved: never 0) and their number
    int32_t left, right, D;
    float sample_rate, pov_scale, pov_offset, pitch_scale, delta_scale;
    double delta_den;      // 2 sum of l^2 over l = 1 .. D
    float *feats;          // [total_rows][F]
};
bool pitch_feat_params_ok(const PitchFeatParams &q);
hipError_t launch_pitch_feats(const PitchFeatParams &q, hipStream_t stream);
// rows [row0, row0 + rows) of out [.][Wd + F] = [ narrow [.][Wd] | feats [.][F] ]
struct PitchPasteParams {
    const float *narrow, *feats;
    float *out;
    int64_t row0, rows;
    int32_t Wd, F;
};
hipError_t launch_pitch_paste(const PitchPasteParams &q, hipStream_t stream);

// Dense padded tensor output (mfx_batch_set_tensor; mfx_tensor.hip; DESIGN.md, "Tensor output").  No work list: a regular grid of
// (u1 - u0) x ceil(Tp / kTensorTileRows) blocks, block (u, i) owning rows t in [i R, min((i + 1) R, Tp)) of utterance u.
struct TensorUtt {
    int64_t row0;          // first row of the utterance in `rows`
    int32_t T;             // its rows in the plan
    int32_t pad;
};
struct TensorParams {
    const float *rows;     // the finished rows, [total_rows][Wo]
    void *out;             // the tensor: [B][Tp][Wo] or [B][Wo][Tp] elements of `dtype`, element-aligned
    const TensorUtt *utt;  // [B]
    const int32_t *voiced; // [B] rows that count of every utterance (MFX_VAD_SELECT), or null: TensorUtt::T
    int32_t *len;          // [B] min(L_u, Tp), written by block (u, 0)
    int32_t u0, u1;        // the utterance range of this run
    int32_t Tp, Wo;        // Tp >= 0, 1 <= Wo
    int32_t layout, dtype; // kTensor*, kDtype* (mfx_tables.h)
    float pad_value;
};
bool tensor_params_ok(const TensorParams &p);
hipError_t launch_tensor_pack(const TensorParams &p, hipStream_t stream);

// Online CMN / CVN (mfx_batch_set_online_norm, mfx_sessions_set_online_norm; mfx_onorm.hip; DESIGN.md, "Online
// normalisation").  One utterance tiling at kOnormChunk rows.
struct OnormParams {
    const float *src;      // the raw rows, [rows][src_pitch], columns [0, Wn): never `out`
    int32_t src_pitch;
    float *out;            // [rows][out_pitch], columns [0, Wn) written
    int32_t out_pitch;
    int32_t Wn;            // 1 .. 256
    int32_t window;        // N: 0, or a multiple of 32
    int32_t cvn;           // 0: CMN, else CVN
    int32_t prior_frames;  // F
    int64_t prior_count;   // p
    const double *prior_acc; // [2][Wn] or null (p == 0)
    const Segment *segs;   // [n_utt]: uses out_row0 / n_out
    UttTiling chunks;
    double *tot;           // [chunks][2][Wn]: the chunks' totals of v and q, turned into the offsets O in place
    int32_t u0, n_utt;     // the utterance range of this run: [u0, u0 + n_utt)
};

// Sliding-window CMN / CVN (mfx_batch_set_sliding_norm; mfx_slide.hip; DESIGN.md, "Sliding-window normalisation"): the
// online normaliser's prefix chains (launch_onorm_prefix fills pre.tot from pre.src) and k_slide_apply over the same tiling.
// `pre` carries src, src_pitch, out, out_pitch, Wn, segs, chunks, tot, u0, n_utt; its window, cvn and prior fields are not read.
struct SlideParams {
    OnormParams pre;
    int32_t window;        // N: 1 .. 4096
    int32_t min_window;    // 0 .. N (read without `center` only)
    int32_t center;        // 0 / 1
    int32_t norm_vars;     // 0: CMN, 1: CVN
};

// k_onorm_sess: the rows one push brings one session, rows [t0, t0 + n_rows) of its stream, normalised in place
struct OnormSessDesc {
    int64_t row0;          // first row inside OnormSessParams::data
    int64_t t0;            // rows of the stream in front of it (0: the session is fresh, its state is not read)
    int32_t n_rows;
    int32_t session;
};
struct OnormSessParams {
    float *data;           // [rows][pitch], columns [0, Wn) normalised in place
    int32_t pitch;
    int32_t Wn;
    int32_t window, cvn, prior_frames;
    int64_t prior_count;
    const double *prior_acc;
    const OnormSessDesc *descs;
    int32_t n_descs;
    double *state;         // [n_sessions][8][Wn]: lead O (v, q), lead I (v, q), trail O (v, q), trail I (v, q)
    float *ring;           // [n_sessions][window][Wn] the last `window` raw rows (null when window == 0)
};

// STFT log-mel front end (mfx_stft.hip; DESIGN.md, "STFT log-mel"): one block of k_stft_mel takes a run of at most tile_rows
// consecutive centred frames of one utterance
struct StftChunk {
    int64_t utt_off;     // first sample of the chunk's UTTERANCE in the PCM array
    int64_t utt_len;     // its samples (the reflections happen at its ends)
    int64_t out_row;     // destination row of the chunk's first frame
    int32_t t0;          // first frame of the chunk inside the utterance
    int32_t n_frames;
    int32_t utt_chunk0;  // first chunk of the utterance, and how many it has: the slots k_stft_post takes its maximum over
    int32_t utt_chunks;  // (both count from the plan's first chunk)
};

// (utt_chunk0 / utt_chunks 0 where no k_stft_post follows: the session entries)
inline StftChunk make_stft_chunk(int64_t utt_off, int64_t utt_len, int64_t out_row, int32_t t0, int32_t n_frames, int32_t chunk0 = 0, int32_t chunks = 0)
{
    return StftChunk{utt_off, utt_len, out_row, t0, n_frames, chunk0, chunks};
}

constexpr int kStftKSteps = 2; // steps of 4 taps per LDS buffer of basis operands

// A mel table as the STFT log-mel and the Kaldi kernels read it (pack_mel_spans of mfx_tables.h): the rows' non-zero spans back to
// back, and per row its first bin, its bins and its first weight
struct MelSpans {
    const float *w;
    const int32_t *beg, *len, *off; // [M]
};

// what every kernel of the method takes: the shape, the post mode, the DFT operands of the handle's form, the mel spans, the rows
struct StftCore {
    int32_t N, S, M;            // DFT length, hop, mel bands
    int32_t post;               // MFX_LOGMEL_*
    const float *operands;      // matrix form: [pass][step][tile of the pass][64] (build_stft_operands); FFT form: the window, the
                                // twiddles and the split table back to back (build_stft_fft_operands: 3 N + 2 floats)
    MelSpans mel;               // the rows of the Slaney table
    float *out;
    int32_t out_pitch;
};

// The batch front end of either form (stft_form(N)): k_stft_mel at tile_rows 64, 32 or 16, or k_stft_fft_mel (mfx_stft_fft.hip;
// DESIGN.md, "STFT log-mel, FFT form") at 16, 8 or 4; k_stft_post follows either unchanged.
struct StftParams {
    const int16_t *pcm;
    const StftChunk *chunks;    // the launch's chunks (blockIdx.x)
    int32_t n_chunks;
    int32_t chunk_first;        // index of chunks[0] in the plan: its slot in blk_max
    int32_t tile_rows;          // frames per block the chunks were cut for
    StftCore core;
    float *blk_max;             // [chunks of the plan] the largest log value of every block (WHISPER)
};
// ALL the LDS a block of the form's kernel asks for at tile_rows frames per block: the kernels declare no static LDS beside it
size_t stft_lds_bytes(int N, int S, int M, int tile_rows);
int stft_tile_rows(int N, int S, int M); // frames per block: the largest of the form's three tiles whose LDS fits, 0: none
hipError_t launch_stft(const StftParams &p, hipStream_t stream);      // k_stft_mel or k_stft_fft_mel, by the form of p.core.N
hipError_t launch_stft_post(const StftParams &p, hipStream_t stream); // k_stft_post (WHISPER: clamp and map, in place)

// k_sess_stft_mel (mfx_stft.hip; DESIGN.md, "Session log-mel"): the rows one push of the session entries delivers on an STFT
// log-mel handle.  The work list: groups of at most 16 consecutive frames of ONE session (StftChunk: utt_off is the element of
// `pcm` where the stream's sample 0 lies or WOULD lie -- the slot holds the stream from a later sample on, so it may be
// negative --, utt_len the stream's samples, at whose ends the reflections happen; utt_chunk0 / utt_chunks are not used);
// block b takes groups [G b, G b + G), wave g of it group g.  No element outside [0, pcm_elems) is read.
struct SessStftParams {
    const int16_t *pcm;         // both PCM slot arrays of the session entries
    int64_t pcm_elems;
    const StftChunk *groups;
    int32_t n_groups;
    int32_t G;                  // groups per block the lists were sized for: sess_stft_groups, or the launcher refuses
    StftCore core;
};
// ALL the LDS a block of k_sess_stft_mel asks for at G groups per block; the G the launcher takes: the largest of 4 / 2 / 1
// whose LDS fits 160 KB (0: the shape is outside the limits of the matrix form)
size_t sess_stft_lds_bytes(int N, int S, int M, int G);
int sess_stft_groups(int N, int S, int M);
hipError_t launch_sess_stft(const SessStftParams &p, hipStream_t stream);

// k_kaldi_front (mfx_kaldi.hip; DESIGN.md section 5, "Kaldi front end"): the front end of MFX_METHOD_KALDI over the chunks of a
// batch plan or of a push -- one block per Chunk of at most 16 frames, statics to `feat` as the fused kinds deliver them.
struct KaldiParams {
    const int16_t *pcm;
    int64_t pcm_total;          // int16 elements readable behind `pcm` (mono)
    const Chunk *chunks;        // the launch's chunks (blockIdx.x)
    int32_t n_chunks;
    int64_t row_limit;          // frames whose destination row is >= row_limit are skipped
    int32_t W, S, N;            // window, shift, DFT length kaldi_fft_size(W)
    int32_t M, C;               // mel bands; cepstra (0: the log mel energies are the statics)
    float preemph;              // c in [0, 1]
    int32_t remove_dc, use_power;
    const float *operands;      // window [N] zero padded | W_{N/2}^k, k < N / 2, complex | -i W_N^k, k < N / 2, complex (build_kaldi_operands)
    MelSpans mel;               // the bands of Kaldi's table
    int32_t mel_w_floats;       // floats of mel.w: 1 .. N (a bin lies in two bands at most)
    const float *dct_t;         // [M][C]: G transposed (null at C = 0)
    float *feat;                // [rows][feat_pitch], statics at columns [0, kaldi_static_cols(M, C, flags))
    int32_t feat_pitch;
    // kaldi_flags of mfx_create_kaldi (kKaldi* of mfx_tables.h); 0: everything below is unused and the rows are those of a handle without
    int32_t flags;
    float energy_log_floor;     // (float)log(energy_floor), -inf for none: the energy column is max(logE, this)
    // kKaldiNoSnipEdges: [n_utt][2] = (first sample, samples) of every utterance; a chunk's `pad` is its utterance and its
    // pcm_off the UNREFLECTED start of its first frame (it may lie in front of the utterance): the span is gathered through
    // kaldi_reflect from the utterance's own samples
    const int64_t *utt_bounds;
    int32_t n_utt;
};
// ALL the LDS a block of k_kaldi_front asks for: the kernel declares no static LDS beside it
size_t kaldi_lds_bytes(int W, int S, int M, int C, int flags = 0);
hipError_t launch_kaldi(const KaldiParams &p, hipStream_t stream);

// All launchers are asynchronous on `stream` and return the launch status.
// every launch of the VAD stage for utterances [u0, u1), in order
hipError_t launch_vad(const VadParams &p, hipStream_t stream);
bool vad_shape_ok(const VadParams &p);
// online normaliser: chunk totals -> offsets -> apply over the utterance range (three launches); the session form
hipError_t launch_onorm(const OnormParams &p, hipStream_t stream);
hipError_t launch_onorm_sess(const OnormSessParams &p, hipStream_t stream);
hipError_t launch_onorm_prefix(const OnormParams &p, hipStream_t stream); // k_onorm_totals + k_onorm_offsets alone
hipError_t launch_slide(const SlideParams &p, hipStream_t stream);        // launch_onorm_prefix, then k_slide_apply
// per-speaker normalisation: chunk totals; accumulators + statistics; apply.  spk_tile_rows: rows of a tile of k_spk_apply at
// Wn columns; spk_chunks: chunks of kNormChunkRows rows of an utterance of `rows` rows
hipError_t launch_spk_sums(const SpkParams &p, hipStream_t stream);
hipError_t launch_spk_finish(const SpkParams &p, hipStream_t stream);
hipError_t launch_spk_apply(const SpkParams &p, hipStream_t stream);
int spk_tile_rows(int wn);
int spk_chunks(int64_t rows);
hipError_t launch_front512(const FrontParams &p, bool to_spectrum, bool aligned, int nm16, hipStream_t stream);
// fused front end + delta stage (p.blk_chunk_off etc. filled in); statics only pass through p.feat
hipError_t launch_front512_delta(const FrontParams &p, bool aligned, int nm16, hipStream_t stream);
size_t front512_delta_lds_bytes(const FrontParams &p);
// fused = mel/log/DCT in the same kernel (statics to p.feat); else magnitudes to p.spec
hipError_t launch_front_generic(const FrontParams &p, bool fused, hipStream_t stream);
size_t front_wave_lds_bytes(const FrontParams &p, bool fused);
hipError_t launch_melcep(const MelcepParams &p, hipStream_t stream);
// the row-run forms: h_off / h_runs are the host's copies of rr.off / rr.runs (they size the grid; nothing is allocated)
hipError_t launch_melcep_runs(const MelcepParams &p, const RowRuns &rr, const int32_t *h_off, const int64_t *h_runs, hipStream_t stream);
hipError_t launch_plp_runs(const PlpParams &p, const RowRuns &rr, const int32_t *h_off, const int64_t *h_runs, hipStream_t stream);
hipError_t launch_delta(const DeltaParams &p, hipStream_t stream);
hipError_t launch_plp(const PlpParams &p, hipStream_t stream);
hipError_t launch_traps(const TrapsParams &p, hipStream_t stream);
// LDS of k_traps with tile_rows output rows per block; traps_tile_rows: the tile the launcher takes (0: none fits)
size_t traps_lds_bytes(const TrapsParams &p, int tile_rows);
int traps_tile_rows(const TrapsParams &p);
hipError_t launch_xform(const XformParams &p, hipStream_t stream);
hipError_t launch_sess_gather(const SessGatherParams &p, hipStream_t stream);
// k_sess_xform: LDS at tile_rows = 16 G rows per block; the tile the launcher takes (the largest G of 4, 2, 1 inside
// kTileLdsTarget, else the largest inside 160 KB; 0: the shape is outside the limits, or none fits); the launch
size_t sess_xform_lds_bytes(const SessXformParams &p, int tile_rows);
int sess_xform_tile_rows(const SessXformParams &p);
hipError_t launch_sess_xform(const SessXformParams &p, hipStream_t stream);
// k_resample and k_sess_resample (geometry and the LDS sum: mfx_tables.h)
hipError_t launch_resample(const ResampleParams &p, hipStream_t stream);
hipError_t launch_sess_resample(const SessResampleParams &p, hipStream_t stream);
// work items of one descriptor: 16-byte words of PCM, then 16-byte words (or single floats) of static rows, then the floats
// of the carried rows y
int sess_gather_items(const SessDesc &d, int stat_pitch, int cols, int y_width = 0);
// LDS of k_splice_affine with tile_rows output rows per block; xform_tile_rows: the tile the launcher takes (0: the shape is
// outside the limits, or none fits); xform_shape_ok: width, context, in_dim and out_dim inside the kernel's limits
size_t xform_lds_bytes(const XformParams &p, int tile_rows);
int xform_tile_rows(const XformParams &p);
bool xform_shape_ok(const XformParams &p);
// LDS of k_plp with n_waves waves per block (the launcher takes as many of 4 as fit)
size_t plp_lds_bytes(const PlpParams &p, int n_waves);
// LDS of k_melcep with n_waves waves per block (the launcher takes as many of 4 as fit)
size_t melcep_lds_bytes(const MelcepParams &p, int n_waves);
hipError_t launch_norm_stats(const NormParams &p, hipStream_t stream);
// doubles of NormParams::partial for n_segs segments of at most max_rows rows (0: none needed)
size_t norm_partial_doubles(int n_segs, int max_rows, int cols);
hipError_t launch_norm_apply(const NormParams &p, hipStream_t stream);
// copy of a small block (even byte count) by a kernel; either side may be page-locked host memory
hipError_t launch_copy_small(void *dst, const void *src, size_t bytes, hipStream_t stream);
// statistics + apply in one launch, for segments of at most 48 KB of rows (norm_fused_fits); same bits as the pair above
bool norm_fused_fits(int max_rows, int cols);
hipError_t launch_norm_fused(const NormParams &p, hipStream_t stream);

// dynamic LDS bytes one block of the 512-point kernel needs for these parameters
size_t front512_lds_bytes(const FrontParams &p);

// true when the 512-point fast path can take this configuration
bool front512_supported(int fft_size, int window_size, int num_banks, int cols, int channels);
// k_front1024: 1024-point transform of a window of at most 512 samples on the k_front512 core (two 256-point complex
// transforms per frame: even and odd bins), mel -> log -> DCT fused, statics out
bool front1024_supported(int fft_size, int window_size, int num_banks, int cols, int channels, int ceps_len);
size_t front1024_lds_bytes(const FrontParams &p, int waves = 12);
int front1024_waves(const FrontParams &p, bool aligned, int nm16, int max_waves = 16); // 16 waves per CU where the build and the LDS allow, else 12
hipError_t launch_front1024(const FrontParams &p, bool aligned, int nm16, hipStream_t stream, int max_waves = 16);

// k_front2048 (mfx_front2048.hip): 2048-point transform of a window of at most 1152 samples, two frames per wave (32 lanes
// each, 32 x 32 two-pass FFT), mono (aligned sample pairs) or interleaved stereo, mel -> log -> DCT fused, statics out
bool front2048_supported(int fft_size, int window_size, int num_banks, int cols, int channels);
size_t front2048_lds_bytes(const FrontParams &p);
hipError_t launch_front2048(const FrontParams &p, int num_cus, hipStream_t stream);

} // namespace mfx
