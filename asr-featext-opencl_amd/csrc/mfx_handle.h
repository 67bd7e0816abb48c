// mfx_handle.h -- internal to the host side of libmfcchip (not installed): the handle behind include/mfx.h, the buffer
// types it owns (UttTilingBuf among them: the one owner of an utterance tiling, host and device), and the few helpers its
// translation units share.
//   mfx_api.cpp    lifetime, tables, kernel choice and front-end dispatch, profiling, test taps (writes the shared part)
//   mfx_stream.cpp the streaming state machine and its host copies         (owns `st` and `sweep`)
//   mfx_batch_plan.cpp   the batch planner, the rates planner, the fused-delta plan (owns `batch`'s plan, `batch.rs`, `fuse`)
//   mfx_batch_attach.cpp what is attached to a plan: warp factors, transform, speakers, VAD, online normaliser, pitch track,
//                        pitch features, tensor output (owns `batch.va`, `.xf`, `.spk`, `.vad`, `.on`, `.pt`, `.pf`, `.tn`)
//   mfx_batch.cpp        the batch runner, device and host entries, overlap   (owns `batch.ov` and `batch.host`)
//   mfx_sessions_host.cpp the session entries: many live streams per push       (owns `sess`; the pending push is `sess.push`)
#pragma once
#include "../../include/mfx.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "mfx_kernels.h"
#include "mfx_tables.h"

constexpr int kChunkFrames = 16;           // frames per work item of the front-end kernels
constexpr size_t kLdsCap = 160 * 1024;     // LDS a block may ask for on gfx950 (the launchers' name for it: kLdsMax, mfx_launch.h)
constexpr int64_t kFuseMinFrames = 500000; // frames of a batch from which the fused delta stage runs without being asked for
                                           // (profiles/r13/README.md; above every batch of the suites that pin the two-kernel path)
constexpr int64_t kFuseMaxFrames = 2000000; // ... and up to which: on a 12.5 M-frame batch it loses 5 % to the two kernels
constexpr size_t kSmallBlock = (size_t)1 << 20; // below this a copy kernel replaces the DMA command (streaming interface)

inline constexpr const char *kMsgBuffer = "Can't process data, buffer is too small";
inline constexpr const char *kMsgWindow = "Can't process data, window count is too small";
inline constexpr const char *kMsgProcessed = "Processed samples <= 0, this should never happen";
inline constexpr const char *kMsgHigh = "Window count too high";

// device memory, freed with its owner
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
    DevBuf &operator=(DevBuf &&o) noexcept // (o frees what this held)
    {
        std::swap(p, o.p), std::swap(n, o.n);
        return *this;
    }
    ~DevBuf() { release(); }
    // device == false (planning handles, mfx_handle::alloc): records the size, allocates nothing
    hipError_t alloc(size_t count, bool device = true)
    {
        release();
        if (count > 0 && device) {
            const hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
            if (e != hipSuccess) {
                p = nullptr;
                return e;
            }
        }
        n = count;
        return hipSuccess;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

// page-locked host memory, freed with its owner
template <class T>
struct PinnedBuf {
    T *p = nullptr;
    size_t n = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { release(); }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    // fewer than `need` elements: wait for `stream` (work on it may still use the old block), then replace the block by
    // one of `want` (>= need) elements
    hipError_t grow(size_t need, size_t want, hipStream_t stream)
    {
        if (n >= need) return hipSuccess;
        if (hipError_t e = hipStreamSynchronize(stream); e != hipSuccess) return e;
        release();
        if (hipError_t e = hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault); e != hipSuccess) {
            p = nullptr;
            return e;
        }
        n = want;
        return hipSuccess;
    }
};

// Mel lane plans in device memory (mfx::MelPlan -> MelPlanArg / MelTablesArg, mfx_kernels.h): the one owner of the arrays a
// kernel walks.  `n` plans (the 64-lane plans of a sweep's tables) are padded to the longest plan's row stride: a row's rounds
// lie back to back from its start, so padding at the end changes nothing; one plan keeps its own stride.
struct MelPlanBuf {
    DevBuf<float> w;               // [n][lanes][row_stride]
    DevBuf<int32_t> start, fid, L; // [n][rounds][lanes] twice, [n][8]
    int n = 0, rounds = 0, row_stride = 0, L0[8] = {}; // (rounds and L0 are plan 0's: every plan of a set has ceil(nb / lanes) rounds)
    bool ok = false;               // built, in place AND the LDS of the kernel that walks it fits (whoever calls set() decides the latter)
    // the host fields alone: what the LDS sums need before anything is replaced
    void shape(const mfx::MelPlan *plans, int count)
    {
        n = count, rounds = plans[0].rounds, row_stride = 0;
        for (int a = 0; a < count; ++a) row_stride = std::max(row_stride, plans[a].row_stride);
        std::copy(plans[0].L, plans[0].L + 8, L0);
    }
    // shape() + upload (defined behind mfx_handle); ok on success.  The caller has waited for whatever reads the old arrays.
    int set(mfx_handle *h, const mfx::MelPlan *plans, int count);
    // plan 0 as a front end takes it; rounds = row_stride = 0 unless ok, so that no LDS sum and no launch counts on it
    mfx::MelPlanArg arg() const
    {
        mfx::MelPlanArg a{w.p, start.p, fid.p, {}, ok ? rounds : 0, ok ? row_stride : 0};
        std::copy(L0, L0 + 8, a.L);
        return a;
    }
    // all n plans as k_melcep / k_plp take them (valid from shape() on: build_cep_tables probes with it)
    mfx::MelTablesArg tables_arg() const { return {w.p, start.p, fid.p, L.p, rounds, row_stride}; }
};

// What k_melcep / k_plp read for n warp factors: the mel tables (mel_w [n][2 * W2], mel_beg [n][nb + 2]), one 64-lane
// plan per table (plan64) and, for PLP, the equal-loudness weights (eql [n][nb]).
struct CepTables {
    DevBuf<float> mel_w, eql;
    DevBuf<int32_t> mel_beg;
    MelPlanBuf plan64;
    std::vector<float> alphas; // the warp factors the tables hold (empty: none)
    bool holds(const float *a, int n) const { return !alphas.empty() && (int)alphas.size() == n && std::equal(a, a + n, alphas.begin()); }
};

// An utterance tiling of the planned batch (mfx::UttTiling, mfx_kernels.h; DESIGN.md, "Utterance tilings"): the host's item0,
// the kernels' two arrays, the item size
struct UttTilingBuf {
    int32_t rows = 0;
    std::vector<int32_t> item0;          // [n_utt + 1]
    DevBuf<int32_t> d_item0, d_item_utt; // [n_utt + 1], [items]
    // builds the tiling of the plan's utterances at `rows_per_item` and uploads it (defined behind mfx_handle): MFX_ERR_ARG,
    // "batch too long", leaves the tiling as it was
    int set(mfx_handle *h, int32_t rows_per_item);
    // the items of utterances [u0, u1), as a kernel takes them
    mfx::UttTiling range(int u0, int u1) const { return {d_item0.p, d_item_utt.p, item0[u0], item0[u1] - item0[u0], rows}; }
    size_t items() const { return item0.empty() ? 0 : (size_t)item0.back(); }
    void release() { d_item0.release(), d_item_utt.release(); }
};

// streaming state (segmentercpu.h:7-17, parambase.h:18): mfx_stream.cpp
struct StreamState {
    DevBuf<int16_t> d_carry[2];
    int cur = 0;
    size_t carry_capacity = 0;
    int remaining = 0, samples = 0;
    bool flushed = true, last_calc_flushed = false, last_block = false;
    int block_wcnd = 0;      // frames (with context) the last FFT covered
    int block_frames = 0;    // frames apply() delivers
    DevBuf<float> d_src, d_blk, d_stats, d_plp_r; // (d_plp_r: PLP's r taps)
    DevBuf<mfx::Chunk> d_chunks;
    int chunk_frames = 16;
    int n_chunks_max = 0;
    PinnedBuf<int16_t> h_stage;
    // small-block handles (every block under 1 MB): the carried tail stays on the HOST, inside the pinned staging buffer, and
    // goes up again in front of the next block -- one copy kernel per set_input instead of copy + device-to-device tail copy
    bool host_tail = false;
    size_t stage_tail_off = 0;  // samples: where the pending tail (`remaining` samples) starts in h_stage
    PinnedBuf<float> h_out_stage;         // staging of get_output_data (allocated on first use)
    bool rows_in_stage = false;           // the current block's PLAIN rows were written straight into h_out_stage by the delta
                                          // kernel (set by a plain apply only; cleared by set_input and flush)
    hipEvent_t ev_copy[16] = {};          // chunk events of the pipelined device-to-host copy
};

// VTLN sweep (mfx_apply_alphas): one filterbank (`tables`), one static and one output block per alpha: mfx_stream.cpp
struct SweepState {
    CepTables tables;                     // of the last sweep's alphas
    int cap = 0;                          // alphas the sweep buffers hold
    int n = 0;                            // alphas of the current block's last sweep (0: none since set_input / flush)
    DevBuf<float> d_src, d_blk, d_stats;
    DevBuf<mfx::Segment> d_segs;          // [2][cap]: rows with context, rows delivered
    PinnedBuf<float> h_stage;             // staging of get_output_data_alpha: never st.h_out_stage, which may hold the plain
                                          // rows a later get_output_data returns
};

// batch plan and what hangs on it: mfx_batch_plan.cpp builds it, mfx_batch_attach.cpp attaches to it, mfx_batch.cpp runs it
struct BatchState {
    // ---- the plan proper
    bool planned = false;                // mfx_batch_plan / mfx_batch_plan_rates has succeeded
    int32_t n_utt = 0;
    int64_t total_rows = 0;
    std::vector<int64_t> utt_off, utt_len, utt_row;
    std::vector<int64_t> utt_frames;     // [n_utt] rows of every utterance
    std::vector<mfx::Chunk> h_chunks;
    std::vector<int32_t> chunk_utt;      // utterance of every entry of h_chunks
    std::vector<int32_t> utt_chunk0;     // [n_utt + 1] first chunk of every utterance (chunks are in utterance order)
    DevBuf<mfx::Chunk> d_chunks;
    DevBuf<mfx::Segment> d_segs;
    DevBuf<float> d_stats, d_spec_slab;
    DevBuf<float> d_logmel;      // TRAPS: log mel rows [total_rows][mel_pitch] between the front end and k_traps
    int mel_pitch = 0;
    std::vector<mfx::StftChunk> h_stft_chunks; // STFT log-mel: one per entry of h_chunks (which keep the utterance slicing working)
    DevBuf<mfx::StftChunk> d_stft_chunks;
    DevBuf<float> d_stft_max;    // [chunks] the blocks' largest log values (k_stft_post)
    DevBuf<float> d_static16[2]; // compact [rows][16] statics between front end and delta (double buffered for overlap)
    int tiles_max = 0;
    bool aligned = true;                 // frames on aligned sample pairs (fill_front / choose_front read it)

    // Ten attachments, each tied to the plan: a new plan drops them.  drop() switches one off and releases what is not kept
    // for the next one (the grown-never-shrunk scratch stays); release() names every buffer once, for the clear entry (and a
    // setter that ran out of memory); sized() says whether the scratch a run writes to holds the plan's rows (batch_run_range
    // refuses otherwise).

    // sample-rate conversion (mfx_batch_plan_rates): while on, the run converts the caller's array into d_pcm with one
    // launch of k_resample and then does what it always does on d_pcm; utt_off / utt_len above describe the scratch, in_off /
    // in_len the caller's array
    struct Rates {
        bool on = false;
        std::vector<int64_t> in_off, in_len;
        std::vector<int32_t> utt_tile0;  // [n_utt + 1] first tile of every utterance (tiles are in utterance order)
        int64_t total = 0;               // samples per channel of the scratch (even)
        mfx::ResLds lds{};               // LDS parts of the launch: maxima over the plan's rates
        DevBuf<int16_t> d_pcm;           // [total * channels + 8]
        DevBuf<float> d_taps;
        DevBuf<mfx::ResRate> d_rates;
        DevBuf<mfx::ResTile> d_tiles;
        void drop() // (the converter of a rates plan goes with the plan)
        {
            on = false;
            d_pcm.release(), d_taps.release(), d_rates.release(), d_tiles.release();
        }
    } rs;
    // per-utterance warp factors (mfx_batch_set_alphas): one table per distinct factor and, per table, the row runs of its
    // utterances (build_alpha_runs); the batch then runs spectrum slab + k_melcep_runs / k_plp_runs
    struct Alphas {
        bool on = false;                 // (batch_front reads it)
        CepTables tables;
        std::vector<int32_t> h_run_off;  // [tables + 1]
        std::vector<int64_t> h_runs;     // [runs][2]
        DevBuf<int32_t> d_run_off;
        DevBuf<int64_t> d_runs;
        void drop() { on = false; }
    } va;
    // splice + affine transform (mfx_batch_set_transform): while on, the run writes its rows to d_y and k_splice_affine turns
    // them into the caller's d_out as the last launch
    struct Xform {
        bool on = false;
        int left = 0, right = 0, out = 0;
        DevBuf<float> d_ops, d_bias;     // [n_xf][steps][tiles][64], [n_xf][tiles * 16]
        DevBuf<int32_t> d_idx;           // [n_utt] transform of every utterance (empty: all 0)
        DevBuf<float> d_y;               // [total_rows][Wy] (grown, never shrunk: only the (NULL, 0) setter releases it)
        void drop() { on = false; }
        void release() { d_ops.release(), d_bias.release(), d_idx.release(), d_y.release(); }
        bool sized(size_t total_rows, int Wy) const { return !on || d_y.n >= total_rows * Wy; }
    } xf;
    // per-speaker normalisation (mfx_batch_set_speakers): while on, the run's normaliser is k_spk_sums -> k_spk_finish ->
    // k_spk_apply over the whole batch instead of run_norm's per-utterance kernels
    struct Speakers {
        bool on = false;
        bool ran = false;                // a run has filled the accumulators since the list was set
        int32_t n_spk = 0, mode = 0, n_tiles = 0, max_rows = 0;
        DevBuf<int32_t> d_off, d_list;   // [n_spk + 1], [utterances with frames] (build_speaker_lists)
        DevBuf<int32_t> d_chunk0;        // [n_utt + 1] first chunk of every utterance: item0 of the tiling at kNormChunkRows
        DevBuf<double> d_partial;        // [chunks][4][Wn]
        DevBuf<int64_t> d_prior_n, d_count; // [n_spk] (the prior's: empty without one)
        DevBuf<double> d_prior, d_acc;   // [n_spk][4][Wn]
        DevBuf<float> d_stats;           // [n_spk][2][Wn]
        DevBuf<mfx::SpkTile> d_tiles;    // k_spk_apply's tiles: whole rows of one utterance
        void drop() { on = false; }
    } spk;
    // energy VAD + voiced-frame selection (mfx_batch_set_vad): while on, the run's last stage writes to d_rows instead of the
    // caller's array (modes SELECT / PACK) and the launches of launch_vad follow it on the tail's stream
    struct Vad {
        bool on = false;
        bool ran = false;                // a run has filled the arrays since the setter
        int32_t column = 0, ctx = 0, mode = 0; // (column resolved: never -1)
        float et = 0.f, ms = 0.f, prop = 0.f;
        UttTilingBuf tiles, chunks;      // at kVadTileRows, kNormChunkRows
        DevBuf<double> d_partial;        // [chunks]
        DevBuf<float> d_thr;             // [n_utt]
        DevBuf<int32_t> d_voiced, d_tile_base; // [n_utt], [tiles]
        DevBuf<uint8_t> d_flags;         // [total_rows]
        DevBuf<uint64_t> d_mask;         // [tiles]
        DevBuf<int64_t> d_packed;        // [n_utt + 1]
        DevBuf<float> d_rows;            // [total_rows][Wo] (grown, never shrunk: only mfx_batch_clear_vad releases it)
        hipStream_t last_stream = nullptr; // the stream the last run's tail ran on
        void drop() { on = false, ran = false; }
        void release()
        {
            tiles.release(), chunks.release(), d_partial.release(), d_thr.release(), d_voiced.release(), d_tile_base.release();
            d_flags.release(), d_mask.release(), d_packed.release(), d_rows.release();
        }
        bool sized(size_t total_rows, int Wo) const { return !on || mode == MFX_VAD_FLAGS || d_rows.n >= total_rows * Wo; }
    } vad;
    // online (causal, sliding-window) CMN / CVN (mfx_batch_set_online_norm): while on, everything ahead of the normaliser's
    // place writes to d_raw instead of the run's d_out, and k_onorm_totals -> k_onorm_offsets -> k_onorm_apply turn the Wn
    // columns of d_raw into d_out in run_norm's place
    struct Onorm {
        bool on = false;
        int32_t window = 0, prior_frames = 0;
        int64_t prior_count = 0;
        UttTilingBuf chunks;             // at kOnormChunk
        DevBuf<double> d_prior;          // [2][Wn] (empty without a prior)
        DevBuf<double> d_tot;            // [chunks][2][Wn]
        DevBuf<float> d_raw;             // [total_rows][width] (grown, never shrunk: only mfx_batch_clear_online_norm releases it)
        void drop() { on = false; }
        void release() { chunks.release(), d_prior.release(), d_tot.release(), d_raw.release(); }
        bool sized(size_t total_rows, int width) const { return !on || d_raw.n >= total_rows * width; }
    } on;
    // sliding-window CMN / CVN (mfx_batch_set_sliding_norm; norm = NONE handles): while on, everything up to and including
    // the pitch paste writes the rows y to d_raw instead of where they go today (RunMode::d_raw, mfx_batch.cpp), and
    // k_onorm_totals -> k_onorm_offsets -> k_slide_apply turn all Wy columns of d_raw into the rows the transform and the
    // tensor output read.  The VAD's decision keeps reading d_raw.
    struct Slide {
        bool on = false;
        int32_t window = 0, min_window = 0, center = 0, norm_vars = 0;
        int32_t Wy = 0;                  // the row width the scratch was sized for
        UttTilingBuf chunks;             // at kOnormChunk
        DevBuf<double> d_tot;            // [chunks][2][Wy]
        DevBuf<float> d_raw;             // [total_rows][Wy] (grown, never shrunk: only mfx_batch_clear_sliding_norm releases it)
        void drop() { on = false; }
        void release() { chunks.release(), d_tot.release(), d_raw.release(); }
        bool sized(size_t total_rows, int width) const { return !on || (Wy == width && d_raw.n >= total_rows * width); }
    } sl;
    // pitch track (mfx_batch_set_pitch): while on, k_pitch_nccf and k_pitch_track follow the front end on the handle's stream
    // and fill the handle-owned arrays below, indexed by the plan's rows; d_out is untouched
    struct Pitch {
        bool on = false;
        bool ran = false;                // a run has filled the arrays since the setter
        int32_t window = 0, lag_min = 0, lag_max = 0, K = 0, J = 0;
        float ballast = 0.f, penalty = 0.f;
        UttTilingBuf tiles;              // at pitch_tile_frames
        DevBuf<int64_t> d_utt;           // [n_utt][2] first sample and samples of every utterance, as the front end reads them
        DevBuf<float> d_wt, d_lg;        // [K]
        DevBuf<float> d_nccf;            // [total_rows][K]
        DevBuf<uint16_t> d_bp;           // [total_rows][K]
        DevBuf<float> d_pitch;           // [total_rows][2]
        DevBuf<int32_t> d_index;         // [total_rows]
        void drop() { on = false, ran = false; }
        void release()
        {
            tiles.release(), d_utt.release(), d_wt.release(), d_lg.release(), d_nccf.release(), d_bp.release();
            d_pitch.release(), d_index.release();
        }
        bool sized(size_t total_rows) const { return !on || d_nccf.n >= total_rows * K; }
    } pt;
    // pitch features (mfx_batch_set_pitch_feats; needs the pitch track): while on, k_pitch_feats follows k_pitch_track on the
    // handle's stream and fills d_feats, indexed by the plan's rows.  With `paste` the rows y of a run are Wy = width + F wide:
    // everything ahead of the transform builds its `width` columns in d_narrow, and k_pitch_paste writes [ narrow | feats ]
    // where the rows y go (RunMode::d_y, mfx_batch.cpp)
    struct PitchFeats {
        bool on = false;
        bool ran = false;                // a run has filled d_feats since the setter
        bool paste = false;
        int32_t columns = 0, F = 0, left = 0, right = 0, D = 0;
        float pov_scale = 0.f, pov_offset = 0.f, pitch_scale = 0.f, delta_scale = 0.f;
        double den = 0.0;
        UttTilingBuf tiles;              // at kPitchFeatRows
        DevBuf<float> d_feats;           // [total_rows][F]
        DevBuf<float> d_narrow;          // [total_rows][width] (paste only)
        void drop() { on = false, ran = false, paste = false; }
        void release() { tiles.release(), d_feats.release(), d_narrow.release(); }
        bool sized(size_t total_rows, int width, bool track_on) const
        {
            return !on || (track_on && d_feats.n >= total_rows * F && (!paste || d_narrow.n >= total_rows * width));
        }
    } pf;
    // dense padded tensor output (mfx_batch_set_tensor; set LAST): while on, the run's last stage -- the VAD's selection
    // included -- writes its rows to d_rows instead of the caller's array, and k_tensor_pack turns them into the caller's
    // tensor as the last launch on the tail's stream
    struct Tensor {
        bool on = false;
        bool ran = false;                // a run has written d_len since the setter
        int32_t layout = 0, dtype = 0, Tp = 0, Wo = 0; // (Wo: the output width the scratch was sized for)
        float pad = 0.f;
        DevBuf<float> d_rows;            // [total_rows][Wo] (grown, never shrunk: only mfx_batch_clear_tensor releases it)
        DevBuf<int32_t> d_len;           // [n_utt] min(L_u, Tp); the setter leaves the plan's values
        DevBuf<mfx::TensorUtt> d_utt;    // [n_utt] first row and rows of every utterance
        void drop() { on = false, ran = false; }
        void release() { d_rows.release(), d_len.release(), d_utt.release(); }
        bool sized(size_t total_rows, int width) const { return !on || (Wo == width && d_rows.n >= total_rows * width); }
    } tn;
    // what a new utterance list invalidates (the converter is mfx_batch_plan's to drop: mfx_batch_plan_rates plans through
    // plan_batch too)
    void detach() { va.drop(), xf.drop(), spk.drop(), vad.drop(), on.drop(), sl.drop(), pt.drop(), pf.drop(), tn.drop(); }

    // ---- not tied to the plan
    // optional overlap of the delta/normalisation tail of batch i with the front end of batch i+1 (mfx_batch_overlap)
    struct Overlap {
        bool enabled = false;
        hipStream_t stream2 = nullptr;
        hipEvent_t ev_front[2] = {nullptr, nullptr}, ev_tail[2] = {nullptr, nullptr};
        bool tail_pending[2] = {false, false};
        unsigned seq = 0;
    } ov;
    // mfx_batch_run_host: device copies of the caller's host buffers; sliced runs upload / download beside the kernels
    struct Host {
        hipStream_t stream_up = nullptr, stream_dn = nullptr;
        hipEvent_t ev_up[16] = {}, ev_run[16] = {};
        DevBuf<int16_t> d_pcm;
        DevBuf<float> d_out;
    } host;
};

// fused delta stage of the 512-point kernel: per-block chunk lists (own rows + halo) and delta tiles: mfx_batch.cpp
struct FuseState {
    bool enabled = false; // mfx_config.engine & MFX_ENGINE_FUSE_DELTA: the fused delta stage on every batch that qualifies
    bool off = false;     // MFX_ENGINE_NO_FUSE_DELTA: never.  Neither bit: batches of kFuseMinFrames .. kFuseMaxFrames frames, with no
                          // attachment and no overlap in force (decide_mode), and never at the price of the host entry's slices
    int share = 1;        // FrontParams::dshare of a run whose orders fit (MFX_ENGINE_FUSE_NO_SHARE 0, MFX_ENGINE_FUSE_SHARE_ALL 2)
    bool planned = false;
    int64_t runs = 0;     // fused launches since the handle was created (mfx_batch_fuse_info)
    int blocks = 0, done_words = 0;
    int32_t nchunks = 0;
    DevBuf<mfx::Chunk> d_chunks;
    DevBuf<int32_t> d_blk_chunk_off, d_blk_tile_off, d_err;
    DevBuf<mfx::DeltaTile> d_tiles;
};

// session entries (mfx_sessions_*): per-session carry state in two slot arrays, the pending push (`push`): mfx_sessions_host.cpp
struct SessState {
    int32_t n = 0, max_push = 0;         // sessions; samples per channel one push may bring a session (n == 0: not created)
    int64_t pcm_stride = 0;              // samples per channel of a slot's PCM part (a multiple of 8)
    int32_t frames_max = 0;              // frames one push can complete for one session
    int32_t row_cap = 0, row_floats = 0; // a slot's statics part: rows (2 D carried + frames_max), floats per row
    DevBuf<int16_t> d_pcm;               // [2][n][pcm_stride * channels] (+ slack for whole-word reads)
    DevBuf<float> d_stat;                // [2][n][row_cap][row_floats]
    DevBuf<float> d_slab;                // spectrum rows of the slab path (PLP, long transforms)
    int64_t slab_rows = 0;
    DevBuf<char> d_desc;                 // one push's upload, desc_bytes of it: the parts SessUpload lays out (mfx_sessions_host.cpp)
    PinnedBuf<char> h_stage[2];          // its staging, double buffered
    hipEvent_t ev_stage[2] = {};         // recorded behind the upload that reads h_stage[i]
    bool stage_used[2] = {false, false};
    int stage_cur = 0;
    size_t desc_bytes = 0;
    DevBuf<int16_t> d_host_pcm;          // mfx_sessions_run_host: device copies of the caller's host buffers (grown on demand)
    DevBuf<float> d_host_out;
    struct Live {
        int64_t n = 0, E = 0;            // samples received, rows delivered
        int64_t f0 = 0;                  // frame whose statics are row 0 of the slot
        int32_t tail_off = 0;            // samples from the slot's base to the first frame not yet computed
        int32_t pitch = 0;               // floats per row the slot's statics were written with
        int32_t parity = 0;              // which of the two slot arrays holds the state
        // session transform (E above is then Ey, the finished rows y): transformed rows delivered, the stream row that is
        // row 0 of the y slot, the session's transform (kept across final pushes and mfx_sessions_reset)
        int64_t Ex = 0, y0 = 0;
        int32_t xf = 0;
        // session rates (n above is then J, the converted samples): input samples received, the session's rate (kept across
        // final pushes and mfx_sessions_reset), which of the two carry slot arrays holds its input tail
        int64_t n_in = 0;
        int32_t rate = 0, rs_parity = 0;
    };
    std::vector<Live> live;
    // online normaliser (mfx_sessions_set_online_norm: parameters only; mfx_sessions_create sizes the state)
    struct Onorm {
        bool set = false;
        int32_t window = 0, prior_frames = 0;
        int64_t prior_count = 0;
        std::vector<double> prior;       // [2][Wn] (empty without a prior)
        DevBuf<double> d_prior, d_state; // [2][Wn]; [n][8][Wn] lead / trail O and I of v and q
        DevBuf<float> d_ring;            // [n][window][Wn] the last `window` raw rows of every session
        void release() { d_prior.release(), d_state.release(), d_ring.release(); }
    } on;
    // splice + affine transform (mfx_sessions_set_transform: the host-side operands; mfx_sessions_create uploads them and sizes
    // the y slots): while set, the delta stage writes the rows y of a push into the session's current y slot behind the rows
    // carried from the previous one, and k_sess_xform (k_splice_affine under MFX_ENGINE_SESS_XFORM_PLAIN) turns them into d_out
    struct Xform {
        bool set = false;
        int32_t left = 0, right = 0, out = 0, n_xf = 0;
        int32_t G = 0;                   // row groups per block of k_sess_xform at this shape (sess_xform_tile_rows / 16)
        std::vector<float> ops, bias;    // [n_xf][steps][tiles][64], [n_xf][tiles * 16]
        DevBuf<float> d_ops, d_bias;
        DevBuf<float> d_y;               // [2][n][y_cap][width]
        int32_t y_cap = 0;               // rows of a y slot: left + right + frames_max + D
        void release() { d_ops.release(), d_bias.release(), d_y.release(); }
    } xf;
    // sample-rate conversion in front of a push (mfx_sessions_set_rates: the host-side tables; mfx_sessions_create uploads them
    // and sizes the carry slots and the scratch): while set, lengths and offsets of a push are in input-rate samples, and a
    // push with a piece to convert runs k_sess_resample first: every piece's converted samples go to d_conv (pieces in the
    // caller's order, each on an even sample), which k_sess_gather then reads in the place of the caller's array
    struct Rates {
        bool set = false;
        std::vector<int32_t> hz;
        std::vector<mfx::ResRate> rates; // one per rate; tile_out == 0: pass-through (the rate is sample_rate)
        std::vector<float> taps;
        mfx::ResLds lds{0, 8, 2};        // LDS parts of the launch: maxima over the rates
        int32_t carry_cap = 0;           // samples per channel of a carry slot: max over rates (2 Wh + M div L + 2), a multiple of 8
        int32_t tile_min = 0;            // the smallest tile_out (kResCopyTile for a pass-through rate)
        int64_t conv_stride = 0;         // samples per channel one piece has in the scratch (max_conv rounded up to even)
        DevBuf<float> d_taps;
        DevBuf<mfx::ResRate> d_rates;
        DevBuf<int16_t> d_carry;         // [2][n][carry_cap * channels]
        DevBuf<int16_t> d_conv;          // [n][conv_stride * channels] (+ slack for whole-word reads)
        std::vector<int64_t> last_off, last_len; // the pieces of the last push that converted, in the scratch
        bool last_valid = false;
        void release() { d_taps.release(), d_rates.release(), d_carry.release(), d_conv.release(); }
    } rs;
    int32_t max_conv = 0;                // samples per channel the front end can receive from one piece (max_push without rates)
    // STFT log-mel handles ("Session log-mel"): the slots carry PCM only; k_sess_stft_mel (k_stft_mel under
    // MFX_ENGINE_SESS_STFT_PLAIN) reads the current slots and writes the delivered rows where the delta stage would
    int32_t stft_G = 0;                  // groups per block of k_sess_stft_mel at this shape (sess_stft_groups)
    DevBuf<float> d_stft_max;            // MFX_ENGINE_SESS_STFT_PLAIN: the slots k_stft_mel leaves its blocks' maxima in (not read)
    // the pending push: everything mfx_sessions_plan leaves for mfx_sessions_run_* (which consumes it)
    struct Piece {                       // one entry of the caller's lists
        int32_t id = 0;
        bool fin = false;
        Live next;                       // state of `id` once the run has queued its launches (id and next: all the commit reads)
        int64_t off = 0, len = 0;        // what the front end sees: the caller's piece, or the converted piece in the scratch
        int64_t n_in_next = 0;           // session rates: input samples once the push has run, and the carry parity
        int32_t rs_parity_next = 0;
        int64_t row = 0;                 // first row of d_out the piece delivers to
        int64_t xsrc = 0;                // session transform: absolute row of y[Ex_old] in d_y (set where the piece delivers rows)
        mfx::SessionStep step;
        mfx::SessionXformStep xstep;     // (session transform only)
        // STFT log-mel handles only (`step` then holds n_out and the carried samples, nothing else): the step; the row of
        // d_out, or of the y slots, the piece's first frame goes to; the element of the slot arrays where stream sample 0 lies
        // or would lie (the last two are set where the piece moves, computes or delivers something)
        mfx::SessionStftStep sstep;
        int64_t stft_row = 0, stft_pcm = 0;
    };
    struct Push {
        bool planned = false;
        std::vector<Piece> pieces;       // in the caller's order
        std::vector<int32_t> xf_rows, xf_idx; // by piece: rows the transform delivers, its transform (pack_sess_xform_groups' input)
        // launch-ready, in ascending slots: what SessUpload (mfx_sessions_host.cpp) lays out for the single upload
        std::vector<mfx::SessDesc> descs;
        std::vector<mfx::Segment> segs;
        std::vector<mfx::Chunk> chunks;  // ascending destination rows
        std::vector<int64_t> runs;       // (first row, rows) of every descriptor's new frames, ascending
        int32_t run_off[2] = {0, 0};     // the one table's runs: [0, runs / 2)
        std::vector<mfx::OnormSessDesc> onorm; // rows to normalise
        std::vector<mfx::SessXfGroup> groups;  // the transform's work list: groups and blocks of k_sess_xform, or under
        std::vector<mfx::SessXfBlock> blocks;  // MFX_ENGINE_SESS_XFORM_PLAIN one segment per delivering piece and its transform
        std::vector<mfx::Segment> xsegs;
        std::vector<int32_t> xseg_xf;
        std::vector<mfx::SessResTile> rtiles; // session rates: the tiles of k_sess_resample (empty: nothing to convert or carry)
        std::vector<mfx::StftChunk> stft;     // STFT log-mel: the groups of k_sess_stft_mel (<= 16 frames of one session), or
                                              // under MFX_ENGINE_SESS_STFT_PLAIN the chunks of k_stft_mel (<= stft_R frames)
        std::vector<int64_t> c_off, c_len;    // the pieces after conversion (the caller's own lists when the push converts nothing)
        bool convert = false;            // the pieces lie in the scratch
        bool need_pcm = false;           // a piece brings input samples: the run needs d_pcm
        int64_t total_rows = 0;
        int64_t max_end = 0;             // the largest offsets[i] + lengths[i]: checked against the run's pcm_samples_total
        bool any_new = false;            // a piece brings samples: the run needs d_pcm
        int tiles_max = 0, xtiles_max = 0;
        void clear_lists() { descs.clear(), segs.clear(), chunks.clear(), runs.clear(), onorm.clear(), groups.clear(), blocks.clear(), xsegs.clear(), xseg_xf.clear(), rtiles.clear(), stft.clear(); }
    } push;
    // the planner's scratch (kept so that a plan allocates nothing once warm): ids seen, (slot, piece) keys, the packer's output
    std::vector<uint8_t> p_seen;
    std::vector<int64_t> p_order;
    std::vector<mfx::SessXfCut> p_cuts;
    std::vector<mfx::SessXfPack> p_packs;
    std::vector<int32_t> p_stft_rows;    // (STFT log-mel: rows every piece computes, the cutter's input and output)
    std::vector<mfx::SessStftCut> p_stft_cuts;
    void release() // (what mfx_sessions_create(0, 0) gives back)
    {
        d_pcm.release(), d_stat.release(), d_slab.release(), d_desc.release(), d_host_pcm.release(), d_host_out.release();
        on.release(), xf.release(), rs.release(), h_stage[0].release(), h_stage[1].release(), d_stft_max.release();
    }
};

// profiling of the dominant kernel
struct ProfState {
    bool on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t used = 0;
    int launches = 0;
    double ms = 0;
};

struct mfx_handle {
    mfx_config cfg{};
    int device = 0;
    // A PLANNING handle (mfx_plan_create) runs mfx_create's own code -- the predicates, the host-built tables, the LDS sums
    // that decide which kernels a shape lands on -- with every device call left out: it can answer mfx_dominant_kernel_name
    // and the geometry accessors, and nothing else (no buffer exists; every other entry fails with MFX_ERR_DEVICE).  It is
    // how the shape -> kernel table of DESIGN.md section 5 is pinned by a test that needs no GPU.  It computes nothing.
    bool planning = false;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;

    // ---- shared: geometry and tables, written at create / refresh_mel / set_window only
    // derived (mfccbase.cpp:18-30, mfcccpu.cpp:94-105)
    // cols: static columns of an output row (delta, normalisation, width, statistics); fcols: columns the front end
    // delivers -- the same number except for TRAPS, whose front end is the log-energy form (nb columns) and whose rows
    // hold nb * traps_K statics
    int W = 0, S = 0, W2 = 0, nb = 0, ceps = 0, dl = 0, cols = 0, fcols = 0, width = 0;
    int l1 = 0, l2 = 0, D = 0;
    int input_window_limit = 0, input_buffer_size = 0, window_limit = 0, cap_rows = 0;
    int spec_pitch = 0;
    int channels = 1;
    int num_cus = 256;
    bool fast512 = false;
    bool stuff256 = false; // fast512 serving 256-point transforms in the zero-stuffed form
    bool fast1024 = false; // 1024 points, window <= 512 samples: k_front1024 (two 256-point transforms per frame)
    int nm16 = 16;
    bool plp = false;  // mfx_config.method == MFX_METHOD_PLP: k_plp where MFCC runs k_melcep, never the fused front ends
    int lpc = 0;       // PLP model order (lpc_order, 0 -> 8)
    bool traps = false; // mfx_config.method == MFX_METHOD_TRAPS: fbank front end -> scratch -> k_traps; batch entries only
    int traps_L = 0, traps_K = 0; // trajectory length, coefficients kept (defaults applied)
    // mfx_config.method == MFX_METHOD_STFT_LOGMEL: k_stft_mel (+ k_stft_post) IS the front end; batch entries, and (LOG10 /
    // LN) the session entries through k_sess_stft_mel.  W is the
    // DFT length N (W2 == W), nb the output width; none of the FFT / mel / DCT tables below exist on such a handle
    bool stft = false;
    mfx::StftForm stft_form = mfx::StftForm::None; // Fft (N = 1024 / 2048): k_stft_fft_mel stands where k_stft_mel does; batch entries only
    int stft_R = 0;                      // frames per block of the form's batch kernel (stft_tile_rows)
    DevBuf<float> d_stft_ops;            // basis operands -- FFT form: window and FFT tables -- (mfx_set_window builds them)
    // the mel table of an STFT log-mel or a Kaldi handle (a handle is one or the other; mel_spans below): the rows' spans back to
    // back, and [3][nb]: beg, len, first weight of every row
    DevBuf<float> d_span_melw;
    DevBuf<int32_t> d_span_mel;
    // mfx_config.method == MFX_METHOD_KALDI: k_kaldi_front IS the front end (FrontKind kKaldi), for the batch and the session
    // entries; everything behind it is an MFCC handle's.  W2 is the DFT length kaldi_fft_size(W); none of the FFT / mel / DCT
    // tables below exist on such a handle
    bool kaldi = false;
    float kaldi_preemph = 0.97f;         // the three options (mfx_kaldi_set_options), Kaldi's defaults
    bool kaldi_remove_dc = true, kaldi_use_power = true;
    DevBuf<float> d_kaldi_ops, d_kaldi_dct_t; // window and FFT tables (mfx_set_window builds them); G transposed [nb][ceps] (empty at
                                         // ceps == 0)
    int kaldi_flags = 0;                 // kaldi_flags of mfx_create_kaldi (kKaldi* of mfx_tables.h), checked at creation
    float kaldi_log_floor = -INFINITY;   // (float)log(kaldi_energy_floor), -inf for none
    DevBuf<int64_t> d_kaldi_bounds;      // kKaldiNoSnipEdges: [n_utt][2] first sample and samples of the plan's utterances (a
                                         // chunk's `pad` is its utterance; plan_batch writes both)
    float alpha = 1.f;
    bool have_window = false;

    // tables in HBM
    DevBuf<float> d_win1024o;
    DevBuf<float> d_window, d_winpair, d_twid_pass, d_twid_half, d_twid_split, d_twid_reg, d_dct;
    // k_melcep / k_plp tables of the handle's alpha (also the fused front ends' mel table and 64-lane plan)
    CepTables own;
    // PLP: autocorrelation basis, lifter
    DevBuf<float> d_plp_idft, d_plp_lift;
    // TRAPS: k_traps' operand table (matrix-pipe or vector form, by MFX_ENGINE_TRAPS_VALU)
    DevBuf<float> d_traps_b;
    // k_front512 / k_front1024: the 16-lane plan + the transposed DCT matrix
    MelPlanBuf plan16;
    DevBuf<float> d_dct_t;
    // wave-per-frame kernels (k_front_reg, fused) walk own.plan64; DCT operands for the matrix pipe
    DevBuf<float> d_dct_b;
    DevBuf<float> d_dct_b4;                          // k_front2048: DCT operands as 16-byte words
    DevBuf<float> d_dct_b4s;                         // k_front2048: the split form for <= 40 columns (or empty)
    int dct_split = 0;
    MelPlanBuf plan32;                               // k_front2048: the 32-lane plan
    bool fast2048 = false;
    int dct_tiles = 0, dct_ksteps = 0;
    int dct_stride = 0, nb_pad = 0;
    std::vector<float> h_dct;
    // scratch both interfaces use
    DevBuf<float> d_spec;                // streaming spectrum (mfx_debug_read kind 3); the batch runner hands it to dev-build stamps
    DevBuf<double> d_norm_partial;       // chunk results of the normaliser's statistics (segments longer than 4096 rows)

    StreamState st;
    SweepState sweep;
    BatchState batch;
    FuseState fuse;
    SessState sess;
    ProfState prof;

    // buffers of the handle go through these two: a planning handle records sizes and touches no device
    template <class T>
    hipError_t alloc(DevBuf<T> &b, size_t count)
    {
        return b.alloc(count, !planning);
    }
    template <class T>
    hipError_t upload(DevBuf<T> &b, const std::vector<T> &v)
    {
        hipError_t e = alloc(b, v.size());
        if (e != hipSuccess || v.empty() || planning) return e;
        return hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }

    // (the buffers free themselves after this; mfx_destroy has waited for the streams)
    ~mfx_handle()
    {
        for (auto &ev : prof.events) {
            (void)hipEventDestroy(ev.first);
            (void)hipEventDestroy(ev.second);
        }
        auto destroy = [](auto &events) {
            for (hipEvent_t e : events)
                if (e) (void)hipEventDestroy(e);
        };
        destroy(batch.ov.ev_front), destroy(batch.ov.ev_tail), destroy(batch.host.ev_up), destroy(batch.host.ev_run), destroy(st.ev_copy),
            destroy(sess.ev_stage);
        for (hipStream_t s : {batch.ov.stream2, batch.host.stream_up, batch.host.stream_dn})
            if (s) (void)hipStreamDestroy(s);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};

inline int fail(mfx_handle *h, int code, const std::string &msg)
{
    if (h) h->err = msg;
    return code;
}

inline int fail_hip(mfx_handle *h, hipError_t e, const char *what)
{
    std::string m = std::string(what) + ": " + hipGetErrorString(e);
    return fail(h, MFX_ERR_DEVICE, m);
}

#define HIP_TRY(h, expr)                                         \
    do {                                                         \
        hipError_t _e = (expr);                                  \
        if (_e != hipSuccess) return fail_hip((h), _e, #expr);   \
    } while (0)

// the handle's device current and its streams idle: ahead of everything that replaces, releases or reads back what a run in
// flight may use
inline int sync_device(mfx_handle *h)
{
    HIP_TRY(h, hipSetDevice(h->device));
    return mfx_synchronize(h);
}

inline int UttTilingBuf::set(mfx_handle *h, int32_t rows_per_item)
{
    std::vector<int32_t> i0, iu;
    if (!mfx::build_utt_tiling(h->batch.utt_frames.data(), h->batch.n_utt, rows_per_item, i0, &iu)) return fail(h, MFX_ERR_ARG, "batch too long");
    HIP_TRY(h, h->upload(d_item0, i0));
    HIP_TRY(h, h->upload(d_item_utt, iu));
    item0.swap(i0);
    rows = rows_per_item;
    return MFX_OK;
}

inline int MelPlanBuf::set(mfx_handle *h, const mfx::MelPlan *plans, int count)
{
    ok = false;
    shape(plans, count);
    const size_t lanes = (size_t)plans[0].lanes, meta = lanes * rounds;
    std::vector<float> pw(count * lanes * row_stride, 0.f);
    std::vector<int32_t> pst(count * meta), pfid(count * meta), pL((size_t)count * 8);
    for (int a = 0; a < count; ++a) {
        const mfx::MelPlan &pl = plans[a];
        for (size_t j = 0; j < lanes; ++j)
            std::copy(pl.w.begin() + j * pl.row_stride, pl.w.begin() + (j + 1) * pl.row_stride, pw.begin() + (a * lanes + j) * row_stride);
        std::copy(pl.start.begin(), pl.start.end(), pst.begin() + a * meta);
        std::copy(pl.fid.begin(), pl.fid.end(), pfid.begin() + a * meta);
        std::copy(pl.L, pl.L + 8, pL.begin() + (size_t)a * 8);
    }
    HIP_TRY(h, h->upload(w, pw));
    HIP_TRY(h, h->upload(start, pst));
    HIP_TRY(h, h->upload(fid, pfid));
    HIP_TRY(h, h->upload(L, pL));
    ok = true;
    return MFX_OK;
}

// top of every entry that needs the device: a handle, and not a planning one
#define MFX_DEVICE_ENTRY(h)                                                                                                  \
    do {                                                                                                                     \
        if (!(h)) return MFX_ERR_ARG;                                                                                        \
        if ((h)->planning) return fail((h), MFX_ERR_DEVICE, "planning handle (mfx_plan_create): no device behind it");      \
    } while (0)

// top of every streaming entry: TRAPS handles have none (the streaming state machine's context is D frames, not H)
#define MFX_STREAM_ENTRY(h)                                                                                                  \
    do {                                                                                                                     \
        if ((h)->stft)                                                                                                       \
            return fail((h), MFX_ERR_STATE,                                                                                  \
                        "STFT log-mel handles have batch entries only: use mfx_batch_plan + mfx_batch_run_device / mfx_batch_run_host"); \
        if ((h)->traps)                                                                                                      \
            return fail((h), MFX_ERR_STATE,                                                                                  \
                        "TRAPS handles have no streaming entries: use mfx_batch_plan + mfx_batch_run_device / mfx_batch_run_host"); \
        if ((h)->kaldi)                                                                                                      \
            return fail((h), MFX_ERR_STATE,                                                                                  \
                        "Kaldi handles have no streaming entries: use mfx_batch_plan + mfx_batch_run_device / mfx_batch_run_host, or the session entries"); \
    } while (0)

// one launch of the dominant kernel between two events, while profiling is on (prof_collect, mfx_api.cpp, sums them up)
struct ProfScope {
    mfx_handle *h;
    hipEvent_t a = nullptr, b = nullptr;
    explicit ProfScope(mfx_handle *hh, bool wanted = true) : h(hh)
    {
        if (!wanted || !h->prof.on) return;
        if (h->prof.used == h->prof.events.size()) {
            hipEvent_t x, y;
            if (hipEventCreate(&x) != hipSuccess || hipEventCreate(&y) != hipSuccess) return;
            h->prof.events.emplace_back(x, y);
        }
        a = h->prof.events[h->prof.used].first;
        b = h->prof.events[h->prof.used].second;
        ++h->prof.used;
        (void)hipEventRecord(a, h->stream);
    }
    ~ProfScope()
    {
        if (b) (void)hipEventRecord(b, h->stream);
    }
};

// ---- mfx_api.cpp, for the others
// Which front-end kernel the BATCH entries run for this handle (see choose_front's definition)
// (kKaldi: k_kaldi_front of a Kaldi handle -- no spectrum kind, no slab, no k_melcep: wherever the kind matters it behaves as
// kFrontGenFused)
enum FrontKind { kFront512, kFront1024, kFront2048, kFrontGenFused, kSpec512, kSpecGen, kKaldi };
inline bool is_spec_kind(FrontKind k) { return k == kSpec512 || k == kSpecGen; }
// the fused kinds whose statics can go out as compact 16-float rows (k_front512: only with the DCT on the matrix pipe)
inline bool compact_statics(FrontKind k, const mfx::FrontParams &p) { return !is_spec_kind(k) && (k != kFront512 || p.dct_mode == 1); }
FrontKind choose_front(const mfx_handle *h);
FrontKind choose_front(const mfx_handle *h, bool aligned); // (the session entries: their frames' alignment, not the batch plan's)
// what batch_run_range launches: choose_front's kernel, or the spectrum form while per-utterance warp factors are in force
FrontKind batch_front(const mfx_handle *h);
// What launch_front needs beyond the kernel parameters.  The chunk list in both copies (the spectrum kinds walk the host
// one); for the spectrum kinds the slab and the cepstra step behind every window of it: the row-run form (`runs` set, its
// host copies h_off / h_runs; row0 / rows are the window's, filled in per launch) or plain k_melcep / k_plp with the
// handle's own table over the window's rows, which must then be contiguous.
struct FrontWork {
    const mfx::Chunk *h_chunks = nullptr, *d_chunks = nullptr;
    size_t n_chunks = 0;
    float *slab = nullptr;
    int64_t slab_rows = 0;
    const CepTables *tables = nullptr;
    const int64_t *runs = nullptr, *h_runs = nullptr;
    const int32_t *run_off = nullptr, *h_run_off = nullptr;
    bool profile = false; // every launch of the dominant kernel inside a ProfScope (the batch entries)
};
// queues the front end `kind` on h->stream: p filled but for chunks / n_chunks / spec / spec_pitch
int launch_front(mfx_handle *h, mfx::FrontParams &p, FrontKind kind, bool aligned, const FrontWork &w);
void fill_front(const mfx_handle *h, mfx::FrontParams &p);
void fill_front(const mfx_handle *h, mfx::FrontParams &p, bool aligned);
void fill_traps(const mfx_handle *h, mfx::TrapsParams &p);
int refresh_mel(mfx_handle *h);
int build_cep_tables(mfx_handle *h, const float *alphas, int n, CepTables &t, mfx::MelTable *first = nullptr);
int launch_cepstra(mfx_handle *h, const CepTables &t, const float *spec, int64_t n_rows, float *feat, int feat_pitch,
                   int n_tables, int64_t feat_table_stride, float *r_out, hipStream_t stream);
// the row-run form: the runs of `rr` (host copies h_off / h_runs) of each of t's tables, absolute rows of spec and feat
int launch_cepstra_runs(mfx_handle *h, const CepTables &t, const float *spec, float *feat, int feat_pitch, const mfx::RowRuns &rr,
                        const int32_t *h_off, const int64_t *h_runs, hipStream_t stream);
int run_norm(mfx_handle *h, hipStream_t stream, float *data, int pitch, const mfx::Segment *segs, int n_segs, const mfx::Segment *seg0,
             float *stats, bool use_last, int max_rows, int groups = 1, size_t group_stats_stride = 0);
// ---- mfx_stream.cpp, for mfx_batch.cpp
bool is_pinned_host(const void *p, void **dev_ptr = nullptr);
// ---- mfx_batch*.cpp, for one another and mfx_api.cpp
constexpr int64_t kSlabRowsMax = 1 << 17; // rows of the spectrum slab of the batch entries' spectrum path
// mfx_batch_plan's work, on the layout the front ends will read: the caller's, or the converted PCM's (mfx_batch_plan_rates)
int plan_batch(mfx_handle *h, int32_t n_utt, const int64_t *offsets, const int64_t *lengths, int64_t *out_rows, int64_t *total_rows);
// scratch for the compact statics of the planned batch: one buffer, two with overlap on (grown, never shrunk)
int size_static16(mfx_handle *h);
// width Wy of the rows y of a batch run, which the transform splices and the VAD moves: `width`, and the F pasted columns
// while mfx_batch_set_pitch_feats pastes
inline int batch_y_width(const mfx_handle *h) { return h->width + (h->batch.pf.on && h->batch.pf.paste ? h->batch.pf.F : 0); }
// row width of the batch entries' output: out_dim while a transform is in force, else Wy
int batch_out_width(const mfx_handle *h);
// frames of an utterance of `samples` samples per channel on this handle (may be <= 0 for the framed methods: callers clamp)
inline int64_t utt_frame_count(const mfx_handle *h, int64_t samples)
{
    if (h->kaldi) return mfx::kaldi_frame_count(samples, h->W, h->S, h->kaldi_flags); // (flags 0: frame_count's rule)
    return h->stft ? mfx::stft_frame_count(samples, h->W, h->S) : mfx::frame_count(samples, h->W, h->S);
}
// the mel table of an STFT log-mel or a Kaldi handle as its kernels take it
inline mfx::MelSpans mel_spans(const mfx_handle *h)
{
    const int32_t *meta = h->d_span_mel.p; // [3][nb]
    return mfx::MelSpans{h->d_span_melw.p, meta, meta + h->nb, meta + 2 * h->nb};
}
// what every STFT log-mel kernel takes from the handle: shape, post mode, operands and the mel spans, for rows to `out`
inline mfx::StftCore stft_core(const mfx_handle *h, float *out, int pitch)
{
    return mfx::StftCore{h->W, h->S, h->nb, h->cfg.logmel_post, h->d_stft_ops.p, mel_spans(h), out, pitch};
}
// normalised columns of a speaker list and of the online normaliser: the whole row after the deltas, else the statics
inline int spk_wn(const mfx_handle *h) { return h->cfg.norm_after_dyn ? h->width : h->cols; }
// mfx_batch_set_online_norm / mfx_sessions_set_online_norm: the checks the two setters share (MFX_OK, or the status with the
// message on the handle)
int check_online_norm(mfx_handle *h, const char *who, int32_t window, int32_t prior_frames, int64_t prior_count, const double *prior_acc);
void fill_xform(const mfx_handle *h, mfx::XformParams &p);
// the shape fields XformParams and SessXformParams share, for rows y of `width` floats (pointers and work lists left zero)
template <class P>
inline void fill_xform_shape(const mfx_handle *h, P &p, int width, int left, int right, int out_dim)
{
    p = P{};
    p.width = width, p.left = left, p.right = right, p.out_dim = out_dim;
    p.src_pitch = width, p.out_pitch = out_dim;
    p.valu = (h->cfg.engine & MFX_ENGINE_XFORM_VALU) ? 1 : 0;
}
// the delta stage's shape on this handle: rows of `width` floats out (source, segments and tiles left zero)
inline void fill_delta(const mfx_handle *h, mfx::DeltaParams &dp)
{
    dp = mfx::DeltaParams{};
    dp.out_pitch = h->width;
    dp.cols = h->cols, dp.l1 = h->l1, dp.l2 = h->l2;
}
// row width of the session entries' output: out_dim while a session transform is set, else `width`
inline int sess_out_width(const mfx_handle *h) { return h->sess.xf.set ? h->sess.xf.out : h->width; }
// the VAD's row scratch at the current output width (mfx_batch_attach.cpp; a no-op unless a selecting VAD is in force)
int size_vad_rows(mfx_handle *h);
// bytes a run writes at d_out: the tensor's while one is in force, else total_rows * Wo * 4 (mfx_batch_attach.cpp)
int64_t batch_output_bytes(const mfx_handle *h);
// the one launch of k_tensor_pack over utterances [u0, u1): `rows` [total_rows][Wo] -> the tensor at `out`; lengths from the
// VAD's counts while `voiced` (mfx_batch_attach.cpp)
int run_tensor(mfx_handle *h, hipStream_t stream, const float *rows, void *out, int u0, int u1, bool voiced);
