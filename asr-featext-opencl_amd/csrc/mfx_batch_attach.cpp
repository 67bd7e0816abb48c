// mfx_batch_attach.cpp -- what a caller attaches to a planned batch (include/mfx.h): per-utterance warp factors, a splice +
// affine transform, a speaker list, the energy VAD, the online normaliser, the sliding-window normaliser, the pitch track, the
// pitch features.  Each is tied to the plan (mfx_batch_plan_rates' converter is the tenth, and is the planner's);
// BatchState::detach drops the nine of this file: the eight above and the dense tensor output, which is set last.  This file
// owns `batch.va`, `batch.xf`, `batch.spk`, `batch.vad`, `batch.on`, `batch.sl`, `batch.pt`, `batch.pf` and `batch.tn`.
#include "mfx_handle.h"

#include <cmath>

using namespace mfx;

extern "C" int mfx_batch_set_alphas(mfx_handle *h, const float *alphas, int32_t n_utt)
{
    MFX_DEVICE_ENTRY(h);
    if (!alphas && n_utt == 0) { // back to mfx_set_alpha's factor and choose_front's kernels
        h->batch.va.drop();
        return MFX_OK;
    }
    if (h->stft) return fail(h, MFX_ERR_CONFIG, "mfx_batch_set_alphas: an STFT log-mel handle has no warped Slaney table");
    if (h->kaldi) return fail(h, MFX_ERR_CONFIG, "mfx_batch_set_alphas: a Kaldi handle has no VTLN warp (vtln_warp is not served)");
    if (!alphas || n_utt != h->batch.n_utt) return fail(h, MFX_ERR_ARG, "one warp factor per planned utterance");
    for (int u = 0; u < n_utt; ++u)
        if (!(alphas[u] > 0.f)) return fail(h, MFX_ERR_ARG, "alpha must be positive");
    std::vector<float> tables;
    std::vector<int32_t> off;
    std::vector<int64_t> runs;
    build_alpha_runs(alphas, h->batch.utt_frames.data(), n_utt, tables, off, runs);
    if (tables.size() > 4096) return fail(h, MFX_ERR_ARG, "more than 4096 distinct warp factors");
    int rc = sync_device(h); // (a run in flight may read the tables and lists replaced below)
    if (rc != MFX_OK) return rc;
    h->batch.va.drop();
    if (tables.empty()) return MFX_OK; // (a plan without utterances)
    rc = build_cep_tables(h, tables.data(), (int)tables.size(), h->batch.va.tables);
    if (rc != MFX_OK) return rc;
    if (runs.empty()) runs.assign(2, 0); // (no utterance has a frame: nothing will run; keep the buffers non-null)
    HIP_TRY(h, h->upload(h->batch.va.d_run_off, off));
    HIP_TRY(h, h->upload(h->batch.va.d_runs, runs));
    h->batch.va.h_run_off.swap(off);
    h->batch.va.h_runs.swap(runs);
    // (everything mfx_batch_run_device needs is allocated here: that entry never allocates)
    const size_t slab = (size_t)std::min<int64_t>(h->batch.total_rows, kSlabRowsMax) * h->spec_pitch;
    if (h->batch.d_spec_slab.n < slab) HIP_TRY(h, h->batch.d_spec_slab.alloc(slab));
    h->batch.va.on = true;
    return MFX_OK;
}

// ------------------------------------------------------------------------------------------------
// per-speaker normalisation ("Per-speaker normalisation")
// ------------------------------------------------------------------------------------------------

extern "C" int mfx_batch_set_speakers(mfx_handle *h, const int32_t *utt_spk, int32_t n_utt, int32_t n_spk, const int64_t *prior_count,
                                      const double *prior_acc, int32_t mode)
{
    MFX_DEVICE_ENTRY(h);
    if (h->cfg.norm == MFX_NORM_NONE) return fail(h, MFX_ERR_CONFIG, "mfx_batch_set_speakers: the handle does not normalise (norm = NONE)");
    if (!utt_spk && n_utt == 0) { // back to every utterance's own statistics and run_norm's kernels
        if (const int rc = sync_device(h); rc != MFX_OK) return rc; // (a run in flight may read what a later call replaces)
        h->batch.spk.drop();
        return MFX_OK;
    }
    if (!h->batch.planned) return fail(h, MFX_ERR_STATE, "mfx_batch_set_speakers: no batch is planned");
    if (h->batch.on.on)
        return fail(h, MFX_ERR_STATE, "mfx_batch_set_speakers: the online normaliser is in force (mfx_batch_clear_online_norm first)");
    if (!utt_spk || n_utt != h->batch.n_utt) return fail(h, MFX_ERR_ARG, "one speaker per planned utterance");
    if (n_spk < 1 || n_spk > (1 << 20)) return fail(h, MFX_ERR_ARG, "n_spk must be 1 .. 2^20");
    if ((prior_count == nullptr) != (prior_acc == nullptr)) return fail(h, MFX_ERR_ARG, "a prior is a count AND an accumulator per speaker");
    if (mode != MFX_SPK_POOL && mode != MFX_SPK_PRIOR_ONLY) return fail(h, MFX_ERR_ARG, "mode must be MFX_SPK_POOL or MFX_SPK_PRIOR_ONLY");
    if (mode == MFX_SPK_PRIOR_ONLY && !prior_count) return fail(h, MFX_ERR_ARG, "MFX_SPK_PRIOR_ONLY needs a prior");
    if (prior_count)
        for (int s = 0; s < n_spk; ++s)
            if (prior_count[s] < 0) return fail(h, MFX_ERR_ARG, "negative prior count");
    const std::vector<int64_t> &frames = h->batch.utt_frames;
    std::vector<int32_t> off, list;
    if (!build_speaker_lists(utt_spk, frames.data(), n_utt, n_spk, off, list)) return fail(h, MFX_ERR_ARG, "speaker id outside [0, n_spk)");
    if (mode == MFX_SPK_PRIOR_ONLY)
        for (int s = 0; s < n_spk; ++s)
            if (prior_count[s] == 0 && off[s + 1] > off[s])
                return fail(h, MFX_ERR_ARG, "MFX_SPK_PRIOR_ONLY: a speaker with rows in the batch has a prior of count 0");
    const int Wn = spk_wn(h);
    const int tile_rows = spk_tile_rows(Wn);
    std::vector<int32_t> chunk0; // (k_spk_sums takes the utterance from the grid: no item_utt)
    if (!build_utt_tiling(frames.data(), n_utt, kNormChunkRows, chunk0, nullptr)) return fail(h, MFX_ERR_ARG, "batch too long");
    const size_t chunks = (size_t)chunk0[n_utt];
    std::vector<SpkTile> tiles;
    int64_t max_rows = 0;
    for (int u = 0; u < n_utt; ++u) {
        max_rows = std::max(max_rows, frames[u]);
        if ((frames[u] + tile_rows - 1) / tile_rows + (int64_t)tiles.size() > 0x7ffffff0) return fail(h, MFX_ERR_ARG, "batch too long");
        for (int64_t r = 0; r < frames[u]; r += tile_rows) {
            SpkTile t;
            t.row0 = h->batch.utt_row[u] + r;
            t.rows = (int32_t)std::min<int64_t>(tile_rows, frames[u] - r);
            t.spk = utt_spk[u];
            tiles.push_back(t);
        }
    }
    int rc = sync_device(h); // (a run in flight may read the lists replaced below)
    if (rc != MFX_OK) return rc;
    h->batch.spk.drop();
    h->batch.spk.ran = false;
    // (everything mfx_batch_run_device needs is allocated here: that entry never allocates)
    HIP_TRY(h, h->upload(h->batch.spk.d_off, off));
    HIP_TRY(h, h->upload(h->batch.spk.d_list, list));
    HIP_TRY(h, h->upload(h->batch.spk.d_chunk0, chunk0));
    HIP_TRY(h, h->upload(h->batch.spk.d_tiles, tiles));
    const size_t per = (size_t)4 * Wn;
    if (prior_count) {
        HIP_TRY(h, h->upload(h->batch.spk.d_prior_n, std::vector<int64_t>(prior_count, prior_count + n_spk)));
        HIP_TRY(h, h->upload(h->batch.spk.d_prior, std::vector<double>(prior_acc, prior_acc + (size_t)n_spk * per)));
    } else {
        h->batch.spk.d_prior_n.release(), h->batch.spk.d_prior.release();
    }
    HIP_TRY(h, h->batch.spk.d_partial.alloc(chunks * per));
    HIP_TRY(h, h->batch.spk.d_count.alloc((size_t)n_spk));
    HIP_TRY(h, h->batch.spk.d_acc.alloc((size_t)n_spk * per));
    HIP_TRY(h, h->batch.spk.d_stats.alloc((size_t)n_spk * 2 * Wn));
    h->batch.spk.n_spk = n_spk;
    h->batch.spk.mode = mode;
    h->batch.spk.n_tiles = (int32_t)tiles.size();
    h->batch.spk.max_rows = (int32_t)max_rows;
    h->batch.spk.on = true;
    return MFX_OK;
}

extern "C" int mfx_batch_speaker_stats(mfx_handle *h, int64_t *count, double *acc, float *stats)
{
    MFX_DEVICE_ENTRY(h);
    if (!h->batch.spk.on) return fail(h, MFX_ERR_STATE, "mfx_batch_speaker_stats: no speaker list is in force");
    if (!h->batch.spk.ran) return fail(h, MFX_ERR_STATE, "mfx_batch_speaker_stats: no batch has run since the list was set");
    if (const int rc = sync_device(h); rc != MFX_OK) return rc;
    const size_t n = (size_t)h->batch.spk.n_spk, Wn = (size_t)spk_wn(h);
    if (count) HIP_TRY(h, hipMemcpy(count, h->batch.spk.d_count.p, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (acc) HIP_TRY(h, hipMemcpy(acc, h->batch.spk.d_acc.p, n * 4 * Wn * sizeof(double), hipMemcpyDeviceToHost));
    if (stats) HIP_TRY(h, hipMemcpy(stats, h->batch.spk.d_stats.p, n * 2 * Wn * sizeof(float), hipMemcpyDeviceToHost));
    return MFX_OK;
}

extern "C" int64_t mfx_host_speaker_lists(int32_t n_utt, const int32_t *utt_spk, const int64_t *frames, int32_t n_spk, int32_t *off,
                                          int32_t *list)
{
    if (n_utt < 0 || n_spk < 0 || (n_utt > 0 && (!utt_spk || !frames))) return MFX_ERR_ARG;
    std::vector<int32_t> o, l;
    if (!build_speaker_lists(utt_spk, frames, n_utt, n_spk, o, l)) return MFX_ERR_ARG;
    if (off) std::copy(o.begin(), o.end(), off);
    if (list) std::copy(l.begin(), l.end(), list);
    return (int64_t)l.size();
}

// ------------------------------------------------------------------------------------------------
// online CMN / CVN ("Online normalisation")
// ------------------------------------------------------------------------------------------------

int check_online_norm(mfx_handle *h, const char *who, int32_t window, int32_t prior_frames, int64_t prior_count, const double *prior_acc)
{
    const std::string w(who);
    if (h->cfg.norm != MFX_NORM_CMN && h->cfg.norm != MFX_NORM_CVN)
        return fail(h, MFX_ERR_CONFIG, w + ": the online normaliser serves norm = CMN and CVN only");
    if (spk_wn(h) > 256) return fail(h, MFX_ERR_CONFIG, w + ": more than 256 normalised columns");
    if (window < 0 || window > 4096 || window % kOnormChunk != 0) return fail(h, MFX_ERR_ARG, w + ": window must be 0 or a multiple of 32 in 32 .. 4096");
    if (prior_frames < 0 || prior_frames > (1 << 20)) return fail(h, MFX_ERR_ARG, w + ": prior_frames must be 0 .. 2^20");
    if (prior_count < 0) return fail(h, MFX_ERR_ARG, w + ": negative prior_count");
    if ((prior_acc == nullptr) != (prior_count == 0)) return fail(h, MFX_ERR_ARG, w + ": prior_acc must be NULL exactly when prior_count is 0");
    return MFX_OK;
}

extern "C" int mfx_batch_set_online_norm(mfx_handle *h, int32_t window, int32_t prior_frames, int64_t prior_count, const double *prior_acc)
{
    MFX_DEVICE_ENTRY(h);
    BatchState &B = h->batch;
    int rc = check_online_norm(h, "mfx_batch_set_online_norm", window, prior_frames, prior_count, prior_acc);
    if (rc == MFX_ERR_CONFIG) return rc;
    if (!B.planned) return fail(h, MFX_ERR_STATE, "mfx_batch_set_online_norm: no batch is planned");
    if (rc != MFX_OK) return rc;
    if (B.spk.on) return fail(h, MFX_ERR_STATE, "mfx_batch_set_online_norm: a speaker list is in force (clear it first)");
    const int Wn = spk_wn(h);
    rc = sync_device(h); // (a run in flight may read the lists replaced below)
    if (rc != MFX_OK) return rc;
    BatchState::Onorm &on = B.on;
    on.drop();
    // (everything mfx_batch_run_device needs is allocated here: that entry never allocates)
    if ((rc = on.chunks.set(h, kOnormChunk)) != MFX_OK) return rc;
    if (prior_count > 0)
        HIP_TRY(h, h->upload(on.d_prior, std::vector<double>(prior_acc, prior_acc + (size_t)2 * Wn)));
    else
        on.d_prior.release();
    HIP_TRY(h, on.d_tot.alloc(on.chunks.items() * 2 * Wn));
    const size_t need = (size_t)std::max<int64_t>(B.total_rows, 1) * h->width;
    if (on.d_raw.n < need) HIP_TRY(h, on.d_raw.alloc(need));
    on.window = window, on.prior_frames = prior_frames, on.prior_count = prior_count;
    on.on = true;
    return MFX_OK;
}

extern "C" int mfx_batch_clear_online_norm(mfx_handle *h)
{
    MFX_DEVICE_ENTRY(h);
    if (const int rc = sync_device(h); rc != MFX_OK) return rc; // (a run in flight may read what is released below)
    BatchState::Onorm &on = h->batch.on;
    on.drop();
    on.release();
    return MFX_OK;
}

// ------------------------------------------------------------------------------------------------
// sliding-window CMN / CVN ("Sliding-window normalisation")
// ------------------------------------------------------------------------------------------------

extern "C" int mfx_batch_set_sliding_norm(mfx_handle *h, int32_t window, int32_t min_window, int32_t center, int32_t norm_vars)
{
    MFX_DEVICE_ENTRY(h);
    BatchState &B = h->batch;
    if (h->cfg.norm != MFX_NORM_NONE)
        return fail(h, MFX_ERR_CONFIG, "mfx_batch_set_sliding_norm: the handle normalises already (the sliding window replaces norm, it does not stack on it)");
    if (h->stft) return fail(h, MFX_ERR_CONFIG, "mfx_batch_set_sliding_norm: an STFT log-mel handle is not served");
    const int Wy = batch_y_width(h);
    if (Wy > 256) return fail(h, MFX_ERR_CONFIG, "mfx_batch_set_sliding_norm: more than 256 columns");
    if (!B.planned) return fail(h, MFX_ERR_STATE, "mfx_batch_set_sliding_norm: no batch is planned");
    if (window < 1 || window > 4096) return fail(h, MFX_ERR_ARG, "mfx_batch_set_sliding_norm: window must be 1 .. 4096");
    if (min_window < 0 || min_window > window) return fail(h, MFX_ERR_ARG, "mfx_batch_set_sliding_norm: min_window must be 0 .. window");
    if ((center != 0 && center != 1) || (norm_vars != 0 && norm_vars != 1))
        return fail(h, MFX_ERR_ARG, "mfx_batch_set_sliding_norm: center and norm_vars must be 0 or 1");
    for (const int64_t T : B.utt_frames) // (k_slide_apply forms t + window in 32 bits)
        if (T > 0x7fffffff - 4096) return fail(h, MFX_ERR_ARG, "mfx_batch_set_sliding_norm: utterance too long");
    int rc = sync_device(h); // (a run in flight may read the lists replaced below)
    if (rc != MFX_OK) return rc;
    BatchState::Slide &sl = B.sl;
    sl.drop();
    // (everything mfx_batch_run_device needs is allocated here: that entry never allocates)
    if ((rc = sl.chunks.set(h, kOnormChunk)) != MFX_OK) return rc;
    HIP_TRY(h, sl.d_tot.alloc(sl.chunks.items() * 2 * Wy));
    const size_t need = (size_t)std::max<int64_t>(B.total_rows, 1) * Wy;
    if (sl.d_raw.n < need) HIP_TRY(h, sl.d_raw.alloc(need));
    sl.window = window, sl.min_window = min_window, sl.center = center, sl.norm_vars = norm_vars, sl.Wy = Wy;
    sl.on = true;
    return MFX_OK;
}

extern "C" int mfx_batch_clear_sliding_norm(mfx_handle *h)
{
    MFX_DEVICE_ENTRY(h);
    if (const int rc = sync_device(h); rc != MFX_OK) return rc; // (a run in flight may read what is released below)
    h->batch.sl.drop();
    h->batch.sl.release();
    return MFX_OK;
}

int batch_out_width(const mfx_handle *h) { return h->batch.xf.on ? h->batch.xf.out : batch_y_width(h); }

extern "C" int mfx_batch_output_width(const mfx_handle *h) { return h ? batch_out_width(h) : MFX_ERR_ARG; }

extern "C" int mfx_batch_set_transform(mfx_handle *h, int32_t left, int32_t right, int32_t out_dim, int32_t n_xf, const float *A,
                                       const float *b, const int32_t *utt_xf, int32_t n_utt)
{
    MFX_DEVICE_ENTRY(h);
    if (h->batch.tn.on) return fail(h, MFX_ERR_STATE, "mfx_batch_set_transform: a tensor output is in force (clear the tensor first)");
    if (!A && n_xf == 0) { // back to the rows the handle delivered before, in the caller's d_out
        if (const int rc = sync_device(h); rc != MFX_OK) return rc; // (a run in flight may read what is released below)
        h->batch.xf.drop();
        h->batch.xf.release();
        return size_vad_rows(h); // (the output rows are Wy floats again)
    }
    if (!h->batch.planned) return fail(h, MFX_ERR_STATE, "mfx_batch_set_transform: no batch is planned");
    if (!A) return fail(h, MFX_ERR_ARG, "no matrix");
    if (left < 0 || left > 32 || right < 0 || right > 32) return fail(h, MFX_ERR_ARG, "left and right must be 0 .. 32");
    if (out_dim < 1 || out_dim > 256) return fail(h, MFX_ERR_ARG, "out_dim must be 1 .. 256");
    if (n_xf < 1 || n_xf > 1024) return fail(h, MFX_ERR_ARG, "n_xf must be 1 .. 1024");
    const int64_t in_dim = (int64_t)(left + right + 1) * batch_y_width(h); // (Wy: `width`, and the pasted pitch features)
    if (in_dim > 8192) return fail(h, MFX_ERR_ARG, "in_dim = (left + right + 1) * width is larger than 8192");
    if (utt_xf) {
        if (n_utt != h->batch.n_utt) return fail(h, MFX_ERR_ARG, "one transform index per planned utterance");
        for (int u = 0; u < n_utt; ++u)
            if (utt_xf[u] < 0 || utt_xf[u] >= n_xf) return fail(h, MFX_ERR_ARG, "transform index outside [0, n_xf)");
    }
    XformParams probe;
    fill_xform(h, probe);
    probe.left = left, probe.right = right, probe.out_dim = out_dim;
    // (the limits above leave a tile of 16 rows inside 160 KB at every row width a handle can have; checked all the same)
    if (xform_tile_rows(probe) == 0) return fail(h, MFX_ERR_ARG, "no tile of k_splice_affine fits the LDS for this shape");
    int rc = sync_device(h); // (a run in flight may read the matrices and the index replaced below)
    if (rc != MFX_OK) return rc;
    h->batch.xf.drop();
    const int tiles = (out_dim + 15) / 16, steps = (int)((in_dim + 3) / 4);
    const size_t per = (size_t)steps * tiles * 64;
    std::vector<float> ops(per * n_xf), bias((size_t)n_xf * tiles * 16, 0.f);
    for (int x = 0; x < n_xf; ++x) {
        int tl = 0, st = 0;
        build_xform_operands(A + (size_t)x * out_dim * in_dim, out_dim, (int)in_dim, tl, st, ops.data() + per * x);
        if (b) std::copy(b + (size_t)x * out_dim, b + (size_t)(x + 1) * out_dim, bias.begin() + (size_t)x * tiles * 16);
    }
    HIP_TRY(h, h->upload(h->batch.xf.d_ops, ops));
    HIP_TRY(h, h->upload(h->batch.xf.d_bias, bias));
    if (utt_xf)
        HIP_TRY(h, h->upload(h->batch.xf.d_idx, std::vector<int32_t>(utt_xf, utt_xf + n_utt)));
    else
        h->batch.xf.d_idx.release();
    // (everything mfx_batch_run_device needs is allocated here: that entry never allocates)
    const size_t need = (size_t)std::max<int64_t>(h->batch.total_rows, 1) * batch_y_width(h);
    if (h->batch.xf.d_y.n < need) HIP_TRY(h, h->batch.xf.d_y.alloc(need));
    h->batch.xf.left = left, h->batch.xf.right = right, h->batch.xf.out = out_dim;
    h->batch.xf.on = true;
    return size_vad_rows(h); // (the output rows are out_dim floats now)
}

// ------------------------------------------------------------------------------------------------
// energy VAD + voiced-frame selection ("Voice activity and frame selection")
// ------------------------------------------------------------------------------------------------

// the scratch the last stage writes to while a selecting VAD is in force: [total_rows][Wo] at the CURRENT output width
// (called by the VAD's and the transform's setters, with the streams idle; grown, never shrunk)
int size_vad_rows(mfx_handle *h)
{
    BatchState::Vad &v = h->batch.vad;
    if (!v.on || v.mode == MFX_VAD_FLAGS) return MFX_OK;
    const size_t need = (size_t)std::max<int64_t>(h->batch.total_rows, 1) * batch_out_width(h);
    if (v.d_rows.n < need) HIP_TRY(h, v.d_rows.alloc(need));
    return MFX_OK;
}

extern "C" int mfx_batch_set_vad(mfx_handle *h, int32_t column, float energy_threshold, float energy_mean_scale, int32_t frames_context,
                                 float proportion_threshold, int32_t mode)
{
    MFX_DEVICE_ENTRY(h);
    BatchState &B = h->batch;
    if (B.tn.on) return fail(h, MFX_ERR_STATE, "mfx_batch_set_vad: a tensor output is in force (clear the tensor first)");
    if (!B.planned) return fail(h, MFX_ERR_STATE, "mfx_batch_set_vad: no batch is planned");
    if (column < -1 || column >= h->width) return fail(h, MFX_ERR_ARG, "column must be -1 (the last static column) or inside the row");
    if (frames_context < 0 || frames_context > kVadTileRows) return fail(h, MFX_ERR_ARG, "frames_context must be 0 .. 64");
    if (!(proportion_threshold > 0.f && proportion_threshold <= 1.f)) return fail(h, MFX_ERR_ARG, "proportion_threshold must lie in (0, 1]");
    if (!std::isfinite(energy_threshold) || !std::isfinite(energy_mean_scale))
        return fail(h, MFX_ERR_ARG, "energy_threshold and energy_mean_scale must be finite");
    if (mode != MFX_VAD_FLAGS && mode != MFX_VAD_SELECT && mode != MFX_VAD_PACK)
        return fail(h, MFX_ERR_ARG, "mode must be MFX_VAD_FLAGS, MFX_VAD_SELECT or MFX_VAD_PACK");
    int rc = sync_device(h); // (a run in flight may read the lists replaced below)
    if (rc != MFX_OK) return rc;
    BatchState::Vad &v = B.vad;
    v.drop();
    // (everything mfx_batch_run_device needs is allocated here: that entry never allocates)
    if ((rc = v.tiles.set(h, kVadTileRows)) != MFX_OK || (rc = v.chunks.set(h, kNormChunkRows)) != MFX_OK) return rc;
    const size_t n = (size_t)B.n_utt, tiles = v.tiles.items();
    HIP_TRY(h, v.d_partial.alloc(v.chunks.items()));
    HIP_TRY(h, v.d_mask.alloc(tiles));
    HIP_TRY(h, v.d_tile_base.alloc(tiles));
    // what a run that launches nothing (a batch without rows) leaves for the read-back: no voiced row, thr = energy_threshold
    HIP_TRY(h, h->upload(v.d_thr, std::vector<float>(n, energy_threshold)));
    HIP_TRY(h, h->upload(v.d_voiced, std::vector<int32_t>(n, 0)));
    HIP_TRY(h, h->upload(v.d_packed, std::vector<int64_t>(n + 1, 0)));
    HIP_TRY(h, v.d_flags.alloc((size_t)B.total_rows)); // (every row has a frame: a run writes them all before a read-back)
    v.column = column >= 0 ? column : h->cols - 1;
    v.et = energy_threshold, v.ms = energy_mean_scale, v.ctx = frames_context, v.prop = proportion_threshold, v.mode = mode;
    v.last_stream = h->stream;
    v.on = true;
    const int rs = size_vad_rows(h);
    if (rs != MFX_OK) v.drop();
    return rs;
}

extern "C" int mfx_batch_clear_vad(mfx_handle *h)
{
    MFX_DEVICE_ENTRY(h);
    if (h->batch.tn.on) return fail(h, MFX_ERR_STATE, "mfx_batch_clear_vad: a tensor output is in force (clear the tensor first)");
    if (const int rc = sync_device(h); rc != MFX_OK) return rc; // (a run in flight may read what is released below)
    BatchState::Vad &v = h->batch.vad;
    v.drop();
    v.release();
    return MFX_OK;
}

extern "C" int mfx_batch_vad_read(mfx_handle *h, uint8_t *flags, int32_t *voiced, float *threshold, int64_t *total_voiced)
{
    MFX_DEVICE_ENTRY(h);
    const BatchState::Vad &v = h->batch.vad;
    if (!v.on) return fail(h, MFX_ERR_STATE, "mfx_batch_vad_read: no VAD is in force");
    if (!v.ran) return fail(h, MFX_ERR_STATE, "mfx_batch_vad_read: no batch has run since the VAD was set");
    if (const int rc = sync_device(h); rc != MFX_OK) return rc;
    const size_t n = (size_t)h->batch.n_utt;
    if (flags && h->batch.total_rows > 0) HIP_TRY(h, hipMemcpy(flags, v.d_flags.p, (size_t)h->batch.total_rows, hipMemcpyDeviceToHost));
    if (voiced && n > 0) HIP_TRY(h, hipMemcpy(voiced, v.d_voiced.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (threshold && n > 0) HIP_TRY(h, hipMemcpy(threshold, v.d_thr.p, n * sizeof(float), hipMemcpyDeviceToHost));
    if (total_voiced) HIP_TRY(h, hipMemcpy(total_voiced, v.d_packed.p + n, sizeof(int64_t), hipMemcpyDeviceToHost));
    return MFX_OK;
}

extern "C" int mfx_batch_vad_device(const mfx_handle *h, const uint8_t **d_flags, const int32_t **d_voiced, const int64_t **d_packed_row0)
{
    if (!h) return MFX_ERR_ARG;
    if (h->planning) return MFX_ERR_DEVICE;
    if (!h->batch.vad.on) return MFX_ERR_STATE;
    if (d_flags) *d_flags = h->batch.vad.d_flags.p;
    if (d_voiced) *d_voiced = h->batch.vad.d_voiced.p;
    if (d_packed_row0) *d_packed_row0 = h->batch.vad.d_packed.p;
    return MFX_OK;
}

// ------------------------------------------------------------------------------------------------
// pitch track ("Pitch track")
// ------------------------------------------------------------------------------------------------

extern "C" int mfx_batch_set_pitch(mfx_handle *h, int32_t window, int32_t lag_min, int32_t lag_max, float ballast, float lag_cost,
                                   float penalty, int32_t max_jump)
{
    MFX_DEVICE_ENTRY(h);
    BatchState &B = h->batch;
    if (h->stft) return fail(h, MFX_ERR_CONFIG, "mfx_batch_set_pitch: an STFT log-mel handle frames its utterances centred");
    if (h->kaldi && (h->kaldi_flags & kKaldiNoSnipEdges))
        return fail(h, MFX_ERR_CONFIG,
                    "mfx_batch_set_pitch: a Kaldi handle with MFX_KALDI_NO_SNIP_EDGES frames its utterances centred (the track's frames "
                    "follow the snip-edged rule and would not line up with the rows)");
    if (!B.planned) return fail(h, MFX_ERR_STATE, "mfx_batch_set_pitch: no batch is planned");
    PitchShape s;
    if (!pitch_shape(window == 0 ? h->cfg.window_size : window, lag_min, lag_max, ballast, lag_cost, penalty, max_jump, s))
        return fail(h, MFX_ERR_ARG,
                    "mfx_batch_set_pitch: window 32 .. 1024, lags 2 .. 1024 (at most 512 of them), finite ballast, lag_cost in [0, 1] "
                    "and penalty >= 0, max_jump 0 .. 511");
    const int tile_frames = pitch_tile_frames(s.window, s.lag_max, h->S);
    PitchParams probe{};
    probe.channels = h->channels, probe.tiles.rows = tile_frames;
    probe.window = s.window, probe.shift = h->S, probe.lag_min = s.lag_min, probe.lag_max = s.lag_max, probe.K = s.K, probe.J = s.J;
    probe.span_pad = pitch_span_pad(h->S);
    probe.groups = pitch_groups(s.lag_min, s.lag_max);
    if (!pitch_params_ok(probe)) return fail(h, MFX_ERR_ARG, "mfx_batch_set_pitch: no tile of k_pitch_nccf fits the LDS for this shift");
    std::vector<float> wt, lg;
    build_pitch_tables(s, lag_cost, wt, lg);
    std::vector<int64_t> utt((size_t)2 * B.n_utt);
    for (int u = 0; u < B.n_utt; ++u) utt[2 * (size_t)u] = B.utt_off[u], utt[2 * (size_t)u + 1] = B.utt_len[u];
    if (const int rc = sync_device(h); rc != MFX_OK) return rc; // (a run in flight may read the lists replaced below)
    BatchState::Pitch &pt = B.pt;
    pt.drop();
    // (everything mfx_batch_run_device needs is allocated here: that entry never allocates)
    const size_t rows = (size_t)B.total_rows;
    auto all = [&]() -> int {
        if (const int rt = pt.tiles.set(h, tile_frames); rt != MFX_OK) return rt;
        HIP_TRY(h, h->upload(pt.d_utt, utt));
        HIP_TRY(h, h->upload(pt.d_wt, wt));
        HIP_TRY(h, h->upload(pt.d_lg, lg));
        HIP_TRY(h, pt.d_nccf.alloc(rows * s.K));
        HIP_TRY(h, pt.d_bp.alloc(rows * s.K));
        HIP_TRY(h, pt.d_pitch.alloc(rows * 2));
        HIP_TRY(h, pt.d_index.alloc(rows));
        return MFX_OK;
    };
    if (const int ra = all(); ra != MFX_OK) { // (it did not fit: nothing of it stays)
        pt.release();
        return ra;
    }
    pt.window = s.window, pt.lag_min = s.lag_min, pt.lag_max = s.lag_max, pt.K = s.K, pt.J = s.J;
    pt.ballast = ballast, pt.penalty = penalty;
    pt.on = true;
    return MFX_OK;
}

extern "C" int mfx_batch_clear_pitch(mfx_handle *h)
{
    MFX_DEVICE_ENTRY(h);
    // (the pitch features go with the track they are computed from; pasted, they are part of the rows a transform or a VAD
    // was sized for)
    if (batch_y_width(h) != h->width && (h->batch.xf.on || h->batch.vad.on || h->batch.sl.on))
        return fail(h, MFX_ERR_STATE, "mfx_batch_clear_pitch: pasted pitch features are in force under a transform, a VAD or the sliding-window normaliser (clear those first)");
    if (batch_y_width(h) != h->width && h->batch.tn.on)
        return fail(h, MFX_ERR_STATE, "mfx_batch_clear_pitch: the row width would change under a tensor output (clear the tensor first)");
    if (const int rc = sync_device(h); rc != MFX_OK) return rc; // (a run in flight may read what is released below)
    h->batch.pt.drop();
    h->batch.pt.release();
    h->batch.pf.drop();
    h->batch.pf.release();
    return MFX_OK;
}

extern "C" int mfx_batch_pitch_read(mfx_handle *h, float *pitch, int32_t *index, float *nccf)
{
    MFX_DEVICE_ENTRY(h);
    const BatchState::Pitch &pt = h->batch.pt;
    if (!pt.on) return fail(h, MFX_ERR_STATE, "mfx_batch_pitch_read: no pitch track is in force");
    if (!pt.ran) return fail(h, MFX_ERR_STATE, "mfx_batch_pitch_read: no batch has run since the pitch track was set");
    if (const int rc = sync_device(h); rc != MFX_OK) return rc;
    const size_t rows = (size_t)h->batch.total_rows;
    if (rows == 0) return MFX_OK;
    if (pitch) HIP_TRY(h, hipMemcpy(pitch, pt.d_pitch.p, rows * 2 * sizeof(float), hipMemcpyDeviceToHost));
    if (index) HIP_TRY(h, hipMemcpy(index, pt.d_index.p, rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (nccf) HIP_TRY(h, hipMemcpy(nccf, pt.d_nccf.p, rows * pt.K * sizeof(float), hipMemcpyDeviceToHost));
    return MFX_OK;
}

extern "C" int mfx_batch_pitch_device(const mfx_handle *h, const float **d_pitch, const int32_t **d_index)
{
    if (!h) return MFX_ERR_ARG;
    if (h->planning) return MFX_ERR_DEVICE;
    if (!h->batch.pt.on) return MFX_ERR_STATE;
    if (d_pitch) *d_pitch = h->batch.pt.d_pitch.p;
    if (d_index) *d_index = h->batch.pt.d_index.p;
    return MFX_OK;
}

// ------------------------------------------------------------------------------------------------
// pitch features ("Pitch features")
// ------------------------------------------------------------------------------------------------

extern "C" int mfx_batch_set_pitch_feats(mfx_handle *h, int32_t columns, int32_t left, int32_t right, int32_t delta_window,
                                         float pov_scale, float pov_offset, float pitch_scale, float delta_scale, int32_t paste)
{
    MFX_DEVICE_ENTRY(h);
    BatchState &B = h->batch;
    if (!B.planned) return fail(h, MFX_ERR_STATE, "mfx_batch_set_pitch_feats: no batch is planned");
    if (!B.pt.on) return fail(h, MFX_ERR_STATE, "mfx_batch_set_pitch_feats: no pitch track is in force (mfx_batch_set_pitch first)");
    PitchFeatShape s;
    if ((paste != 0 && paste != 1) || !pitch_feat_shape(columns, left, right, delta_window, pov_scale, pov_offset, pitch_scale, delta_scale, s))
        return fail(h, MFX_ERR_ARG,
                    "mfx_batch_set_pitch_feats: columns 0 or MFX_PF_* bits, left and right 0 .. 1024, delta_window 1 .. 16, finite "
                    "scales, paste 0 or 1");
    if (h->width + (paste ? s.F : 0) != batch_y_width(h) && (B.xf.on || B.vad.on || B.sl.on))
        return fail(h, MFX_ERR_STATE,
                    "mfx_batch_set_pitch_feats: the row width would change under a transform, a VAD or the sliding-window normaliser (clear "
                    "them, set the paste, set them again)");
    if (h->width + (paste ? s.F : 0) != batch_y_width(h) && B.tn.on)
        return fail(h, MFX_ERR_STATE, "mfx_batch_set_pitch_feats: the row width would change under a tensor output (clear the tensor first)");
    if (const int rc = sync_device(h); rc != MFX_OK) return rc; // (a run in flight may read the arrays replaced below)
    BatchState::PitchFeats &pf = B.pf;
    pf.drop();
    // (everything mfx_batch_run_device needs is allocated here: that entry never allocates)
    const size_t rows = (size_t)B.total_rows;
    auto all = [&]() -> int {
        if (const int rt = pf.tiles.set(h, kPitchFeatRows); rt != MFX_OK) return rt;
        HIP_TRY(h, pf.d_feats.alloc(rows * s.F));
        if (paste)
            HIP_TRY(h, pf.d_narrow.alloc(rows * h->width));
        else
            pf.d_narrow.release();
        return MFX_OK;
    };
    if (const int ra = all(); ra != MFX_OK) { // (it did not fit: nothing of it stays)
        pf.release();
        return ra;
    }
    pf.columns = s.columns, pf.F = s.F, pf.left = s.left, pf.right = s.right, pf.D = s.D, pf.den = s.den;
    pf.pov_scale = pov_scale, pf.pov_offset = pov_offset, pf.pitch_scale = pitch_scale, pf.delta_scale = delta_scale;
    pf.paste = paste != 0;
    pf.on = true;
    return MFX_OK;
}

extern "C" int mfx_batch_clear_pitch_feats(mfx_handle *h)
{
    MFX_DEVICE_ENTRY(h);
    if (batch_y_width(h) != h->width && (h->batch.xf.on || h->batch.vad.on || h->batch.sl.on))
        return fail(h, MFX_ERR_STATE, "mfx_batch_clear_pitch_feats: the row width would change under a transform, a VAD or the sliding-window normaliser (clear them first)");
    if (batch_y_width(h) != h->width && h->batch.tn.on)
        return fail(h, MFX_ERR_STATE, "mfx_batch_clear_pitch_feats: the row width would change under a tensor output (clear the tensor first)");
    if (const int rc = sync_device(h); rc != MFX_OK) return rc; // (a run in flight may read what is released below)
    h->batch.pf.drop();
    h->batch.pf.release();
    return MFX_OK;
}

extern "C" int mfx_batch_pitch_feats_read(mfx_handle *h, float *feats)
{
    MFX_DEVICE_ENTRY(h);
    const BatchState::PitchFeats &pf = h->batch.pf;
    if (!pf.on) return fail(h, MFX_ERR_STATE, "mfx_batch_pitch_feats_read: no pitch features are in force");
    if (!pf.ran) return fail(h, MFX_ERR_STATE, "mfx_batch_pitch_feats_read: no batch has run since the pitch features were set");
    if (const int rc = sync_device(h); rc != MFX_OK) return rc;
    const size_t rows = (size_t)h->batch.total_rows;
    if (rows == 0 || !feats) return MFX_OK;
    HIP_TRY(h, hipMemcpy(feats, pf.d_feats.p, rows * pf.F * sizeof(float), hipMemcpyDeviceToHost));
    return MFX_OK;
}

extern "C" int mfx_batch_pitch_feats_device(const mfx_handle *h, const float **d_feats, int32_t *F)
{
    if (!h) return MFX_ERR_ARG;
    if (h->planning) return MFX_ERR_DEVICE;
    if (!h->batch.pf.on) return MFX_ERR_STATE;
    if (d_feats) *d_feats = h->batch.pf.d_feats.p;
    if (F) *F = h->batch.pf.F;
    return MFX_OK;
}

// ------------------------------------------------------------------------------------------------
// dense padded tensor output ("Tensor output")
// ------------------------------------------------------------------------------------------------

int64_t batch_output_bytes(const mfx_handle *h)
{
    const BatchState &B = h->batch;
    if (B.tn.on) return tensor_bytes(B.n_utt, B.tn.Wo, B.tn.Tp, B.tn.dtype);
    return B.total_rows * (int64_t)batch_out_width(h) * (int64_t)sizeof(float);
}

int run_tensor(mfx_handle *h, hipStream_t stream, const float *rows, void *out, int u0, int u1, bool voiced)
{
    BatchState::Tensor &tn = h->batch.tn;
    TensorParams tp{};
    tp.rows = rows;
    tp.out = out;
    tp.utt = tn.d_utt.p;
    tp.voiced = voiced ? h->batch.vad.d_voiced.p : nullptr;
    tp.len = tn.d_len.p;
    tp.u0 = u0, tp.u1 = u1;
    tp.Tp = tn.Tp, tp.Wo = tn.Wo;
    tp.layout = tn.layout, tp.dtype = tn.dtype;
    tp.pad_value = tn.pad;
    HIP_TRY(h, launch_tensor_pack(tp, stream));
    tn.ran = true;
    return MFX_OK;
}

extern "C" int mfx_batch_set_tensor(mfx_handle *h, int32_t layout, int32_t dtype, int32_t t_pad, float pad_value)
{
    MFX_DEVICE_ENTRY(h);
    BatchState &B = h->batch;
    if (!B.planned) return fail(h, MFX_ERR_STATE, "mfx_batch_set_tensor: no batch is planned");
    if (layout != MFX_TENSOR_TIME_MAJOR && layout != MFX_TENSOR_CHANNEL_MAJOR)
        return fail(h, MFX_ERR_ARG, "mfx_batch_set_tensor: layout must be MFX_TENSOR_TIME_MAJOR or MFX_TENSOR_CHANNEL_MAJOR");
    if (dtype != MFX_DTYPE_F32 && dtype != MFX_DTYPE_F16 && dtype != MFX_DTYPE_BF16)
        return fail(h, MFX_ERR_ARG, "mfx_batch_set_tensor: dtype must be MFX_DTYPE_F32, MFX_DTYPE_F16 or MFX_DTYPE_BF16");
    if (t_pad < 0 || t_pad > kTensorPadMax) return fail(h, MFX_ERR_ARG, "mfx_batch_set_tensor: t_pad must be 0 .. 2^24");
    if (B.vad.on && B.vad.mode == MFX_VAD_PACK)
        return fail(h, MFX_ERR_STATE, "mfx_batch_set_tensor: a packing VAD is in force (packed rows have no per-utterance place)");
    const int Wo = batch_out_width(h);
    int64_t Tp = t_pad;
    if (t_pad == 0)
        for (int u = 0; u < B.n_utt; ++u) Tp = std::max(Tp, B.utt_frames[u]);
    TensorParams probe{};
    probe.u1 = B.n_utt, probe.Tp = (int32_t)std::min<int64_t>(Tp, kTensorPadMax), probe.Wo = Wo, probe.layout = layout, probe.dtype = dtype;
    if (Tp > kTensorPadMax || tensor_bytes(B.n_utt, Wo, Tp, dtype) < 0) return fail(h, MFX_ERR_ARG, "mfx_batch_set_tensor: the tensor is too large");
    if (layout == MFX_TENSOR_CHANNEL_MAJOR && tensor_lds_bytes(Wo) > kLdsCap)
        return fail(h, MFX_ERR_CONFIG, "mfx_batch_set_tensor: no tile of k_tensor_pack fits the LDS at this output width");
    if (!tensor_params_ok(probe)) return fail(h, MFX_ERR_ARG, "mfx_batch_set_tensor: batch too long");
    std::vector<TensorUtt> utt((size_t)B.n_utt);
    std::vector<int32_t> len((size_t)B.n_utt);
    for (int u = 0; u < B.n_utt; ++u) {
        utt[u] = TensorUtt{B.utt_row[u], (int32_t)B.utt_frames[u], 0};
        len[u] = (int32_t)std::min<int64_t>(B.utt_frames[u], Tp);
    }
    if (const int rc = sync_device(h); rc != MFX_OK) return rc; // (a run in flight may read the arrays replaced below)
    BatchState::Tensor &tn = B.tn;
    tn.drop();
    // (everything mfx_batch_run_device needs is allocated here: that entry never allocates)
    auto all = [&]() -> int {
        HIP_TRY(h, h->upload(tn.d_utt, utt));
        HIP_TRY(h, h->upload(tn.d_len, len));
        const size_t need = (size_t)std::max<int64_t>(B.total_rows, 1) * Wo;
        if (tn.d_rows.n < need) HIP_TRY(h, tn.d_rows.alloc(need));
        return MFX_OK;
    };
    if (const int ra = all(); ra != MFX_OK) { // (it did not fit: nothing of it stays)
        tn.release();
        return ra;
    }
    tn.layout = layout, tn.dtype = dtype, tn.Tp = (int32_t)Tp, tn.Wo = Wo, tn.pad = pad_value;
    tn.on = true;
    return MFX_OK;
}

extern "C" int mfx_batch_clear_tensor(mfx_handle *h)
{
    MFX_DEVICE_ENTRY(h);
    if (const int rc = sync_device(h); rc != MFX_OK) return rc; // (a run in flight may read what is released below)
    h->batch.tn.drop();
    h->batch.tn.release();
    return MFX_OK;
}

extern "C" int64_t mfx_batch_output_bytes(const mfx_handle *h)
{
    if (!h) return MFX_ERR_ARG;
    if (h->planning) return MFX_ERR_DEVICE;
    return batch_output_bytes(h);
}

extern "C" int mfx_batch_tensor_shape(const mfx_handle *h, int64_t dims[3], int32_t *elem_bytes)
{
    if (!h) return MFX_ERR_ARG;
    if (h->planning) return MFX_ERR_DEVICE;
    const BatchState::Tensor &tn = h->batch.tn;
    if (!tn.on) return MFX_ERR_STATE;
    if (dims) {
        dims[0] = h->batch.n_utt;
        dims[1] = tn.layout == MFX_TENSOR_TIME_MAJOR ? tn.Tp : tn.Wo;
        dims[2] = tn.layout == MFX_TENSOR_TIME_MAJOR ? tn.Wo : tn.Tp;
    }
    if (elem_bytes) *elem_bytes = tensor_elem_bytes(tn.dtype);
    return MFX_OK;
}

extern "C" int mfx_batch_tensor_lengths(mfx_handle *h, int32_t *len, const int32_t **d_len)
{
    MFX_DEVICE_ENTRY(h);
    const BatchState &B = h->batch;
    if (!B.tn.on) return fail(h, MFX_ERR_STATE, "mfx_batch_tensor_lengths: no tensor output is in force");
    if (B.vad.on && B.vad.mode == MFX_VAD_SELECT && !B.tn.ran)
        return fail(h, MFX_ERR_STATE, "mfx_batch_tensor_lengths: a selecting VAD decides the lengths and no batch has run since the tensor was set");
    if (const int rc = sync_device(h); rc != MFX_OK) return rc;
    if (len && B.n_utt > 0) HIP_TRY(h, hipMemcpy(len, B.tn.d_len.p, (size_t)B.n_utt * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (d_len) *d_len = B.tn.d_len.p;
    return MFX_OK;
}

extern "C" int mfx_batch_tensor_from_rows(mfx_handle *h, const float *d_rows, void *d_out)
{
    MFX_DEVICE_ENTRY(h);
    const BatchState &B = h->batch;
    if (!B.tn.on) return fail(h, MFX_ERR_STATE, "mfx_batch_tensor_from_rows: no tensor output is in force");
    if (B.vad.on) return fail(h, MFX_ERR_STATE, "mfx_batch_tensor_from_rows: a VAD is in force");
    if (batch_output_bytes(h) == 0) return MFX_OK; // (no element to write)
    if (!d_rows || !d_out) return fail(h, MFX_ERR_ARG, "invalid argument");
    if (((uintptr_t)d_rows & 3) != 0 || ((uintptr_t)d_out & (uintptr_t)(tensor_elem_bytes(B.tn.dtype) - 1)) != 0)
        return fail(h, MFX_ERR_ARG, "mfx_batch_tensor_from_rows: d_rows must be 4-byte aligned and d_out aligned to its element");
    HIP_TRY(h, hipSetDevice(h->device));
    return run_tensor(h, h->stream, d_rows, d_out, 0, B.n_utt, false);
}
