// mfx_batch_attach.cpp -- what a caller attaches to a planned batch (include/mfx.h): per-utterance warp factors, a splice +
// affine transform, a speaker list.  Each is tied to the plan (mfx_batch_plan_rates' converter is the fourth, and is the
// planner's); BatchState::detach drops the three of this file.  This file owns `batch.va`, `batch.xf` and `batch.spk`.
#include "mfx_handle.h"

using namespace mfx;

extern "C" int mfx_batch_set_alphas(mfx_handle *h, const float *alphas, int32_t n_utt)
{
    MFX_DEVICE_ENTRY(h);
    if (!alphas && n_utt == 0) { // back to mfx_set_alpha's factor and choose_front's kernels
        h->batch.va.drop();
        return MFX_OK;
    }
    if (!alphas || n_utt != h->batch.n_utt) return fail(h, MFX_ERR_ARG, "one warp factor per planned utterance");
    for (int u = 0; u < n_utt; ++u)
        if (!(alphas[u] > 0.f)) return fail(h, MFX_ERR_ARG, "alpha must be positive");
    std::vector<float> tables;
    std::vector<int32_t> off;
    std::vector<int64_t> runs;
    build_alpha_runs(alphas, h->batch.utt_frames.data(), n_utt, tables, off, runs);
    if (tables.size() > 4096) return fail(h, MFX_ERR_ARG, "more than 4096 distinct warp factors");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = mfx_synchronize(h); // (a run in flight may read the tables and lists replaced below)
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
        HIP_TRY(h, hipSetDevice(h->device));
        const int rc = mfx_synchronize(h); // (a run in flight may read what a later call replaces)
        if (rc != MFX_OK) return rc;
        h->batch.spk.drop();
        return MFX_OK;
    }
    if (!h->batch.planned) return fail(h, MFX_ERR_STATE, "mfx_batch_set_speakers: no batch is planned");
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
    std::vector<int32_t> chunk0((size_t)n_utt + 1);
    std::vector<SpkTile> tiles;
    int64_t chunks = 0, max_rows = 0;
    for (int u = 0; u < n_utt; ++u) {
        chunk0[u] = (int32_t)chunks;
        chunks += spk_chunks(frames[u]);
        max_rows = std::max(max_rows, frames[u]);
        if (chunks > 0x7ffffff0 || (frames[u] + tile_rows - 1) / tile_rows + (int64_t)tiles.size() > 0x7ffffff0)
            return fail(h, MFX_ERR_ARG, "batch too long");
        for (int64_t r = 0; r < frames[u]; r += tile_rows) {
            SpkTile t;
            t.row0 = h->batch.utt_row[u] + r;
            t.rows = (int32_t)std::min<int64_t>(tile_rows, frames[u] - r);
            t.spk = utt_spk[u];
            tiles.push_back(t);
        }
    }
    chunk0[n_utt] = (int32_t)chunks;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = mfx_synchronize(h); // (a run in flight may read the lists replaced below)
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
    HIP_TRY(h, h->batch.spk.d_partial.alloc((size_t)chunks * per));
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
    HIP_TRY(h, hipSetDevice(h->device));
    const int rc = mfx_synchronize(h);
    if (rc != MFX_OK) return rc;
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

int batch_out_width(const mfx_handle *h) { return h->batch.xf.on ? h->batch.xf.out : h->width; }

extern "C" int mfx_batch_output_width(const mfx_handle *h) { return h ? batch_out_width(h) : MFX_ERR_ARG; }

extern "C" int mfx_batch_set_transform(mfx_handle *h, int32_t left, int32_t right, int32_t out_dim, int32_t n_xf, const float *A,
                                       const float *b, const int32_t *utt_xf, int32_t n_utt)
{
    MFX_DEVICE_ENTRY(h);
    if (!A && n_xf == 0) { // back to the rows the handle delivered before, in the caller's d_out
        HIP_TRY(h, hipSetDevice(h->device));
        const int rc = mfx_synchronize(h); // (a run in flight may read what is released below)
        if (rc != MFX_OK) return rc;
        h->batch.xf.drop();
        h->batch.xf.d_ops.release(), h->batch.xf.d_bias.release(), h->batch.xf.d_idx.release(), h->batch.xf.d_y.release();
        return MFX_OK;
    }
    if (!h->batch.planned) return fail(h, MFX_ERR_STATE, "mfx_batch_set_transform: no batch is planned");
    if (!A) return fail(h, MFX_ERR_ARG, "no matrix");
    if (left < 0 || left > 32 || right < 0 || right > 32) return fail(h, MFX_ERR_ARG, "left and right must be 0 .. 32");
    if (out_dim < 1 || out_dim > 256) return fail(h, MFX_ERR_ARG, "out_dim must be 1 .. 256");
    if (n_xf < 1 || n_xf > 1024) return fail(h, MFX_ERR_ARG, "n_xf must be 1 .. 1024");
    const int64_t in_dim = (int64_t)(left + right + 1) * h->width;
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
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = mfx_synchronize(h); // (a run in flight may read the matrices and the index replaced below)
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
    const size_t need = (size_t)std::max<int64_t>(h->batch.total_rows, 1) * h->width;
    if (h->batch.xf.d_y.n < need) HIP_TRY(h, h->batch.xf.d_y.alloc(need));
    h->batch.xf.left = left, h->batch.xf.right = right, h->batch.xf.out = out_dim;
    h->batch.xf.on = true;
    return MFX_OK;
}
