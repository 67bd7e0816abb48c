// mfx_batch.cpp -- the runner of the batch interface of include/mfx.h: a planned batch (mfx_batch_plan.cpp) with what is
// attached to it (mfx_batch_attach.cpp) through the device and host entries, the overlap of a batch's tail with the next
// front end, the pinned allocator.  Which front end runs is choose_front's decision and launch_front's work (mfx_api.cpp).
// This file owns `batch.ov` and `batch.host`; of the rest of `batch` and of `fuse` it only reads, but for spk.ran, vad.ran, pt.ran,
// pf.ran (tn.ran is run_tensor's, mfx_batch_attach.cpp) and the spectrum slab it grows.  It names no field of `st` or `sweep`.
#include "mfx_handle.h"

using namespace mfx;

void fill_xform(const mfx_handle *h, XformParams &p)
{
    fill_xform_shape(h, p, batch_y_width(h), h->batch.xf.left, h->batch.xf.right, h->batch.xf.out);
}

namespace {
// the normaliser of a run while a speaker list is in force: in run_norm's place, on its stream, over the whole batch
int run_speaker_norm(mfx_handle *h, hipStream_t stream, float *data)
{
    SpkParams sp{};
    sp.data = data;
    sp.pitch = h->width;
    sp.cols = h->cols;
    sp.groups = spk_wn(h) / h->cols;
    sp.norm_type = h->cfg.norm;
    sp.mode = h->batch.spk.mode;
    sp.segs = h->batch.d_segs.p;
    sp.n_utt = h->batch.n_utt;
    sp.max_rows = h->batch.spk.max_rows;
    sp.utt_chunk0 = h->batch.spk.d_chunk0.p;
    sp.partial = h->batch.spk.d_partial.p;
    sp.spk_off = h->batch.spk.d_off.p;
    sp.spk_list = h->batch.spk.d_list.p;
    sp.n_spk = h->batch.spk.n_spk;
    sp.prior_count = h->batch.spk.d_prior_n.p;
    sp.prior_acc = h->batch.spk.d_prior.p;
    sp.count = h->batch.spk.d_count.p;
    sp.acc = h->batch.spk.d_acc.p;
    sp.stats = h->batch.spk.d_stats.p;
    sp.tiles = h->batch.spk.d_tiles.p;
    sp.n_tiles = h->batch.spk.n_tiles;
    if (sp.mode == MFX_SPK_POOL) HIP_TRY(h, launch_spk_sums(sp, stream));
    HIP_TRY(h, launch_spk_finish(sp, stream));
    HIP_TRY(h, launch_spk_apply(sp, stream));
    h->batch.spk.ran = true;
    return MFX_OK;
}

// the normaliser of a run while the online attachment is in force: in run_norm's place, on its stream, from the raw rows of
// the scratch (d_pre) into the run's rows (d_out), over the chunks of the utterance range
int run_online_norm(mfx_handle *h, hipStream_t stream, const float *d_pre, float *d_out, int u0, int u1)
{
    const BatchState &B = h->batch;
    OnormParams op{};
    op.src = d_pre;
    op.src_pitch = h->width;
    op.out = d_out;
    op.out_pitch = h->width;
    op.Wn = spk_wn(h);
    op.window = B.on.window;
    op.cvn = h->cfg.norm == MFX_NORM_CVN ? 1 : 0;
    op.prior_frames = B.on.prior_frames;
    op.prior_count = B.on.prior_count;
    op.prior_acc = B.on.d_prior.p;
    op.segs = B.d_segs.p;
    op.chunks = B.on.chunks.range(u0, u1);
    op.tot = B.on.d_tot.p;
    op.u0 = u0, op.n_utt = u1 - u0;
    HIP_TRY(h, launch_onorm(op, stream));
    return MFX_OK;
}

// the sliding-window normaliser of a run: behind the paste, on the tail's stream, from the raw rows y of its scratch (d_raw)
// into where the rows y go (d_y), all Wy columns, over the chunks of the utterance range
int run_sliding_norm(mfx_handle *h, hipStream_t stream, const float *d_raw, float *d_y, int u0, int u1)
{
    const BatchState &B = h->batch;
    SlideParams sp{};
    sp.pre.src = d_raw;
    sp.pre.src_pitch = B.sl.Wy;
    sp.pre.out = d_y;
    sp.pre.out_pitch = B.sl.Wy;
    sp.pre.Wn = B.sl.Wy;
    sp.pre.segs = B.d_segs.p;
    sp.pre.chunks = B.sl.chunks.range(u0, u1);
    sp.pre.tot = B.sl.d_tot.p;
    sp.pre.u0 = u0, sp.pre.n_utt = u1 - u0;
    sp.window = B.sl.window, sp.min_window = B.sl.min_window, sp.center = B.sl.center, sp.norm_vars = B.sl.norm_vars;
    HIP_TRY(h, launch_slide(sp, stream));
    return MFX_OK;
}

// ---- stage 1: the checks every layout of the PCM array goes through (the caller's, and the scratch of a rates plan)
int check_layout(mfx_handle *h, const int16_t *d_pcm, int64_t pcm_samples_total, const std::vector<int64_t> &off,
                 const std::vector<int64_t> &len, int u0, int u1)
{
    if (((uintptr_t)d_pcm & 3) != 0) return fail(h, MFX_ERR_ARG, "d_pcm must be 4-byte aligned");
    for (int u = u0; u < u1; ++u)
        if (off[u] + len[u] > pcm_samples_total) return fail(h, MFX_ERR_ARG, "utterance extends past the end of the PCM array");
    return MFX_OK;
}

// ---- stage 2, a rates plan in force: the caller's array is converted into the handle's scratch by one launch over the tiles
// of the utterance range, and everything behind it runs as it always does on the scratch and its layout
int convert_rates(mfx_handle *h, const int16_t *d_pcm, int u0, int u1)
{
    const BatchState::Rates &rs = h->batch.rs;
    HIP_TRY(h, hipSetDevice(h->device));
    const int32_t t0 = rs.utt_tile0[u0], t1 = rs.utt_tile0[u1];
    ResampleParams rp{};
    rp.pcm = d_pcm;
    rp.out = rs.d_pcm.p;
    rp.tiles = rs.d_tiles.p + t0;
    rp.n_tiles = t1 - t0;
    rp.rates = rs.d_rates.p;
    rp.taps = rs.d_taps.p;
    rp.channels = h->channels;
    rp.lds = rs.lds;
    HIP_TRY(h, launch_resample(rp, h->stream));
    return MFX_OK;
}

// ---- stage 3: how this run goes, decided up front
struct RunMode {
    FrontKind kind;         // the 512-point register kernel, else the fused wave-per-frame kernel when its LDS fits, else
                            // spectrum through an HBM slab + melcep (per-utterance warp factors in force: always the slab)
    float *d_out, *d_last, *d_final; // where the rows y are built, where the run's last stage before the VAD writes, where
                            // the finished rows go: all the same unless a transform (d_out is its scratch) or a
                            // selecting VAD (d_last is its scratch) is in force.  d_final is the caller's array, unless a
                            // tensor output is in force: then its row scratch, and k_tensor_pack writes the caller's tensor
    void *d_tensor;         // the caller's array while a tensor output is in force, else null
    float *d_y;             // where the transform reads the rows y
    float *d_raw;           // where the rows y are finished and the VAD's decision reads them: d_y, unless the sliding-window
                            // normaliser is in force (its raw-row scratch; k_slide_apply writes the normalised rows to d_y).
                            // It is d_out, unless pitch features are pasted (d_out is then the scratch of the `width`
                            // columns, and k_pitch_paste writes the wide rows to d_raw)
    float *d_pre;           // where everything AHEAD of the normaliser's place writes: d_out, unless the online normaliser is
                            // in force (its raw-row scratch: it must not run in place, its trailing edge reads raw rows that
                            // another block may already have turned into output)
    int sb;                 // which of the two statics buffers (overlap)
    bool via_scratch;       // With deltas on, the front end writes its statics as compact 64-byte rows into a scratch buffer
                            // and the delta kernel emits whole [static | d | dd] rows: every HBM write is then a full line
                            // (13-float row pieces at a 156-byte pitch cost 1.5x their size in 32-byte sectors).
    bool fuse;              // Fused delta stage: the 512-point kernel's last wave per block turns the statics into whole
                            // output rows while the other 15 produce them, and help it with the block's last tiles once their
                            // frames are over; no separate delta launch.
    bool split_tail;        // Overlap (opt-in, mfx_batch_overlap): the delta/normalisation tail runs on a second stream behind
                            // an event, so the memory-bound tail of batch i shares the GPU with the compute-bound front end of
                            // batch i+1; the statics scratch is double buffered and the front end of batch i+2 waits for tail i.
    hipStream_t tail_stream;
};

// (p: filled by fill_front; a run that may fuse gets the delta wave's parameters)
RunMode decide_mode(const mfx_handle *h, FrontParams &p, float *d_out, bool whole)
{
    const BatchState &B = h->batch;
    RunMode m{};
    m.kind = batch_front(h);
    // A transform in force: everything runs as it always does with the handle's scratch in the place of d_out, and
    // k_splice_affine turns the scratch rows into the caller's array as the last launch.
    // A selecting VAD in force: the last stage writes to the VAD's scratch, and k_vad_select moves the voiced rows from there
    // into the caller's array.
    // A tensor output in force: the last link.  The finished rows go to its scratch, and k_tensor_pack turns them into the
    // caller's tensor.
    m.d_tensor = B.tn.on ? d_out : nullptr;
    m.d_final = B.tn.on ? B.tn.d_rows.p : d_out;
    m.d_last = (B.vad.on && B.vad.mode != MFX_VAD_FLAGS) ? B.vad.d_rows.p : m.d_final;
    m.d_y = B.xf.on ? B.xf.d_y.p : m.d_last;
    m.d_raw = B.sl.on ? B.sl.d_raw.p : m.d_y;
    m.d_out = B.pf.on && B.pf.paste ? B.pf.d_narrow.p : m.d_raw;
    m.d_pre = B.on.on ? B.on.d_raw.p : m.d_out;
    const bool norm_before = h->cfg.norm != MFX_NORM_NONE && !h->cfg.norm_after_dyn;
    m.sb = (B.ov.enabled && whole) ? (int)(B.ov.seq & 1) : 0;
    m.via_scratch = compact_statics(m.kind, p) && h->l1 > 0 && h->cols <= 16 && !h->traps && !norm_before &&
                    B.d_static16[m.sb].n >= (size_t)B.total_rows * 16;
    m.fuse = whole && h->fuse.planned && m.kind == kFront512 && m.via_scratch && ((uintptr_t)m.d_pre & 15) == 0;
    // Not asked for (MFX_ENGINE_FUSE_DELTA): the plain run only -- the planner has looked at the batch's size; nothing
    // attached, no overlap in force (the fused form has no tail to put on the second stream)
    if (m.fuse && !h->fuse.enabled)
        m.fuse = !B.ov.enabled && !B.rs.on && !B.va.on && !B.xf.on && !B.spk.on && !B.vad.on && !B.on.on && !B.sl.on && !B.pt.on && !B.pf.on && !B.tn.on;
    if (m.fuse) {
        p.dl1 = h->l1;
        p.dl2 = h->l2;
        p.done_words = h->fuse.done_words;
        p.dshare = delta_share_fits(h->l1, h->l2) ? h->fuse.share : 0; // (orders whose sub-tile does not fit: the delta wave alone)
        m.fuse = p.dct_mode == 1 && front512_delta_lds_bytes(p) <= kLdsCap;
    }
    m.split_tail = whole && B.ov.enabled && m.via_scratch && !m.fuse;
    m.tail_stream = m.split_tail ? B.ov.stream2 : h->stream;
    return m;
}

// ---- stage 4, on the handle's stream: the front end over chunks [c0, c1) of the plan, then k_traps
int run_front(mfx_handle *h, FrontParams &p, const RunMode &m, int u0, int u1, int32_t c0, int32_t c1)
{
    BatchState &B = h->batch;
    if (h->stft) { // k_stft_mel (k_stft_fft_mel) over the range's blocks, then (WHISPER) the clamp by the utterance's maximum, in place
        StftParams sp{};
        sp.pcm = p.pcm;
        sp.chunks = B.d_stft_chunks.p + c0;
        sp.n_chunks = c1 - c0;
        sp.chunk_first = c0;
        sp.tile_rows = h->stft_R;
        sp.core = stft_core(h, p.feat, p.feat_pitch);
        sp.blk_max = B.d_stft_max.p;
        {
            ProfScope ps(h);
            HIP_TRY(h, launch_stft(sp, h->stream));
        }
        if (sp.core.post == MFX_LOGMEL_WHISPER) HIP_TRY(h, launch_stft_post(sp, h->stream));
        return MFX_OK;
    }
    if (m.split_tail && B.ov.tail_pending[m.sb]) // tail of batch i-2 still reads this scratch buffer
        HIP_TRY(h, hipStreamWaitEvent(h->stream, B.ov.ev_tail[m.sb], 0));
    if (m.fuse) {
        p.chunks = h->fuse.d_chunks.p;
        p.n_chunks = h->fuse.nchunks;
        p.blk_chunk_off = h->fuse.d_blk_chunk_off.p;
        p.blk_tile_off = h->fuse.d_blk_tile_off.p;
        p.tiles = h->fuse.d_tiles.p;
        p.out = m.d_pre; // (fusing means no normaliser before the deltas: the delta wave is ahead of the normaliser's place)
        p.out_pitch = h->width;
        p.n_blocks = h->fuse.blocks;
        p.err_flag = h->fuse.d_err.p;
        p.spec = h->d_spec.p; // unused by this kernel; a -DMFX_DSTAMPS dev build drops the delta wave's tick counts here
        ProfScope ps(h);
        HIP_TRY(h, launch_front512_delta(p, B.aligned, h->nm16, h->stream));
        ++h->fuse.runs;
    } else {
        FrontWork w;
        w.h_chunks = B.h_chunks.data() + c0, w.d_chunks = B.d_chunks.p + c0, w.n_chunks = (size_t)(c1 - c0);
        w.profile = true;
        if (is_spec_kind(m.kind)) { // magnitudes go through an HBM slab, then melcep
            w.slab_rows = std::min<int64_t>(B.total_rows, kSlabRowsMax);
            if (B.d_spec_slab.n < (size_t)w.slab_rows * h->spec_pitch) HIP_TRY(h, B.d_spec_slab.alloc((size_t)w.slab_rows * h->spec_pitch));
            w.slab = B.d_spec_slab.p;
            if (B.va.on) { // every table on its own rows of the slab, one launch per window
                w.tables = &B.va.tables;
                w.runs = B.va.d_runs.p, w.run_off = B.va.d_run_off.p;
                w.h_runs = B.va.h_runs.data(), w.h_run_off = B.va.h_run_off.data();
            }
        }
        // (launch_front bounds a window of the slab by the row span of its chunks, and the plain cepstra step wants a
        // window's rows contiguous.  Both hold here: the rows of the plan's chunks ascend without a gap inside any utterance
        // range, utterances without frames own no chunk, and the tail split cuts chunks in place, keeping that order --
        // the span of a window is the sum of its chunks' frames.)
        const int rc = launch_front(h, p, m.kind, B.aligned, w);
        if (rc != MFX_OK) return rc;
    }
    if (h->traps) { // part of the front end: on the handle's stream, before anything of the tail
        TrapsParams tp;
        fill_traps(h, tp);
        tp.src = B.d_logmel.p;
        tp.src_pitch = B.mel_pitch;
        tp.out = m.d_pre;
        tp.out_pitch = h->width;
        tp.segs = B.d_segs.p + u0;
        tp.n_segs = u1 - u0;
        tp.tiles_per_seg_max = B.tiles_max;
        HIP_TRY(h, launch_traps(tp, h->stream));
    }
    return MFX_OK;
}

// the pitch track of a run: k_pitch_nccf and k_pitch_track over the utterance range, on the handle's stream behind the front
// end (never the tail's: once the handle's stream has passed them the PCM may be reused); `pcm` is what the front end read.
// Pitch features in force: k_pitch_feats directly behind them, so that run_tail's ev_front orders the tail's stream behind it.
int run_pitch(mfx_handle *h, const RunMode &m, const int16_t *pcm, int u0, int u1)
{
    BatchState &B = h->batch;
    BatchState::Pitch &pt = B.pt;
    PitchParams pp{};
    pp.pcm = pcm;
    pp.channels = h->channels;
    pp.utt = pt.d_utt.p;
    pp.segs = B.d_segs.p;
    pp.tiles = pt.tiles.range(u0, u1);
    pp.u0 = u0, pp.u1 = u1;
    pp.window = pt.window, pp.shift = h->S, pp.lag_min = pt.lag_min, pp.lag_max = pt.lag_max, pp.K = pt.K, pp.J = pt.J;
    pp.span_pad = pitch_span_pad(h->S);
    pp.groups = pitch_groups(pt.lag_min, pt.lag_max);
    pp.ballast = pt.ballast, pp.penalty = pt.penalty;
    pp.c1 = (float)(1.0 / (32768.0 * (double)(pt.window + pt.lag_max)));
    pp.wt = pt.d_wt.p, pp.lg = pt.d_lg.p;
    pp.nccf = pt.d_nccf.p, pp.bp = pt.d_bp.p, pp.pitch = pt.d_pitch.p, pp.index = pt.d_index.p;
    HIP_TRY(h, launch_pitch(pp, h->stream));
    pt.ran = true;
    BatchState::PitchFeats &pf = B.pf;
    if (!pf.on) return MFX_OK;
    // (overlap: the paste of the batch before this one reads d_feats on the tail's stream)
    if (pf.paste && m.split_tail && B.ov.tail_pending[m.sb ^ 1]) HIP_TRY(h, hipStreamWaitEvent(h->stream, B.ov.ev_tail[m.sb ^ 1], 0));
    PitchFeatParams fp{};
    fp.pitch = pt.d_pitch.p;
    fp.segs = B.d_segs.p;
    fp.tiles = pf.tiles.range(u0, u1);
    fp.columns = pf.columns, fp.F = pf.F;
    fp.left = pf.left, fp.right = pf.right, fp.D = pf.D;
    fp.sample_rate = h->cfg.sample_rate;
    fp.pov_scale = pf.pov_scale, fp.pov_offset = pf.pov_offset, fp.pitch_scale = pf.pitch_scale, fp.delta_scale = pf.delta_scale;
    fp.delta_den = pf.den;
    fp.feats = pf.d_feats.p;
    HIP_TRY(h, launch_pitch_feats(fp, h->stream));
    pf.ran = true;
    return MFX_OK;
}

// the normaliser of a run over `groups` column groups of m.d_out: the online attachment's kernels while it is in force (raw
// rows from m.d_pre), the speaker list's while one is (the run then covers the whole batch, mfx_batch_run_host does not
// slice), else every utterance's own statistics
int run_batch_norm(mfx_handle *h, const RunMode &m, int u0, int u1, int groups, size_t group_stats_stride)
{
    const BatchState &B = h->batch;
    if (B.on.on) return run_online_norm(h, m.tail_stream, m.d_pre, m.d_out, u0, u1);
    if (B.spk.on) return run_speaker_norm(h, m.tail_stream, m.d_out);
    return run_norm(h, m.tail_stream, m.d_out, h->width, B.d_segs.p + u0, u1 - u0, nullptr, B.d_stats.p + (size_t)u0 * 2 * h->cols, false,
                    B.tiles_max * 64, groups, group_stats_stride);
}

// the VAD of a run: decision on the rows y (m.d_raw: before a transform, and before the sliding-window normaliser), selection
// from m.d_last into the caller's array
int run_vad(mfx_handle *h, const RunMode &m, int u0, int u1)
{
    BatchState &B = h->batch;
    BatchState::Vad &v = B.vad;
    VadParams vp{};
    vp.y = m.d_raw;
    vp.y_pitch = batch_y_width(h);
    vp.column = v.column;
    vp.segs = B.d_segs.p;
    vp.n_utt = B.n_utt;
    vp.u0 = u0, vp.u1 = u1;
    vp.tiles = v.tiles.range(u0, u1), vp.chunks = v.chunks.range(u0, u1);
    vp.energy_threshold = v.et, vp.energy_mean_scale = v.ms, vp.proportion_threshold = v.prop;
    vp.frames_context = v.ctx;
    vp.mode = v.mode;
    vp.partial = v.d_partial.p;
    vp.thr = v.d_thr.p;
    vp.voiced = v.d_voiced.p;
    vp.flags = v.d_flags.p;
    vp.mask = v.d_mask.p;
    vp.tile_base = v.d_tile_base.p;
    vp.packed_row0 = v.d_packed.p;
    vp.rows = v.mode != MFX_VAD_FLAGS ? m.d_last : nullptr;
    vp.out = v.mode != MFX_VAD_FLAGS ? m.d_final : nullptr;
    vp.width = batch_out_width(h);
    HIP_TRY(h, launch_vad(vp, m.tail_stream));
    v.last_stream = m.tail_stream;
    v.ran = true;
    if (m.d_tensor) // behind the selection, on its stream: the lengths are this run's counts under MFX_VAD_SELECT
        return run_tensor(h, m.tail_stream, m.d_final, m.d_tensor, u0, u1, v.mode == MFX_VAD_SELECT);
    return MFX_OK;
}

// ---- stage 5, on m.tail_stream: normaliser before the deltas, deltas, normaliser after them, paste, sliding-window
// normaliser, transform, VAD
int run_tail(mfx_handle *h, const RunMode &m, int u0, int u1)
{
    BatchState &B = h->batch;
    if (m.split_tail) {
        HIP_TRY(h, hipEventRecord(B.ov.ev_front[m.sb], h->stream));
        HIP_TRY(h, hipStreamWaitEvent(B.ov.stream2, B.ov.ev_front[m.sb], 0));
    }
    const bool norm = h->cfg.norm != MFX_NORM_NONE;
    if (norm && !h->cfg.norm_after_dyn) {
        const int rc = run_batch_norm(h, m, u0, u1, 1, 0);
        if (rc != MFX_OK) return rc;
    }
    if (h->l1 > 0 && !m.fuse) {
        DeltaParams dp;
        fill_delta(h, dp);
        // (the online normaliser in force: behind it the deltas work on d_out as always, ahead of it on its scratch)
        float *rows = B.on.on && h->cfg.norm_after_dyn ? m.d_pre : m.d_out;
        dp.src = m.via_scratch ? B.d_static16[m.sb].p : rows;
        dp.src_pitch = m.via_scratch ? 16 : h->width;
        dp.out = rows;
        dp.segs = B.d_segs.p + u0;
        dp.n_segs = u1 - u0;
        dp.tiles_per_seg_max = B.tiles_max;
        HIP_TRY(h, launch_delta(dp, m.tail_stream));
    }
    if (norm && h->cfg.norm_after_dyn) {
        const int rc = run_batch_norm(h, m, u0, u1, h->width / h->cols, (size_t)B.n_utt * 2 * h->cols);
        if (rc != MFX_OK) return rc;
    }
    if (B.pf.on && B.pf.paste) { // the rows y become [ y | feats ]: the last launch ahead of the transform
        PitchPasteParams pq{};
        pq.narrow = m.d_out, pq.feats = B.pf.d_feats.p;
        pq.out = m.d_raw;
        pq.row0 = B.utt_row[u0], pq.rows = (u1 < B.n_utt ? B.utt_row[u1] : B.total_rows) - B.utt_row[u0];
        pq.Wd = h->width, pq.F = B.pf.F;
        HIP_TRY(h, launch_pitch_paste(pq, m.tail_stream));
    }
    if (B.sl.on) { // the rows y, pasted columns included, become their normalised twins: the last link ahead of the transform
        const int rc = run_sliding_norm(h, m.tail_stream, m.d_raw, m.d_y, u0, u1);
        if (rc != MFX_OK) return rc;
    }
    if (B.xf.on) { // behind the tail, on its stream: ev_tail covers it
        XformParams xp;
        fill_xform(h, xp);
        xp.src = m.d_y;
        xp.out = m.d_last;
        xp.segs = B.d_segs.p + u0;
        xp.n_segs = u1 - u0;
        xp.seg_xf = B.xf.d_idx.p ? B.xf.d_idx.p + u0 : nullptr;
        xp.operands = B.xf.d_ops.p;
        xp.bias = B.xf.d_bias.p;
        xp.tiles_per_seg_max = B.tiles_max;
        HIP_TRY(h, launch_xform(xp, m.tail_stream));
    }
    if (B.vad.on) { // last of all (but for the tensor launch at its end), on the tail's stream: ev_tail covers it
        const int rc = run_vad(h, m, u0, u1);
        if (rc != MFX_OK) return rc;
    } else if (m.d_tensor) { // the finished rows become the caller's tensor: the last launch, on the tail's stream
        const int rc = run_tensor(h, m.tail_stream, m.d_final, m.d_tensor, u0, u1, false);
        if (rc != MFX_OK) return rc;
    }
    if (m.split_tail) {
        HIP_TRY(h, hipEventRecord(B.ov.ev_tail[m.sb], m.tail_stream));
        B.ov.tail_pending[m.sb] = true;
    }
    return MFX_OK;
}

// utterances [u0, u1) of the planned batch (all of them: the fused-delta and overlap modes apply); DESIGN.md section 5,
// "Batch entries", describes the five stages
int batch_run_range(mfx_handle *h, const int16_t *d_pcm, int64_t pcm_samples_total, float *d_out, int u0, int u1)
{
    BatchState &B = h->batch;
    if (!d_pcm || !d_out || pcm_samples_total <= 0) return fail(h, MFX_ERR_ARG, "invalid argument");
    const bool whole = u0 == 0 && u1 == B.n_utt;
    if (B.spk.on && !whole) return fail(h, MFX_ERR_STATE, "a speaker list is in force: the batch runs as a whole");
    if (B.vad.on && B.vad.mode == MFX_VAD_PACK && !whole) return fail(h, MFX_ERR_STATE, "a packing VAD is in force: the batch runs as a whole");
    if (!h->have_window) return fail(h, MFX_ERR_STATE, "set_window has not been called");
    int rc;
    if (B.rs.on) {
        if ((rc = check_layout(h, d_pcm, pcm_samples_total, B.rs.in_off, B.rs.in_len, u0, u1)) != MFX_OK) return rc;
        if ((rc = convert_rates(h, d_pcm, u0, u1)) != MFX_OK) return rc;
        d_pcm = B.rs.d_pcm.p;
        pcm_samples_total = B.rs.total;
    }
    if (B.total_rows == 0) {
        B.vad.ran = B.vad.on; // (nothing to decide: the read-back returns what the setter left, no voiced row)
        B.pt.ran = B.pt.on;   // (no row to track: the read-back copies nothing)
        B.pf.ran = B.pf.on;
        if (!B.tn.on) return MFX_OK;
        HIP_TRY(h, hipSetDevice(h->device)); // (a tensor of pad values: every element is written on every run)
        return run_tensor(h, h->stream, B.tn.d_rows.p, d_out, u0, u1, B.vad.on && B.vad.mode == MFX_VAD_SELECT);
    }
    if ((rc = check_layout(h, d_pcm, pcm_samples_total, B.utt_off, B.utt_len, u0, u1)) != MFX_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = refresh_mel(h)) != MFX_OK) return rc;
    const int32_t c0 = B.utt_chunk0[u0], c1 = B.utt_chunk0[u1]; // chunk range of the utterance range
    if (c1 <= c0) { // a range without a frame: nothing to compute, but the VAD's counts and prefix are still to be written
        B.pt.ran = B.pt.ran || B.pt.on; // (the pitch track has no row to write either)
        B.pf.ran = B.pf.ran || B.pf.on;
        RunMode none{};
        none.d_tensor = B.tn.on ? d_out : nullptr;
        none.d_last = B.vad.d_rows.p, none.d_final = B.tn.on ? B.tn.d_rows.p : d_out;
        none.tail_stream = h->stream;
        if (B.vad.on) return run_vad(h, none, u0, u1);
        return B.tn.on ? run_tensor(h, h->stream, none.d_final, d_out, u0, u1, false) : MFX_OK; // (pad values: every element is written)
    }
    const size_t rows = (size_t)B.total_rows; // (every scratch a launch below writes to holds the plan's rows)
    if ((h->traps && B.d_logmel.n < rows * B.mel_pitch) || !B.xf.sized(rows, batch_y_width(h)) || !B.vad.sized(rows, batch_out_width(h)) ||
        !B.on.sized(rows, h->width) || !B.sl.sized(rows, batch_y_width(h)) || !B.pt.sized(rows) || !B.pf.sized(rows, h->width, B.pt.on) || !B.tn.sized(rows, batch_out_width(h)))
        return fail(h, MFX_ERR_STATE, "batch not planned");

    FrontParams p;
    fill_front(h, p);
    p.pcm = d_pcm;
    p.pcm_total = pcm_samples_total * h->channels;
    p.row_limit = B.total_rows;
    const RunMode m = decide_mode(h, p, d_out, whole);
    if (m.via_scratch) {
        p.feat = B.d_static16[m.sb].p;
        p.feat_pitch = 16;
    } else { // (TRAPS: the front end's log mel rows go to the scratch; k_traps turns them into the statics of d_out)
        p.feat = h->traps ? B.d_logmel.p : m.d_pre;
        p.feat_pitch = h->traps ? B.mel_pitch : h->width;
    }
    if ((rc = run_front(h, p, m, u0, u1, c0, c1)) != MFX_OK) return rc;
    if (B.pt.on && (rc = run_pitch(h, m, d_pcm, u0, u1)) != MFX_OK) return rc;
    if ((rc = run_tail(h, m, u0, u1)) != MFX_OK) return rc;
    if (whole) ++B.ov.seq;
    return MFX_OK;
}
} // namespace

extern "C" int mfx_batch_run_device(mfx_handle *h, const int16_t *d_pcm, int64_t pcm_samples_total, float *d_out)
{
    MFX_DEVICE_ENTRY(h);
    return batch_run_range(h, d_pcm, pcm_samples_total, d_out, 0, h->batch.n_utt);
}


extern "C" void *mfx_alloc_pinned(size_t bytes)
{
    void *p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

extern "C" void mfx_free_pinned(void *p)
{
    if (p) (void)hipHostFree(p);
}

extern "C" int mfx_batch_overlap(mfx_handle *h, int enable)
{
    MFX_DEVICE_ENTRY(h);
    if (const int rc = sync_device(h); rc != MFX_OK) return rc;
    if (enable && !h->batch.ov.stream2) {
        HIP_TRY(h, hipStreamCreateWithFlags(&h->batch.ov.stream2, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            HIP_TRY(h, hipEventCreateWithFlags(&h->batch.ov.ev_front[i], hipEventDisableTiming));
            HIP_TRY(h, hipEventCreateWithFlags(&h->batch.ov.ev_tail[i], hipEventDisableTiming));
        }
    }
    h->batch.ov.enabled = enable != 0;
    h->batch.ov.tail_pending[0] = h->batch.ov.tail_pending[1] = false;
    return size_static16(h);
}

extern "C" int mfx_batch_run_host(mfx_handle *h, const int16_t *pcm, int64_t pcm_samples_total, float *out)
{
    MFX_DEVICE_ENTRY(h);
    if (!pcm || !out || pcm_samples_total <= 0) return fail(h, MFX_ERR_ARG, "invalid argument");
    HIP_TRY(h, hipSetDevice(h->device));
    // device-side staging of the host buffers, kept by the handle and grown on demand
    const size_t n_in = (size_t)pcm_samples_total * h->channels;
    const int64_t ow = batch_out_width(h); // floats of an output row
    // (a tensor output in force: `out` is the tensor, mfx_batch_output_bytes of it; staged in whole floats)
    const BatchState::Tensor &tn = h->batch.tn;
    const int64_t out_bytes = batch_output_bytes(h);
    const size_t n_out = tn.on ? (size_t)(out_bytes + 3) / 4 + 1 : (size_t)std::max<int64_t>(h->batch.total_rows, 1) * ow;
    if (h->batch.host.d_pcm.n < n_in + 8) HIP_TRY(h, h->batch.host.d_pcm.alloc(n_in + 8));
    if (h->batch.host.d_out.n < n_out) HIP_TRY(h, h->batch.host.d_out.alloc(n_out));

    // Pinned caller buffers and a batch worth slicing: the utterances go through in up to 8 slices, the upload of slice
    // k + 1 and the download of slice k - 1 running beside the kernels of slice k on their own streams (PCIe is full
    // duplex: the 320 MB in and the 156 MB out of a C2 batch overlap instead of queueing up).  Utterance offsets must
    // ascend for a slice to be one contiguous piece of the PCM array; anything else takes the plain path below.
    // (a rates plan in force: the caller's array is cut by its own layout, in input-rate samples)
    const std::vector<int64_t> &in_off = h->batch.rs.on ? h->batch.rs.in_off : h->batch.utt_off;
    const std::vector<int64_t> &in_len = h->batch.rs.on ? h->batch.rs.in_len : h->batch.utt_len;
    bool ascending = true;
    for (int u = 1; u < h->batch.n_utt && ascending; ++u) ascending = in_off[u] >= in_off[u - 1] + in_len[u - 1];
    const int K = (int)std::min<int64_t>(8, h->batch.n_utt / 4);
    // (a speaker list in force: a speaker may span slices, the batch goes through whole)
    // (the fused delta stage asked for: it runs on whole batches only; not asked for, it yields to the slices)
    // (a packing VAD in force: an utterance's destination depends on the slices in front of it, the batch goes through whole)
    const bool packing = h->batch.vad.on && h->batch.vad.mode == MFX_VAD_PACK;
    if (K >= 2 && ascending && !h->batch.ov.enabled && !(h->fuse.planned && h->fuse.enabled) && !h->batch.spk.on && !packing && n_in * sizeof(int16_t) >= ((size_t)32 << 20) &&
        is_pinned_host(pcm) && is_pinned_host(out)) {
        if (!h->batch.host.stream_up) {
            HIP_TRY(h, hipStreamCreateWithFlags(&h->batch.host.stream_up, hipStreamNonBlocking));
            HIP_TRY(h, hipStreamCreateWithFlags(&h->batch.host.stream_dn, hipStreamNonBlocking));
            for (int i = 0; i < 16; ++i) {
                HIP_TRY(h, hipEventCreateWithFlags(&h->batch.host.ev_up[i], hipEventDisableTiming));
                HIP_TRY(h, hipEventCreateWithFlags(&h->batch.host.ev_run[i], hipEventDisableTiming));
            }
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        // every utterance inside the caller's array BEFORE the first copy is queued (batch_run_range only looks at the
        // slice it is given, and only after that slice's upload is in flight)
        for (int u = 0; u < h->batch.n_utt; ++u)
            if (in_off[u] < 0 || in_off[u] + in_len[u] > pcm_samples_total)
                return fail(h, MFX_ERR_ARG, "utterance outside the PCM array");
        const int ch = h->channels;
        // one slice; an error leaves copies in flight on three streams, which slices_done drains before returning
        auto run_slice = [&](int k) -> int {
            const int u0 = (int)((int64_t)h->batch.n_utt * k / K), u1 = (int)((int64_t)h->batch.n_utt * (k + 1) / K);
            // samples [s0, s1) of the array hold the slice (s0 rounded down to an even sample: 4-byte aligned pieces)
            const int64_t s0 = (k == 0 ? 0 : in_off[u0]) & ~(int64_t)1;
            const int64_t s1 = std::min<int64_t>(k + 1 == K ? pcm_samples_total : in_off[u1], pcm_samples_total);
            if (s1 > s0)
                HIP_TRY(h, hipMemcpyAsync(h->batch.host.d_pcm.p + s0 * ch, pcm + s0 * ch, (size_t)(s1 - s0) * ch * sizeof(int16_t),
                                          hipMemcpyHostToDevice, h->batch.host.stream_up));
            HIP_TRY(h, hipEventRecord(h->batch.host.ev_up[k], h->batch.host.stream_up));
            HIP_TRY(h, hipStreamWaitEvent(h->stream, h->batch.host.ev_up[k], 0));
            int rc = batch_run_range(h, h->batch.host.d_pcm.p, pcm_samples_total, h->batch.host.d_out.p, u0, u1);
            if (rc != MFX_OK) return rc;
            HIP_TRY(h, hipEventRecord(h->batch.host.ev_run[k], h->stream));
            HIP_TRY(h, hipStreamWaitEvent(h->batch.host.stream_dn, h->batch.host.ev_run[k], 0));
            if (tn.on) { // an utterance's block of the tensor is contiguous in both layouts: the slice's blocks are one piece
                const int64_t per = (int64_t)tn.Tp * tn.Wo * tensor_elem_bytes(tn.dtype);
                if (per > 0)
                    HIP_TRY(h, hipMemcpyAsync((char *)out + u0 * per, (const char *)h->batch.host.d_out.p + u0 * per, (size_t)((u1 - u0) * per),
                                              hipMemcpyDeviceToHost, h->batch.host.stream_dn));
                return MFX_OK;
            }
            const int64_t r0 = h->batch.utt_row[u0], r1 = u1 < h->batch.n_utt ? h->batch.utt_row[u1] : h->batch.total_rows;
            if (r1 > r0)
                HIP_TRY(h, hipMemcpyAsync(out + r0 * ow, h->batch.host.d_out.p + r0 * ow, (size_t)(r1 - r0) * ow * sizeof(float),
                                          hipMemcpyDeviceToHost, h->batch.host.stream_dn));
            return MFX_OK;
        };
        for (int k = 0; k < K; ++k) {
            const int rc = run_slice(k);
            if (rc != MFX_OK) { // nothing may still read `pcm` or write `out` once we have returned
                (void)hipStreamSynchronize(h->batch.host.stream_up);
                (void)hipStreamSynchronize(h->stream);
                (void)hipStreamSynchronize(h->batch.host.stream_dn);
                return rc;
            }
        }
        HIP_TRY(h, hipStreamSynchronize(h->batch.host.stream_dn));
        return mfx_synchronize(h);
    }

    HIP_TRY(h, hipMemcpyAsync(h->batch.host.d_pcm.p, pcm, n_in * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
    int rc = mfx_batch_run_device(h, h->batch.host.d_pcm.p, pcm_samples_total, h->batch.host.d_out.p);
    if (rc != MFX_OK) {
        (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    if (h->batch.ov.stream2) HIP_TRY(h, hipStreamSynchronize(h->batch.ov.stream2)); // overlapped tail, if any
    if (out_bytes > 0) // (total_rows * ow floats, or the tensor)
        HIP_TRY(h, hipMemcpyAsync(out, h->batch.host.d_out.p, (size_t)out_bytes, hipMemcpyDeviceToHost, h->stream));
    return mfx_synchronize(h);
}
