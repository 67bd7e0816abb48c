// mfx_stream.cpp -- the streaming interface of include/mfx.h: set_input / flush / apply / get_output_data.
//
// The bookkeeping restates the reference's segmenter and apply() state machines (segmentercpu.cpp:56-106 /
// segmenteropencl.cpp:120-175, mfcccpu.cpp:371-425 / mfccopencl.cpp:495-549) on top of device buffers; all arithmetic on
// samples and features happens in the HIP kernels.  This file owns the handle's `st` and `sweep` parts and names no field
// of `batch` or `fuse`.
#include "mfx_handle.h"

#include <cstring>
#include <thread>

using namespace mfx;

// page-locked host memory?  dev_ptr (optional): the address a kernel uses for it (the same address for hipHostMalloc memory;
// registered memory reports its own)
bool is_pinned_host(const void *p, void **dev_ptr)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError(); // plain pageable memory: not an error
        return false;
    }
    if (a.type != hipMemoryTypeHost) return false;
    if (dev_ptr) *dev_ptr = a.devicePointer ? a.devicePointer : const_cast<void *>(p);
    return true;
}

namespace {

// ---- host side of the streaming copies --------------------------------------------------------------------------
// The drop-in interface hands over pageable host memory that the caller may overwrite on return (ASR_OCL.cpp:160-161,
// 231,243), so a block goes through pinned staging.  The staging copy is split over a few threads when it is large
// (one core moves ~10 GB/s, the link 50) and pipelined with the DMA in chunks; a caller buffer that is itself pinned
// (hipHostMalloc / hipHostRegister, a pinned torch tensor) is used by the DMA directly.
void host_copy(void *dst, const void *src, size_t bytes)
{
    const size_t kMin = (size_t)1 << 20;
    const unsigned nt = (unsigned)std::min<size_t>(4, bytes / kMin);
    if (nt <= 1) {
        std::memcpy(dst, src, bytes);
        return;
    }
    const size_t piece = ((bytes / nt) + 63) & ~(size_t)63;
    std::thread th[3];
    for (unsigned t = 1; t < nt; ++t) {
        const size_t off = piece * t, len = t + 1 == nt ? bytes - off : piece;
        th[t - 1] = std::thread([=] { std::memcpy((char *)dst + off, (const char *)src + off, len); });
    }
    std::memcpy(dst, src, piece);
    for (unsigned t = 1; t < nt; ++t) th[t - 1].join();
}

constexpr size_t kCopyChunk = (size_t)4 << 20;

bool small_block(const mfx_handle *h, size_t bytes)
{
    return bytes > 0 && bytes < kSmallBlock && !(h->cfg.engine & MFX_ENGINE_DMA_SMALL_BLOCKS);
}

// host block -> device, asynchronous on the stream; `src` is free for the caller when this returns
int upload_block(mfx_handle *h, int16_t *d_dst, const int16_t *src, size_t samples, bool *direct)
{
    const size_t bytes = samples * sizeof(int16_t);
    *direct = bytes >= kCopyChunk && is_pinned_host(src);
    if (*direct) { // DMA straight from the caller's pinned buffer; the caller waits for it (wait_upload) before returning
        HIP_TRY(h, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, h->stream));
        if (!h->st.ev_copy[0]) HIP_TRY(h, hipEventCreateWithFlags(&h->st.ev_copy[0], hipEventDisableTiming));
        HIP_TRY(h, hipEventRecord(h->st.ev_copy[0], h->stream));
        return MFX_OK;
    }
    if (small_block(h, bytes)) {
        // a small block: into the pinned staging buffer at the destination's alignment, then a copy KERNEL reads it over the
        // link (one launch; a DMA command of this size costs more in latency than in transfer)
        char *stage = (char *)h->st.h_stage.p + ((uintptr_t)d_dst & 15);
        std::memcpy(stage, src, bytes);
        HIP_TRY(h, launch_copy_small(d_dst, stage, bytes, h->stream));
        return MFX_OK;
    }
    for (size_t off = 0; off < bytes; off += kCopyChunk) { // staging copy of chunk c+1 runs under the DMA of chunk c
        const size_t len = std::min(kCopyChunk, bytes - off);
        host_copy((char *)h->st.h_stage.p + off, (const char *)src + off, len);
        HIP_TRY(h, hipMemcpyAsync((char *)d_dst + off, (char *)h->st.h_stage.p + off, len, hipMemcpyHostToDevice, h->stream));
    }
    return MFX_OK;
}

// device rows -> host, returns when `dst` holds them; `stage`: the pinned staging buffer of the caller (h_out_stage for the
// plain rows, h_alpha_stage for a sweep's), grown here when it is too small
int download_rows(mfx_handle *h, float *dst, const float *d_src, size_t count, PinnedBuf<float> &stage)
{
    const size_t bytes = count * sizeof(float);
    if (small_block(h, bytes)) {
        // small: a copy kernel writes the rows into page-locked memory (the caller's buffer if it is pinned, else the
        // staging buffer at the source's alignment), one stream wait, one memcpy
        void *dst_dev = nullptr;
        if (is_pinned_host(dst, &dst_dev)) {
            HIP_TRY(h, launch_copy_small(dst_dev, d_src, bytes, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            return MFX_OK;
        }
        HIP_TRY(h, stage.grow(count + 4, std::max(count, (size_t)h->cap_rows * h->width) + 4, h->stream));
        char *at = (char *)stage.p + ((uintptr_t)d_src & 15);
        HIP_TRY(h, launch_copy_small(at, d_src, bytes, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        std::memcpy(dst, at, bytes);
        return MFX_OK;
    }
    if (bytes < kCopyChunk || is_pinned_host(dst)) {
        HIP_TRY(h, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return MFX_OK;
    }
    HIP_TRY(h, stage.grow(count, std::max(count, (size_t)h->cap_rows * h->width), h->stream));
    // chunks of the DMA into pinned staging, each followed by an event; the copy out of staging of chunk c runs under
    // the DMA of chunk c+1
    const size_t chunk = std::max(kCopyChunk, (bytes / 16 + 4095) & ~(size_t)4095);
    int n = 0;
    for (size_t off = 0; off < bytes; off += chunk, ++n) {
        const size_t len = std::min(chunk, bytes - off);
        HIP_TRY(h, hipMemcpyAsync((char *)stage.p + off, (const char *)d_src + off, len, hipMemcpyDeviceToHost, h->stream));
        if (!h->st.ev_copy[n]) HIP_TRY(h, hipEventCreateWithFlags(&h->st.ev_copy[n], hipEventDisableTiming));
        HIP_TRY(h, hipEventRecord(h->st.ev_copy[n], h->stream));
    }
    n = 0;
    for (size_t off = 0; off < bytes; off += chunk, ++n) {
        const size_t len = std::min(chunk, bytes - off);
        HIP_TRY(h, hipEventSynchronize(h->st.ev_copy[n]));
        host_copy((char *)dst + off, (const char *)stage.p + off, len);
    }
    return MFX_OK;
}

// frame + window + FFT + magnitude over the first `wcnd` frames of the carry buffer
int stream_front(mfx_handle *h, int wcnd)
{
    FrontParams p;
    fill_front(h, p);
    p.pcm = h->st.d_carry[h->st.cur].p;
    p.pcm_total = (int64_t)h->st.d_carry[h->st.cur].n;
    p.chunks = h->st.d_chunks.p;
    p.n_chunks = (wcnd + h->st.chunk_frames - 1) / h->st.chunk_frames;
    p.row_limit = wcnd;
    p.channels = 1;
    p.pair_ok = ((h->S % 2) == 0 && (h->W % 2) == 0) ? 1 : 0; // carry-buffer frames start at multiples of S
    p.spec = h->d_spec.p;
    p.spec_pitch = h->spec_pitch;
    if (h->fast512)
        HIP_TRY(h, launch_front512(p, /*to_spectrum=*/true, /*aligned=*/(h->S % 2) == 0, h->nm16, h->stream));
    else
        HIP_TRY(h, launch_front_generic(p, /*fused=*/false, h->stream));
    h->st.block_wcnd = wcnd;
    return MFX_OK;
}

// move the unconsumed tail to the front of the other carry buffer (the reference copies inside
// one buffer with overlapping ranges: segmentercpu.cpp:73,92 / segmenteropencl.cpp:139,160)
int carry_tail(mfx_handle *h, int total_samples)
{
    const int other = h->st.cur ^ 1;
    if (h->st.remaining > 0) {
        const size_t bytes = sizeof(int16_t) * (size_t)h->st.remaining;
        const int16_t *src = h->st.d_carry[h->st.cur].p + (total_samples - h->st.remaining);
        if (small_block(h, bytes))
            HIP_TRY(h, launch_copy_small(h->st.d_carry[other].p, src, bytes, h->stream));
        else
            HIP_TRY(h, hipMemcpyAsync(h->st.d_carry[other].p, src, bytes, hipMemcpyDeviceToDevice, h->stream));
    }
    h->st.cur = other;
    return MFX_OK;
}

// host_tail handles: the pending tail (`pending` samples at stage_tail_off) moves to the front of the staging buffer (the
// stream is idle: no kernel is reading it), the block (if any) goes behind it, and ONE copy kernel takes both to the front
// of the carry buffer
int stage_host_tail(mfx_handle *h, int pending, const int16_t *block, int samples)
{
    StreamState &st = h->st;
    if (pending > 0) {
        if (st.stage_tail_off > 0) std::memmove(st.h_stage.p, st.h_stage.p + st.stage_tail_off, (size_t)pending * sizeof(int16_t));
        st.stage_tail_off = 0;
    }
    if (block) std::memcpy(st.h_stage.p + pending, block, (size_t)samples * sizeof(int16_t));
    HIP_TRY(h, launch_copy_small(st.d_carry[st.cur].p, st.h_stage.p, ((size_t)pending + (size_t)samples) * sizeof(int16_t), h->stream));
    return MFX_OK;
}

} // namespace

extern "C" int mfx_set_input(mfx_handle *h, const int16_t *pcm, int32_t samples, int32_t *frames_out)
{
    MFX_DEVICE_ENTRY(h);
    MFX_STREAM_ENTRY(h);
    if (!pcm || !frames_out || samples < 0) return fail(h, MFX_ERR_ARG, "invalid argument");
    *frames_out = 0;
    if (!h->have_window) return fail(h, MFX_ERR_STATE, "set_window has not been called");
    if (samples > h->input_buffer_size) return fail(h, MFX_ERR_BUFFER_TOO_SMALL, kMsgBuffer);
    HIP_TRY(h, hipSetDevice(h->device));
    StreamState &st = h->st;
    st.last_block = false; // a new stream may follow a flush (reference never resets this: DESIGN.md B7)
    st.rows_in_stage = false;
    h->sweep.n = 0;
    st.block_frames = 0;

    const int D = h->D, W = h->W, S = h->S;
    // the caller may overwrite `pcm` as soon as we return: the block goes through pinned staging (upload_block), whose
    // previous contents the stream has long consumed (get_output_data / mfx_synchronize waited for it)
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    bool direct = false;
    // `pcm` must be free for the caller on EVERY return: when the block is DMA'd straight from the caller's pinned buffer
    // (upload_block sets `direct`), any exit -- the error returns below included -- first waits for that copy
    struct DirectWait {
        mfx_handle *h;
        const bool *direct;
        ~DirectWait()
        {
            if (*direct && h->st.ev_copy[0]) (void)hipEventSynchronize(h->st.ev_copy[0]);
        }
    } direct_wait{h, &direct};

    // first block of a stream (segmentercpu.cpp:59-75), or a continuation behind the `pending` carried samples (:76-93); the
    // capacity check is the continuation's alone (a first block was checked against input_buffer_size above)
    const bool first = st.last_calc_flushed = st.flushed;
    const int pending = first ? 0 : st.remaining;
    if (!first && (size_t)samples + (size_t)pending > st.carry_capacity) return fail(h, MFX_ERR_BUFFER_TOO_SMALL, kMsgBuffer);
    int rc = st.host_tail ? stage_host_tail(h, pending, pcm, samples)
                          : upload_block(h, st.d_carry[st.cur].p + pending, pcm, (size_t)samples, &direct);
    if (rc != MFX_OK) return rc;
    const int total = samples + pending;
    const int wcnd = estimated_window_count_f32(total, W, S);
    int window_count, processed;
    if (first) { // wcnd - D frames, and an error if that is none (segmentercpu.cpp:62-65,69)
        window_count = wcnd - D;
        if (window_count <= 0) return fail(h, MFX_ERR_WINDOW_COUNT, kMsgWindow);
        processed = (window_count - D) * S + W - S;
        // B13: a first block of fewer than 2 D frames.  The reference guards `processed <= 0` only (segmentercpu.cpp:70-71);
        // for D < frames < 2 D with W - S > (D - window_count) S it goes on and copies its carry-over from BEFORE the start
        // of its buffer (m_tmpbuffer + samples - m_remaining_samples is negative, :72-73) -- undefined there, refused here
        // with the message the reference's own guard carries.
        if (processed <= 0 || window_count < D) return fail(h, MFX_ERR_PROCESSED, kMsgProcessed);
    } else { // wcnd - 2 D frames, clamped to 0: no frames yet is no error (segmentercpu.cpp:81-90)
        window_count = std::max(wcnd - 2 * D, 0);
        processed = window_count * S + W - S;
    }
    if (window_count > 0) {
        rc = stream_front(h, wcnd);
        if (rc != MFX_OK) return rc;
    }
    st.remaining = total - processed + W - S;
    if (st.host_tail) {
        st.stage_tail_off = (size_t)(total - st.remaining);
    } else {
        rc = carry_tail(h, total);
        if (rc != MFX_OK) return rc;
    }
    st.flushed = false;
    st.samples = total;
    st.block_frames = window_count;
    *frames_out = window_count;
    if (direct) HIP_TRY(h, hipEventSynchronize(st.ev_copy[0])); // DMA from the caller's own (pinned) buffer: done before we return
    return MFX_OK;
}

extern "C" int mfx_flush(mfx_handle *h, int32_t *frames_out)
{
    MFX_DEVICE_ENTRY(h);
    MFX_STREAM_ENTRY(h);
    if (!frames_out) return fail(h, MFX_ERR_ARG, "invalid argument");
    *frames_out = 0;
    if (h->st.last_block) return MFX_OK; // nothing to flush (mfcccpu.cpp:350-351)
    HIP_TRY(h, hipSetDevice(h->device));
    h->st.last_block = true;
    h->st.flushed = true;
    h->st.rows_in_stage = false;
    h->sweep.n = 0;
    h->st.block_frames = 0;
    const int wcnd = estimated_window_count_f32(h->st.remaining, h->W, h->S);
    const int window_count = wcnd - h->D;
    if (window_count <= 0) return MFX_OK;
    if (h->st.host_tail && h->st.remaining > 0) { // the tail is on the host: up it goes, to the front of the carry buffer
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        int rc = stage_host_tail(h, h->st.remaining, nullptr, 0);
        if (rc != MFX_OK) return rc;
    }
    int rc = stream_front(h, wcnd);
    if (rc != MFX_OK) return rc;
    h->st.block_frames = window_count;
    *frames_out = window_count;
    return MFX_OK;
}

namespace {

// Size the buffers of a sweep of n alphas; (re)build its tables.
int prepare_sweep(mfx_handle *h, const float *alphas, int n)
{
    if (n > h->sweep.cap) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, h->sweep.d_src.alloc((size_t)n * h->cap_rows * h->cols));
        HIP_TRY(h, h->sweep.d_blk.alloc((size_t)n * h->cap_rows * h->width));
        HIP_TRY(h, h->sweep.d_stats.alloc((size_t)3 * n * 2 * h->cols));
        HIP_TRY(h, hipMemset(h->sweep.d_stats.p, 0, (size_t)3 * n * 2 * h->cols * sizeof(float)));
        HIP_TRY(h, h->sweep.d_segs.alloc((size_t)2 * n));
        h->sweep.cap = n;
    }
    return build_cep_tables(h, alphas, n, h->sweep.tables);
}

// apply() for the current block: n_alpha == 0 -> the handle's alpha into d_src/d_blk (ParamBase::apply);
// n_alpha >= 1 -> every alpha of the list from the same stored spectrum, alpha a into block a of
// d_sweep_src/d_sweep_blk (the reference's alpha loop ASR_OCL.cpp:236-243 as one launch per stage).
int apply_impl(mfx_handle *h, const float *alphas, int n_alpha)
{
    HIP_TRY(h, hipSetDevice(h->device));
    const int D = h->D;
    int wcnd, wc;
    bool first = false, last = false, use_last = false;
    // the three cases of mfcccpu.cpp:371-425
    if (h->st.last_block) {
        wcnd = estimated_window_count_f32(h->st.remaining, h->W, h->S);
        wc = wcnd - D;
        last = true;
        use_last = true;
        if (wc <= 0) return MFX_OK;
    } else if (h->st.last_calc_flushed) {
        wcnd = estimated_window_count_f32(h->st.samples, h->W, h->S);
        wc = wcnd - D;
        first = true;
        if (wc <= 0) return fail(h, MFX_ERR_WINDOW_COUNT, kMsgWindow);
    } else {
        wcnd = estimated_window_count_f32(h->st.samples, h->W, h->S);
        wc = wcnd - 2 * D;
        if (wc <= 0) return MFX_OK;
    }
    if (wcnd > h->cap_rows) return fail(h, MFX_ERR_WINDOW_HIGH, kMsgHigh);

    const bool sweep = n_alpha > 0;
    const int n_tab = sweep ? n_alpha : 1;
    int rc = sweep ? prepare_sweep(h, alphas, n_alpha) : refresh_mel(h);
    if (rc != MFX_OK) return rc;
    float *d_src = sweep ? h->sweep.d_src.p : h->st.d_src.p;
    float *d_blk = sweep ? h->sweep.d_blk.p : h->st.d_blk.p;
    float *d_stats = sweep ? h->sweep.d_stats.p : h->st.d_stats.p;

    // cepstra over all frames with context
    rc = launch_cepstra(h, sweep ? h->sweep.tables : h->own, h->d_spec.p, wcnd, d_src, h->cols, n_tab, (int64_t)h->cap_rows * h->cols,
                        sweep ? nullptr : h->st.d_plp_r.p, h->stream);
    if (rc != MFX_OK) return rc;

    // static row offset as the reference reads it (mfcccpu.cpp:274,439): was_flushed() ? 0 : D.
    // With bug_compat off a flush block always reads at D (fixes B1).
    bool at_zero = h->st.last_calc_flushed;
    if (!h->cfg.bug_compat && h->st.last_block) at_zero = false;
    const int static_off = at_zero ? 0 : D;

    Segment sg{}; // rows with context (statics), used by the normalisation before the deltas
    sg.n_out = wcnd;
    Segment sd{}; // the block's delivered rows
    sd.n_out = wc;
    sd.static_off = static_off;
    if (first) { // D replicated rows in front (mfcccpu.cpp:243-248)
        sd.shift = -D;
        sd.lo = 0;
        sd.hi = wcnd - 1;
    } else if (last) { // D replicated rows behind (mfcccpu.cpp:249-254)
        sd.shift = 0;
        sd.lo = 0;
        sd.hi = wc + D - 1;
    } else {
        sd.shift = 0;
        sd.lo = 0;
        sd.hi = wcnd - 1;
    }
    const Segment *segs_ctx = nullptr, *segs_out = nullptr;
    if (sweep) { // one segment per alpha: block a of the sweep buffers
        std::vector<Segment> hs((size_t)2 * n_alpha);
        for (int a = 0; a < n_alpha; ++a) {
            hs[a] = sg;
            hs[a].src_row0 = hs[a].out_row0 = (int64_t)a * h->cap_rows;
            hs[n_alpha + a] = sd;
            hs[n_alpha + a].src_row0 = hs[n_alpha + a].out_row0 = (int64_t)a * h->cap_rows;
        }
        HIP_TRY(h, hipMemcpyAsync(h->sweep.d_segs.p, hs.data(), hs.size() * sizeof(Segment), hipMemcpyHostToDevice,
                                  h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream)); // hs is a local
        segs_ctx = h->sweep.d_segs.p;
        segs_out = h->sweep.d_segs.p + n_alpha;
    }

    const bool norm = h->cfg.norm != MFX_NORM_NONE;
    if (norm && !h->cfg.norm_after_dyn) { // normalise statics (with context) before the deltas
        rc = run_norm(h, h->stream, d_src, h->cols, segs_ctx, n_tab, sweep ? nullptr : &sg, d_stats, use_last, wcnd);
        if (rc != MFX_OK) return rc;
    }

    // Small blocks (round 4): the delta kernel -- the last one that touches the rows unless they are normalised after the
    // deltas -- writes them straight into the page-locked staging buffer (posted writes over the link, consecutive
    // threads on consecutive addresses), and get_output_data has nothing to launch: one kernel and one launch less per
    // call sequence (profiles/r04/stream_small_timeline.txt).  Same kernel, same values: the same bits as through d_blk.
    // Only a plain apply (and set_input / flush) changes rows_in_stage: a sweep writes d_sweep_blk and leaves the plain
    // rows -- in h_out_stage or in d_blk -- for get_output_data as they are.
    if (!sweep) h->st.rows_in_stage = false;
    float *rows_out = d_blk;
    // (not when the rows are normalised after the deltas: the one-launch normaliser is ONE block per segment, and a
    // single CU writing 155 KB over the link takes what the copy kernel it would save takes -- measured, +- 0.5 us)
    if (!sweep && !(norm && h->cfg.norm_after_dyn) && small_block(h, (size_t)wc * h->width * sizeof(float))) {
        const size_t want = (size_t)h->cap_rows * h->width + 4;
        HIP_TRY(h, h->st.h_out_stage.grow(want, want, h->stream));
        void *dev = nullptr;
        if (is_pinned_host(h->st.h_out_stage.p, &dev) && dev) {
            rows_out = (float *)dev;
            h->st.rows_in_stage = true;
        }
    }
    DeltaParams dp;
    fill_delta(h, dp);
    dp.src = d_src;
    dp.src_pitch = h->cols;
    dp.out = rows_out;
    dp.segs = segs_out;
    dp.n_segs = n_tab;
    dp.tiles_per_seg_max = (wc + 63) / 64;
    dp.inline_seg = sweep ? 0 : 1;
    dp.seg0 = sd;
    HIP_TRY(h, launch_delta(dp, h->stream));

    if (norm && h->cfg.norm_after_dyn) {
        const int groups = h->width / h->cols;
        rc = run_norm(h, h->stream, d_blk, h->width, segs_out, n_tab, sweep ? nullptr : &sd, d_stats, use_last, wc, groups,
                      (size_t)n_tab * 2 * h->cols);
        if (rc != MFX_OK) return rc;
    }
    if (sweep) h->sweep.n = n_alpha; // a plain apply leaves the sweep's rows readable
    return MFX_OK;
}

} // namespace

extern "C" int mfx_apply(mfx_handle *h)
{
    MFX_DEVICE_ENTRY(h);
    MFX_STREAM_ENTRY(h);
    return apply_impl(h, nullptr, 0);
}

extern "C" int mfx_apply_alphas(mfx_handle *h, const float *alphas, int32_t n_alpha)
{
    MFX_DEVICE_ENTRY(h);
    MFX_STREAM_ENTRY(h);
    if (!alphas || n_alpha < 1 || n_alpha > 4096) return fail(h, MFX_ERR_ARG, "invalid argument");
    for (int a = 0; a < n_alpha; ++a)
        if (!(alphas[a] > 0.f)) return fail(h, MFX_ERR_ARG, "alpha must be positive");
    return apply_impl(h, alphas, n_alpha);
}

extern "C" int mfx_get_output_data_alpha(mfx_handle *h, int32_t alpha_index, float *data_out, int32_t frames)
{
    MFX_DEVICE_ENTRY(h);
    MFX_STREAM_ENTRY(h);
    if ((!data_out && frames > 0) || frames < 0) return fail(h, MFX_ERR_ARG, "invalid argument");
    if (h->sweep.n == 0) return fail(h, MFX_ERR_STATE, "no sweep on the current block");
    if (alpha_index < 0 || alpha_index >= h->sweep.n) return fail(h, MFX_ERR_ARG, "alpha index outside the last sweep");
    if (frames > h->cap_rows) return fail(h, MFX_ERR_WINDOW_HIGH, kMsgHigh);
    if (frames == 0) return MFX_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    // (own staging buffer: h_out_stage may hold the plain rows that get_output_data returns next)
    return download_rows(h, data_out, h->sweep.d_blk.p + (size_t)alpha_index * h->cap_rows * h->width, (size_t)frames * h->width,
                         h->sweep.h_stage);
}

extern "C" int mfx_get_output_data(mfx_handle *h, float *data_out, int32_t frames)
{
    MFX_DEVICE_ENTRY(h);
    MFX_STREAM_ENTRY(h);
    if ((!data_out && frames > 0) || frames < 0) return fail(h, MFX_ERR_ARG, "invalid argument");
    if (frames > h->cap_rows) return fail(h, MFX_ERR_WINDOW_HIGH, kMsgHigh);
    if (frames == 0) return MFX_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->st.rows_in_stage) { // the delta kernel wrote the rows into page-locked memory: wait for it, copy
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        std::memcpy(data_out, h->st.h_out_stage.p, (size_t)frames * h->width * sizeof(float));
        return MFX_OK;
    }
    return download_rows(h, data_out, h->st.d_blk.p, (size_t)frames * h->width, h->st.h_out_stage);
}
