// mfx_batch_plan.cpp -- the planners of the batch interface of include/mfx.h: chunks and segments of an utterance list
// (mfx_batch_plan), the same behind a sample-rate converter (mfx_batch_plan_rates), the fused-delta plan.  Running
// a plan is mfx_batch.cpp, what is attached to one mfx_batch_attach.cpp.  This file owns the plan proper of the handle's
// `batch`, its `rs` and `fuse`.
#include "mfx_handle.h"

using namespace mfx;

extern "C" int64_t mfx_batch_frames(const mfx_handle *h, int64_t samples)
{
    if (!h) return MFX_ERR_ARG;
    int64_t t = utt_frame_count(h, samples);
    return t > 0 ? t : 0;
}

namespace {

// pieces of equal FRAME count for B blocks (the tail of the chunk list holds 4-frame chunks): cut[b] = first chunk of block b
std::vector<size_t> fuse_piece_cuts(const std::vector<Chunk> &chunks, int B)
{
    const size_t n = chunks.size();
    std::vector<size_t> cut((size_t)B + 1, n);
    int64_t total = 0;
    for (const Chunk &c : chunks) total += c.n_frames;
    int64_t acc = 0;
    size_t c = 0;
    for (int b = 0; b < B; ++b) {
        cut[b] = c;
        const int64_t target = total * (b + 1) / B;
        while (c < n && acc + chunks[c].n_frames <= target) acc += chunks[c++].n_frames;
        if (b + 1 == B) c = n;
    }
    cut[0] = 0;
    return cut;
}

Chunk halo_chunk(int64_t pcm_off, int64_t row, int frames)
{
    Chunk c;
    c.pcm_off = pcm_off;
    c.out_row = row;
    c.n_frames = frames;
    c.pad = 0;
    return c;
}

// tiles over a block's own chunks -- fch[own0, own1) of the `cnt` chunks at fch (plan chunks c0 ...): runs of one utterance,
// <= 64 rows each
void fuse_block_tiles(const mfx_handle *h, const Chunk *fch, size_t cnt, size_t own0, size_t own1, size_t c0, std::vector<DeltaTile> &tiles)
{
    const std::vector<int64_t> &T_of = h->batch.utt_frames;
    const std::vector<int32_t> &utt_of = h->batch.chunk_utt;
    const int D = h->D;
    auto local_of_row = [&](int64_t r, size_t hint) -> int32_t { // block-local chunk that holds row r
        size_t k = hint;
        while (k > 0 && fch[k].out_row > r) --k;
        while (k + 1 < cnt && fch[k].out_row + fch[k].n_frames <= r) ++k;
        return (int32_t)k;
    };
    size_t k = own0;
    while (k < own1) {
        const int u = utt_of[c0 + (k - own0)];
        const int64_t r0 = fch[k].out_row;
        int64_t rows = 0;
        size_t k2 = k;
        while (k2 < own1 && utt_of[c0 + (k2 - own0)] == u && rows + fch[k2].n_frames <= 64) {
            rows += fch[k2].n_frames;
            ++k2;
        }
        const int64_t u0 = h->batch.utt_row[u], u1 = u0 + T_of[u];
        DeltaTile t{};
        t.out_row0 = r0;
        t.seg_row0 = u0;
        t.n_rows = (int32_t)rows;
        t.r0 = (int32_t)(r0 - u0);
        t.shift = -D;           // whole utterance: D replicated rows on both sides (as the batch Segment)
        t.lo = 0;
        t.hi = (int32_t)(T_of[u] - 1);
        t.static_off = 0;
        t.dep_lo = local_of_row(std::max(r0 - D, u0), k);
        t.dep_hi = local_of_row(std::min(r0 + rows + D, u1) - 1, k2 - 1);
        tiles.push_back(t);
        k = k2;
    }
}

// Plan of the fused front end + delta stage (k_front512<..., FUSE>).  The global chunk list is cut into
// B contiguous pieces, one per block; a piece that starts or ends inside an utterance gets a halo chunk of
// D frames on that side (both neighbours compute those statics; identical values land on the same
// scratch rows).  The block's own rows are grouped into tiles of <= 64 rows of one utterance; each tile
// names the block-local chunks whose statics it reads.
int plan_fused_delta(mfx_handle *h)
{
    const std::vector<int64_t> &T_of = h->batch.utt_frames;
    h->fuse.planned = false;
    const size_t n = h->batch.h_chunks.size();
    // (asked for: any batch; not asked for: batches of kFuseMinFrames .. kFuseMaxFrames frames -- decide_mode has the rest of
    // that gate)
    int64_t frames = 0;
    for (const int64_t T : T_of) frames += T;
    if (h->fuse.off || (!h->fuse.enabled && (frames < kFuseMinFrames || frames > kFuseMaxFrames))) return MFX_OK;
    if (!h->fast512 || h->stuff256 || h->channels != 1 || h->l1 <= 0 || h->cols > 16 || h->ceps <= 0 || h->D > 16 || n == 0 ||
        n > 0x3fffffff || (h->cfg.norm != MFX_NORM_NONE && !h->cfg.norm_after_dyn))
        return MFX_OK;
    const int D = h->D;
    const int B = (int)std::min<size_t>((size_t)h->num_cus, (n + 14) / 15);
    const std::vector<int32_t> &utt_of = h->batch.chunk_utt; // utterance of every chunk
    std::vector<Chunk> fch;
    fch.reserve(n + 2 * (size_t)B);
    std::vector<DeltaTile> tiles;
    std::vector<int32_t> coff((size_t)B + 1), toff((size_t)B + 1);
    size_t max_list = 0;
    const std::vector<size_t> cut = fuse_piece_cuts(h->batch.h_chunks, B);
    for (int b = 0; b < B; ++b) {
        const size_t c0 = cut[b], c1 = cut[b + 1];
        coff[b] = (int32_t)fch.size();
        toff[b] = (int32_t)tiles.size();
        if (c1 <= c0) continue;
        const size_t base = fch.size();
        const Chunk &f = h->batch.h_chunks[c0], &l = h->batch.h_chunks[c1 - 1];
        if (const int64_t avail = f.out_row - h->batch.utt_row[utt_of[c0]]; avail > 0) { // halo in front
            const int hal = (int)std::min<int64_t>(D, avail);
            fch.push_back(halo_chunk(f.pcm_off - (int64_t)hal * h->S, f.out_row - hal, hal));
        }
        const size_t own0 = fch.size() - base; // local index of the first own chunk
        for (size_t c = c0; c < c1; ++c) fch.push_back(h->batch.h_chunks[c]);
        const int u = utt_of[c1 - 1];
        const int64_t end_row = l.out_row + l.n_frames;
        if (const int64_t avail = h->batch.utt_row[u] + T_of[u] - end_row; avail > 0) // halo behind
            fch.push_back(halo_chunk(l.pcm_off + (int64_t)l.n_frames * h->S, end_row, (int)std::min<int64_t>(D, avail)));
        const size_t cnt = fch.size() - base;
        max_list = std::max(max_list, cnt);
        fuse_block_tiles(h, fch.data() + base, cnt, own0, own0 + (c1 - c0), c0, tiles);
        // the block's claim word counts its tiles in 16 bits (claim_init): a list beyond that -- tens of thousands of
        // utterances of a frame or two per block -- takes the separate delta kernel
        if (tiles.size() - (size_t)toff[b] > (size_t)kClaimMaxTiles) return MFX_OK;
    }
    coff[B] = (int32_t)fch.size();
    toff[B] = (int32_t)tiles.size();
    {   // one padding entry: the delta wave prefetches the descriptor after its last tile
        DeltaTile t{};
        tiles.push_back(t);
    }
    const int done_words = (int)((max_list + 31) / 32) + 1;
    FrontParams probe;
    fill_front(h, probe);
    probe.dl1 = h->l1;
    probe.dl2 = h->l2;
    probe.done_words = done_words;
    if (!h->plan16.ok || probe.dct_mode != 1 || front512_delta_lds_bytes(probe) > kLdsCap) return MFX_OK;
    HIP_TRY(h, h->upload(h->fuse.d_chunks, fch));
    HIP_TRY(h, h->upload(h->fuse.d_blk_chunk_off, coff));
    HIP_TRY(h, h->upload(h->fuse.d_blk_tile_off, toff));
    HIP_TRY(h, h->upload(h->fuse.d_tiles, tiles));
    if (!h->fuse.d_err.p) {
        HIP_TRY(h, h->fuse.d_err.alloc(1));
        HIP_TRY(h, hipMemset(h->fuse.d_err.p, 0, sizeof(int32_t)));
    }
    h->fuse.blocks = B;
    h->fuse.done_words = done_words;
    h->fuse.nchunks = (int32_t)fch.size();
    h->fuse.planned = true;
    return MFX_OK;
}

} // namespace

// scratch for the compact statics of the planned batch: one buffer, two with overlap on (grown, never shrunk)
int size_static16(mfx_handle *h)
{
    const size_t need = (size_t)h->batch.total_rows * 16;
    for (int b = 0; b < (h->batch.ov.enabled ? 2 : 1); ++b)
        if (h->l1 > 0 && h->cols <= 16 && !h->traps && h->batch.d_static16[b].n < need) HIP_TRY(h, h->batch.d_static16[b].alloc(need));
    return MFX_OK;
}

namespace {
// The 512-point kernel deals chunks to the 16 waves of each block as they become free; with 16-frame
// chunks a wave can sit idle for most of a chunk time (~34 us on C2) at the end of the launch.  The last two
// chunks of every wave of the grid are therefore cut into 4-frame pieces (one kernel iteration each).
// (k_front2048: 12 waves per CU, each 16-frame chunk is 8 iterations of ~10 us -- on C5 a wave sees only ~4 chunks in
// all, so the last ONE per wave is cut, and a launch twice that long already qualifies)
void split_tail_chunks(mfx_handle *h)
{
    const int ts = h->cfg.tail_split;
    const bool f2048 = h->fast2048 && h->plan32.ok; // (stereo, mono on aligned pairs, mono at any alignment: all three builds)
    if ((h->fast512 || (h->fast1024 && h->plan16.ok) || f2048) && ts >= 0) {
        const size_t n = h->batch.h_chunks.size();
        const size_t tail = std::min<size_t>(n, (size_t)(ts > 0 ? std::min(ts, 64) : f2048 ? 1 : 2) * (f2048 ? 12 : 16) * h->num_cus);
        if (n >= (f2048 ? 2 : 4) * tail) { // only when the launch is long enough for the tail to matter
            std::vector<Chunk> cut;
            std::vector<int32_t> cut_utt;
            for (size_t c = n - tail; c < n; ++c) {
                const Chunk &src = h->batch.h_chunks[c];
                for (int f = 0; f < src.n_frames; f += 4) {
                    Chunk q = src;
                    q.pcm_off = src.pcm_off + (int64_t)f * h->S;
                    q.out_row = src.out_row + f;
                    q.n_frames = std::min(4, src.n_frames - f);
                    cut.push_back(q);
                    cut_utt.push_back(h->batch.chunk_utt[c]);
                }
            }
            h->batch.h_chunks.resize(n - tail);
            h->batch.chunk_utt.resize(n - tail);
            h->batch.h_chunks.insert(h->batch.h_chunks.end(), cut.begin(), cut.end());
            h->batch.chunk_utt.insert(h->batch.chunk_utt.end(), cut_utt.begin(), cut_utt.end());
        }
    }
}
} // namespace

extern "C" int mfx_batch_plan(mfx_handle *h, int32_t n_utt, const int64_t *offsets, const int64_t *lengths,
                              int64_t *out_rows, int64_t *total_rows)
{
    MFX_DEVICE_ENTRY(h);
    const int rc = plan_batch(h, n_utt, offsets, lengths, out_rows, total_rows);
    // (refused arguments leave the previous plan, and its converter, as they were; otherwise plan_batch has waited for the stream)
    if (rc == MFX_OK || !h->batch.planned) h->batch.rs.drop();
    return rc;
}

int plan_batch(mfx_handle *h, int32_t n_utt, const int64_t *offsets, const int64_t *lengths, int64_t *out_rows, int64_t *total_rows)
{
    if (n_utt < 0 || (n_utt > 0 && (!offsets || !lengths))) return fail(h, MFX_ERR_ARG, "invalid argument");
    for (int u = 0; u < n_utt; ++u) { // (the whole list before anything of the previous plan is touched)
        if (offsets[u] < 0 || lengths[u] < 0) return fail(h, MFX_ERR_ARG, "negative utterance offset/length");
        if (utt_frame_count(h, lengths[u]) > 0x7fffffff) return fail(h, MFX_ERR_ARG, "utterance too long");
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->batch.detach(); // (a warp-factor list, a transform's utterance index and scratch, a speaker list, the VAD, the tensor output: tied to the plan)
    h->batch.planned = false;
    h->batch.n_utt = n_utt;
    h->batch.utt_off.assign(offsets, offsets + n_utt);
    h->batch.utt_len.assign(lengths, lengths + n_utt);
    h->batch.utt_row.resize(n_utt);
    h->batch.h_chunks.clear();
    h->batch.chunk_utt.clear();
    h->batch.h_stft_chunks.clear();
    // (STFT log-mel: a chunk is the run of frames one block of k_stft_mel takes)
    const int chunk_frames = h->stft ? h->stft_R : kChunkFrames;
    // (a Kaldi handle with snip_edges = false: a chunk starts at the UNREFLECTED first tap of its first frame, which may lie in
    // front of the utterance, and names its utterance in `pad`; k_kaldi_front mirrors the span into the utterance's bounds)
    const bool centred = h->kaldi && (h->kaldi_flags & kKaldiNoSnipEdges);
    std::vector<Segment> segs((size_t)n_utt);
    std::vector<int64_t> &T_of = h->batch.utt_frames;
    T_of.assign((size_t)n_utt, 0);
    int64_t row = 0;
    int tiles_max = 0;
    bool aligned = (h->S % 2) == 0;
    for (int u = 0; u < n_utt; ++u) {
        const int64_t T = std::max<int64_t>(utt_frame_count(h, lengths[u]), 0);
        h->batch.utt_row[u] = row;
        T_of[u] = T;
        if (out_rows) out_rows[u] = row;
        if (offsets[u] & 1) aligned = false;
        if (h->stft && (T + chunk_frames - 1) / chunk_frames + (int64_t)h->batch.h_chunks.size() > 0x7ffffff0) {
            h->batch.n_utt = 0, h->batch.total_rows = 0;
            return fail(h, MFX_ERR_ARG, "batch too long");
        }
        for (int64_t t0 = 0; t0 < T; t0 += chunk_frames) {
            Chunk c;
            c.pcm_off = offsets[u] + (centred ? kaldi_centred_start(t0, h->W, h->S) : t0 * h->S);
            c.out_row = row + t0;
            c.n_frames = (int32_t)std::min<int64_t>(chunk_frames, T - t0);
            c.pad = centred ? u : 0;
            if (h->stft) {
                const int32_t first = (int32_t)(h->batch.h_chunks.size() - (size_t)(t0 / chunk_frames)), count = (int32_t)((T + chunk_frames - 1) / chunk_frames);
                h->batch.h_stft_chunks.push_back(make_stft_chunk(offsets[u], lengths[u], c.out_row, (int32_t)t0, c.n_frames, first, count));
            }
            h->batch.h_chunks.push_back(c);
            h->batch.chunk_utt.push_back(u);
        }
        Segment &s = segs[u]; // (all zero so far)
        s.src_row0 = row;
        s.out_row0 = row;
        s.n_out = (int32_t)T;
        s.shift = -h->D; // whole utterance: D replicated rows on both sides
        s.lo = 0;
        s.hi = (int32_t)std::max<int64_t>(T - 1, 0);
        s.static_off = 0;
        // Statistics of the normaliser (norm after dyn): the reference, fed the utterance as ONE block (its default
        // sample_limit holds ~10 minutes of audio), computes them over the T - D rows that block delivers and
        // re-uses them for the D rows of the flush (mfcccpu.cpp:377-388,395-407; normalizercpu.cpp:22-27).  That is
        // the default here too (batch_norm_stats = 0); 1 = over all T rows.  Normalisation before the deltas covers
        // the block's T rows with context in the reference as well, i.e. all rows either way.
        s.pad = (h->cfg.norm != MFX_NORM_NONE && h->cfg.norm_after_dyn && h->cfg.batch_norm_stats == 0 && T > h->D)
                    ? (int32_t)(T - h->D) : 0;
        tiles_max = std::max<int>(tiles_max, (int)((T + 63) / 64));
        row += T;
    }
    split_tail_chunks(h);
    h->batch.utt_chunk0.assign((size_t)n_utt + 1, (int32_t)h->batch.h_chunks.size());
    for (size_t c = h->batch.h_chunks.size(); c-- > 0;) h->batch.utt_chunk0[h->batch.chunk_utt[c]] = (int32_t)c;
    for (int u = n_utt - 1; u >= 0; --u) // utterances without frames: empty chunk range
        if (h->batch.utt_chunk0[u] > h->batch.utt_chunk0[u + 1]) h->batch.utt_chunk0[u] = h->batch.utt_chunk0[u + 1];
    h->batch.total_rows = row;
    h->batch.tiles_max = tiles_max;
    h->batch.aligned = aligned;
    if (total_rows) *total_rows = row;
    HIP_TRY(h, h->upload(h->batch.d_chunks, h->batch.h_chunks));
    HIP_TRY(h, h->upload(h->batch.d_segs, segs));
    if (centred) {
        std::vector<int64_t> bounds((size_t)n_utt * 2);
        for (int u = 0; u < n_utt; ++u) bounds[2 * (size_t)u] = offsets[u], bounds[2 * (size_t)u + 1] = lengths[u];
        HIP_TRY(h, h->upload(h->d_kaldi_bounds, bounds));
    }
    if (h->cfg.norm != MFX_NORM_NONE) {
        HIP_TRY(h, h->batch.d_stats.alloc((size_t)n_utt * 3 * 2 * h->cols));
        const size_t need = norm_partial_doubles(n_utt, tiles_max * 64, h->cols);
        if (need > h->d_norm_partial.n) HIP_TRY(h, h->d_norm_partial.alloc(need));
    }
    int rcf = plan_fused_delta(h);
    if (rcf != MFX_OK) return rcf;
    // (allocated here so that mfx_batch_run_device itself never allocates)
    if (h->traps) { // log mel rows between the front end and k_traps (grown, never shrunk)
        h->batch.mel_pitch = (h->nb + 3) & ~3;
        const size_t need = (size_t)row * h->batch.mel_pitch;
        if (h->batch.d_logmel.n < need) HIP_TRY(h, h->batch.d_logmel.alloc(need));
    }
    if (h->stft) { // the blocks' descriptors and their slots for the utterance maximum (grown, never shrunk)
        HIP_TRY(h, h->upload(h->batch.d_stft_chunks, h->batch.h_stft_chunks));
        if (h->batch.d_stft_max.n < h->batch.h_stft_chunks.size()) HIP_TRY(h, h->batch.d_stft_max.alloc(h->batch.h_stft_chunks.size()));
    }
    rcf = size_static16(h);
    h->batch.planned = rcf == MFX_OK;
    return rcf;
}

// ------------------------------------------------------------------------------------------------
// sample-rate conversion in front of the batch ("Sample-rate conversion")
// ------------------------------------------------------------------------------------------------

extern "C" int mfx_batch_plan_rates(mfx_handle *h, int32_t n_utt, const int64_t *offsets, const int64_t *lengths, const int32_t *rates_hz,
                                    int32_t zeros, float rolloff, int64_t *out_rows, int64_t *total_rows)
{
    MFX_DEVICE_ENTRY(h);
    if (n_utt < 0 || (n_utt > 0 && (!offsets || !lengths || !rates_hz))) return fail(h, MFX_ERR_ARG, "invalid argument");
    // (the range first: a float outside int32 must not reach the cast)
    if (!(h->cfg.sample_rate >= 1000.f && h->cfg.sample_rate <= 768000.f))
        return fail(h, MFX_ERR_ARG, "sample rates must lie in 1000 .. 768000 Hz");
    const int32_t out_hz = (int32_t)h->cfg.sample_rate;
    if ((float)out_hz != h->cfg.sample_rate) return fail(h, MFX_ERR_CONFIG, "mfx_batch_plan_rates: sample_rate is not an integral number of Hz");
    // the distinct input rates, in order of first appearance: one table each (none for the output rate itself)
    std::vector<int32_t> distinct;
    std::vector<int32_t> rate_of((size_t)n_utt);
    for (int u = 0; u < n_utt; ++u) {
        if (offsets[u] < 0 || lengths[u] < 0) return fail(h, MFX_ERR_ARG, "negative utterance offset/length");
        if (rates_hz[u] < 1000 || rates_hz[u] > 768000) return fail(h, MFX_ERR_ARG, "sample rates must lie in 1000 .. 768000 Hz");
        size_t k = 0;
        while (k < distinct.size() && distinct[k] != rates_hz[u]) ++k;
        if (k == distinct.size()) {
            if (distinct.size() == 16) return fail(h, MFX_ERR_ARG, "more than 16 distinct input rates in one plan");
            distinct.push_back(rates_hz[u]);
        }
        rate_of[u] = (int32_t)k;
    }
    // (zeros and rolloff are not judged for the output rate itself: a plan whose utterances all have it takes any)
    ResRateSet set;
    if (const int e = build_resample_rates(h->channels, out_hz, distinct.data(), (int)distinct.size(), zeros, rolloff, false, set); e != 0)
        return fail(h, MFX_ERR_ARG, kResampleWhy[e]);
    const std::vector<ResRate> &rates = set.rates;
    std::vector<int64_t> sc_off((size_t)n_utt), sc_len((size_t)n_utt);
    const int64_t sc_total = resample_layout(n_utt, lengths, rates_hz, out_hz, sc_off.data(), sc_len.data());
    if (sc_total < 0) return fail(h, MFX_ERR_ARG, "invalid argument");
    std::vector<ResTile> tiles;
    std::vector<int32_t> tile0((size_t)n_utt + 1);
    for (int u = 0; u < n_utt; ++u) {
        tile0[u] = (int32_t)tiles.size();
        const ResRate &r = rates[rate_of[u]];
        const int64_t step = r.tile_out > 0 ? r.tile_out : kResCopyTile;
        if ((sc_len[u] + step - 1) / step + (int64_t)tiles.size() > 0x7ffffff0) return fail(h, MFX_ERR_ARG, "batch too long");
        for (int64_t j0 = 0; j0 < sc_len[u]; j0 += step) {
            ResTile t{};
            t.in_off = offsets[u], t.out_off = sc_off[u], t.n_in = lengths[u], t.n_out = sc_len[u], t.j0 = j0;
            t.rate = r.tile_out > 0 ? rate_of[u] : -1;
            tiles.push_back(t);
        }
    }
    tile0[n_utt] = (int32_t)tiles.size();
    if (resample_lds_bytes(h->channels, set.lds) > kLdsCap) return fail(h, MFX_ERR_ARG, "no tile of k_resample fits the LDS for this shape");

    int rc = plan_batch(h, n_utt, sc_off.data(), sc_len.data(), out_rows, total_rows); // (waits for the stream)
    h->batch.rs.on = false; // (not drop(): the scratch is grown, never shrunk, and the tables are replaced below)
    if (rc != MFX_OK) return rc;
    h->batch.planned = false;
    if (tiles.empty()) tiles.push_back(ResTile{});
    HIP_TRY(h, h->upload(h->batch.rs.d_taps, set.taps));
    HIP_TRY(h, h->upload(h->batch.rs.d_rates, rates));
    HIP_TRY(h, h->upload(h->batch.rs.d_tiles, tiles));
    // (allocated here so that mfx_batch_run_device itself never allocates; 8 elements of padding: the front ends read the
    // 32-bit word that holds the last sample)
    const size_t need = (size_t)sc_total * h->channels + 8;
    if (h->batch.rs.d_pcm.n < need) {
        HIP_TRY(h, h->batch.rs.d_pcm.alloc(need));
        HIP_TRY(h, hipMemset(h->batch.rs.d_pcm.p, 0, need * sizeof(int16_t)));
    }
    h->batch.rs.in_off.assign(offsets, offsets + n_utt);
    h->batch.rs.in_len.assign(lengths, lengths + n_utt);
    h->batch.rs.utt_tile0.swap(tile0);
    h->batch.rs.total = sc_total;
    h->batch.rs.lds = set.lds;
    h->batch.rs.on = true;
    h->batch.planned = true;
    return MFX_OK;
}

extern "C" int mfx_batch_resample_layout(const mfx_handle *h, int64_t *offsets, int64_t *lengths, int64_t *total)
{
    if (!h) return MFX_ERR_ARG;
    if (h->planning) return fail(const_cast<mfx_handle *>(h), MFX_ERR_DEVICE, "planning handle (mfx_plan_create): no device behind it");
    if (!h->batch.rs.on) return fail(const_cast<mfx_handle *>(h), MFX_ERR_STATE, "mfx_batch_resample_layout: no rates plan is in force");
    if (offsets) std::copy(h->batch.utt_off.begin(), h->batch.utt_off.end(), offsets);
    if (lengths) std::copy(h->batch.utt_len.begin(), h->batch.utt_len.end(), lengths);
    if (total) *total = h->batch.rs.total;
    return MFX_OK;
}

// the fused delta stage: what the plan and the runs so far say (unstable, like the engine bits that steer it)
extern "C" int mfx_batch_fuse_info(const mfx_handle *h, int32_t *planned, int32_t *share, int64_t *runs, int64_t *min_frames,
                                   int64_t *max_frames)
{
    if (!h) return MFX_ERR_ARG;
    if (planned) *planned = h->fuse.planned ? 1 : 0;
    if (share) *share = delta_share_fits(h->l1, h->l2) ? h->fuse.share : 0;
    if (runs) *runs = h->fuse.runs;
    if (min_frames) *min_frames = kFuseMinFrames;
    if (max_frames) *max_frames = kFuseMaxFrames;
    return MFX_OK;
}

extern "C" int32_t mfx_host_delta_tile_lds_floats(int32_t rows, int32_t l1, int32_t l2, int32_t *shares)
{
    if (shares) *shares = delta_share_fits(l1, l2) ? 1 : 0;
    return delta_tile_lds_floats(rows, l1, l2);
}

extern "C" int64_t mfx_host_fuse_claim(int64_t word, int32_t from_head, int32_t *tile)
{
    if (!tile) return -1;
    if (word < 0) return *tile >= 0 && *tile <= kClaimMaxTiles ? (int64_t)claim_init(*tile) : -1;
    const uint32_t w = (uint32_t)word;
    if (claim_empty(w)) {
        *tile = -1;
        return word;
    }
    *tile = from_head ? claim_head_tile(w) : claim_tail_tile(w);
    return (int64_t)(from_head ? claim_take_head(w) : claim_take_tail(w));
}
