// mfx_batch.cpp -- the batch interface of include/mfx.h: planner (chunks, segments, the opt-in fused-delta plan) and runner
// (device and host entries, overlap of a batch's tail with the next front end).  Which front end runs is choose_front's
// decision (mfx_api.cpp).  This file owns the handle's `batch` and `fuse` parts and names no field of `st` or `sweep`.
#include "mfx_handle.h"

using namespace mfx;

// ------------------------------------------------------------------------------------------------
// batch interface
// ------------------------------------------------------------------------------------------------

extern "C" int64_t mfx_batch_frames(const mfx_handle *h, int64_t samples)
{
    if (!h) return MFX_ERR_ARG;
    int64_t t = frame_count(samples, h->W, h->S);
    return t > 0 ? t : 0;
}

namespace {

// one launch of the dominant kernel between two events, while profiling is on (prof_collect, mfx_api.cpp, sums them up)
struct ProfScope {
    mfx_handle *h;
    hipEvent_t a = nullptr, b = nullptr;
    explicit ProfScope(mfx_handle *hh) : h(hh)
    {
        if (!h->prof.on) return;
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

// Plan of the fused front end + delta stage (k_front512<..., FUSE>).  The global chunk list is cut into
// B contiguous pieces, one per block; a piece that starts or ends inside an utterance gets a halo chunk of
// D frames on that side (both neighbours compute those statics; identical values land on the same
// scratch rows).  The block's own rows are grouped into tiles of <= 64 rows of one utterance; each tile
// names the block-local chunks whose statics it reads.
int plan_fused_delta(mfx_handle *h, const std::vector<int64_t> &T_of)
{
    h->fuse.planned = false;
    const size_t n = h->batch.h_chunks.size();
    if (!h->fuse.enabled || !h->fast512 || h->stuff256 || h->channels != 1 || h->l1 <= 0 || h->cols > 16 || h->ceps <= 0 || h->D > 16 || n == 0 ||
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
    // pieces of equal FRAME count (the tail of the chunk list holds 4-frame chunks): cut[b] = first chunk of block b
    std::vector<size_t> cut((size_t)B + 1, n);
    {
        int64_t total = 0;
        for (const Chunk &c : h->batch.h_chunks) total += c.n_frames;
        int64_t acc = 0;
        size_t c = 0;
        for (int b = 0; b < B; ++b) {
            cut[b] = c;
            const int64_t target = total * (b + 1) / B;
            while (c < n && acc + h->batch.h_chunks[c].n_frames <= target) acc += h->batch.h_chunks[c++].n_frames;
            if (b + 1 == B) c = n;
        }
        cut[0] = 0;
    }
    for (int b = 0; b < B; ++b) {
        const size_t c0 = cut[b], c1 = cut[b + 1];
        coff[b] = (int32_t)fch.size();
        toff[b] = (int32_t)tiles.size();
        if (c1 <= c0) continue;
        const size_t base = fch.size();
        {   // halo in front
            const Chunk &f = h->batch.h_chunks[c0];
            const int64_t avail = f.out_row - h->batch.utt_row[utt_of[c0]];
            if (avail > 0) {
                const int hal = (int)std::min<int64_t>(D, avail);
                Chunk c;
                c.pcm_off = f.pcm_off - (int64_t)hal * h->S;
                c.out_row = f.out_row - hal;
                c.n_frames = hal;
                c.pad = 0;
                fch.push_back(c);
            }
        }
        const size_t own0 = fch.size() - base; // local index of the first own chunk
        for (size_t c = c0; c < c1; ++c) fch.push_back(h->batch.h_chunks[c]);
        {   // halo behind
            const Chunk &l = h->batch.h_chunks[c1 - 1];
            const int u = utt_of[c1 - 1];
            const int64_t end_row = l.out_row + l.n_frames;
            const int64_t avail = h->batch.utt_row[u] + T_of[u] - end_row;
            if (avail > 0) {
                const int hal = (int)std::min<int64_t>(D, avail);
                Chunk c;
                c.pcm_off = l.pcm_off + (int64_t)l.n_frames * h->S;
                c.out_row = end_row;
                c.n_frames = hal;
                c.pad = 0;
                fch.push_back(c);
            }
        }
        const size_t cnt = fch.size() - base;
        max_list = std::max(max_list, cnt);
        // tiles over the own chunks: runs of one utterance, <= 64 rows each
        auto local_of_row = [&](int64_t r, size_t hint) -> int32_t { // block-local chunk that holds row r
            size_t k = hint;
            while (k > 0 && fch[base + k].out_row > r) --k;
            while (k + 1 < cnt && fch[base + k].out_row + fch[base + k].n_frames <= r) ++k;
            return (int32_t)k;
        };
        size_t k = own0;
        const size_t own1 = own0 + (c1 - c0);
        while (k < own1) {
            const int u = utt_of[c0 + (k - own0)];
            const int64_t r0 = fch[base + k].out_row;
            int64_t rows = 0;
            size_t k2 = k;
            while (k2 < own1 && utt_of[c0 + (k2 - own0)] == u && rows + fch[base + k2].n_frames <= 64) {
                rows += fch[base + k2].n_frames;
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
    if (!h->fused_ok || probe.dct_mode != 1 || front512_delta_lds_bytes(probe) > kLdsCap) return MFX_OK;
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

// scratch for the compact statics of the planned batch: one buffer, two with overlap on (grown, never shrunk)
int size_static16(mfx_handle *h)
{
    const size_t need = (size_t)h->batch.total_rows * 16;
    for (int b = 0; b < (h->batch.overlap ? 2 : 1); ++b)
        if (h->l1 > 0 && h->cols <= 16 && !h->traps && h->batch.d_static16[b].n < need) HIP_TRY(h, h->batch.d_static16[b].alloc(need));
    return MFX_OK;
}

} // namespace

namespace {
// mfx_batch_plan's work, on the layout the front ends will read: the caller's, or the converted PCM's (mfx_batch_plan_rates)
int plan_batch(mfx_handle *h, int32_t n_utt, const int64_t *offsets, const int64_t *lengths, int64_t *out_rows, int64_t *total_rows);

// the converter of a rates plan goes with the plan
void drop_resampler(mfx_handle *h)
{
    h->batch.rs_on = false;
    h->batch.d_rs_pcm.release(), h->batch.d_rs_taps.release(), h->batch.d_rs_rates.release(), h->batch.d_rs_tiles.release();
}
} // namespace

extern "C" int mfx_batch_plan(mfx_handle *h, int32_t n_utt, const int64_t *offsets, const int64_t *lengths,
                              int64_t *out_rows, int64_t *total_rows)
{
    MFX_DEVICE_ENTRY(h);
    const int rc = plan_batch(h, n_utt, offsets, lengths, out_rows, total_rows);
    // (refused arguments leave the previous plan, and its converter, as they were; otherwise plan_batch has waited for the stream)
    if (rc == MFX_OK || !h->batch.planned) drop_resampler(h);
    return rc;
}

namespace {
int plan_batch(mfx_handle *h, int32_t n_utt, const int64_t *offsets, const int64_t *lengths, int64_t *out_rows, int64_t *total_rows)
{
    if (n_utt < 0 || (n_utt > 0 && (!offsets || !lengths))) return fail(h, MFX_ERR_ARG, "invalid argument");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->batch.alphas_on = false; // (a warp-factor list is tied to the plan's utterance order)
    h->batch.xf_on = false;     // (and so are a transform's utterance index and its scratch)
    h->batch.spk_on = false;    // (and a speaker list)
    h->batch.planned = false;
    h->batch.n_utt = n_utt;
    h->batch.utt_off.assign(offsets, offsets + n_utt);
    h->batch.utt_len.assign(lengths, lengths + n_utt);
    h->batch.utt_row.resize(n_utt);
    h->batch.h_chunks.clear();
    h->batch.chunk_utt.clear();
    std::vector<Segment> segs((size_t)n_utt);
    std::vector<int64_t> T_of((size_t)n_utt);
    int64_t row = 0;
    int tiles_max = 0;
    bool aligned = (h->S % 2) == 0;
    for (int u = 0; u < n_utt; ++u) {
        if (offsets[u] < 0 || lengths[u] < 0) return fail(h, MFX_ERR_ARG, "negative utterance offset/length");
        int64_t T = frame_count(lengths[u], h->W, h->S);
        if (T < 0) T = 0;
        if (T > 0x7fffffff) return fail(h, MFX_ERR_ARG, "utterance too long");
        h->batch.utt_row[u] = row;
        T_of[u] = T;
        if (out_rows) out_rows[u] = row;
        if (offsets[u] & 1) aligned = false;
        for (int64_t t0 = 0; t0 < T; t0 += kChunkFrames) {
            Chunk c;
            c.pcm_off = offsets[u] + t0 * h->S;
            c.out_row = row + t0;
            c.n_frames = (int32_t)std::min<int64_t>(kChunkFrames, T - t0);
            c.pad = 0;
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
    // The 512-point kernel deals chunks to the 16 waves of each block as they become free; with 16-frame
    // chunks a wave can sit idle for most of a chunk time (~34 us on C2) at the end of the launch.  The last two
    // chunks of every wave of the grid are therefore cut into 4-frame pieces (one kernel iteration each).
    // (k_front2048: 12 waves per CU, each 16-frame chunk is 8 iterations of ~10 us -- on C5 a wave sees only ~4 chunks in
    // all, so the last ONE per wave is cut, and a launch twice that long already qualifies)
    const int ts = h->cfg.tail_split;
    const bool f2048 = h->fast2048 && h->wplan32_ok; // (stereo, mono on aligned pairs, mono at any alignment: all three builds)
    if ((h->fast512 || (h->fast1024 && h->fused_ok) || f2048) && ts >= 0) {
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
    if (h->cfg.norm != MFX_NORM_NONE) {
        HIP_TRY(h, h->batch.d_stats.alloc((size_t)n_utt * 3 * 2 * h->cols));
        const size_t need = norm_partial_doubles(n_utt, tiles_max * 64, h->cols);
        if (need > h->d_norm_partial.n) HIP_TRY(h, h->d_norm_partial.alloc(need));
    }
    int rcf = plan_fused_delta(h, T_of);
    if (rcf != MFX_OK) return rcf;
    // (allocated here so that mfx_batch_run_device itself never allocates)
    if (h->traps) { // log mel rows between the front end and k_traps (grown, never shrunk)
        h->batch.mel_pitch = (h->nb + 3) & ~3;
        const size_t need = (size_t)row * h->batch.mel_pitch;
        if (h->batch.d_logmel.n < need) HIP_TRY(h, h->batch.d_logmel.alloc(need));
    }
    rcf = size_static16(h);
    h->batch.planned = rcf == MFX_OK;
    return rcf;
}
} // namespace

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
    std::vector<ResRate> rates(distinct.size());
    std::vector<float> taps;
    int32_t taps_floats = 0, x_floats = 8, out_elems = 2;
    for (size_t k = 0; k < distinct.size(); ++k) {
        ResRate &r = rates[k];
        r = ResRate{};
        if (distinct[k] == out_hz) continue; // (tile_out == 0 marks the copy)
        ResampleShape sh;
        static const char *const why[] = {"", "sample rates must lie in 1000 .. 768000 Hz", "zeros must be 1 .. 64 (0 = 6)",
                                          "rolloff must lie in (0, 1] (0 = 0.99)", "L = out_hz / gcd is larger than 4096",
                                          "the filter has more than 4096 taps per phase", "the tap table L x P is larger than 2^20 floats"};
        if (const int e = resample_shape(distinct[k], out_hz, zeros, rolloff, sh); e != 0) return fail(h, MFX_ERR_ARG, why[-e]);
        r.taps_off = (int64_t)taps.size();
        r.L = sh.L, r.M = sh.M, r.P = sh.P, r.Wh = sh.Wh;
        taps.resize(taps.size() + (size_t)sh.L * sh.P);
        build_resample_taps(sh, taps.data() + r.taps_off);
        resample_geometry(h->channels, r);
        if (r.in_lds) taps_floats = std::max(taps_floats, (r.L * (r.P + 1) + 3) & ~3);
        x_floats = std::max(x_floats, resample_span_floats(r));
        out_elems = std::max(out_elems, r.tile_out * h->channels);
    }
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
    ResampleParams probe{};
    probe.channels = h->channels, probe.taps_floats = taps_floats, probe.x_floats = x_floats, probe.out_elems = out_elems;
    if (resample_lds_bytes(probe) > kLdsCap) return fail(h, MFX_ERR_ARG, "no tile of k_resample fits the LDS for this shape");

    int rc = plan_batch(h, n_utt, sc_off.data(), sc_len.data(), out_rows, total_rows); // (waits for the stream)
    h->batch.rs_on = false;
    if (rc != MFX_OK) return rc;
    h->batch.planned = false;
    if (taps.empty()) taps.assign(4, 0.f); // (every utterance at the output rate: keep the buffers non-null)
    if (tiles.empty()) tiles.push_back(ResTile{});
    HIP_TRY(h, h->upload(h->batch.d_rs_taps, taps));
    HIP_TRY(h, h->upload(h->batch.d_rs_rates, rates));
    HIP_TRY(h, h->upload(h->batch.d_rs_tiles, tiles));
    // (allocated here so that mfx_batch_run_device itself never allocates; 8 elements of padding: the front ends read the
    // 32-bit word that holds the last sample)
    const size_t need = (size_t)sc_total * h->channels + 8;
    if (h->batch.d_rs_pcm.n < need) {
        HIP_TRY(h, h->batch.d_rs_pcm.alloc(need));
        HIP_TRY(h, hipMemset(h->batch.d_rs_pcm.p, 0, need * sizeof(int16_t)));
    }
    h->batch.rs_in_off.assign(offsets, offsets + n_utt);
    h->batch.rs_in_len.assign(lengths, lengths + n_utt);
    h->batch.rs_utt_tile0.swap(tile0);
    h->batch.rs_total = sc_total;
    h->batch.rs_taps_floats = taps_floats, h->batch.rs_x_floats = x_floats, h->batch.rs_out_elems = out_elems;
    h->batch.rs_on = true;
    h->batch.planned = true;
    return MFX_OK;
}

extern "C" int mfx_batch_resample_layout(const mfx_handle *h, int64_t *offsets, int64_t *lengths, int64_t *total)
{
    if (!h) return MFX_ERR_ARG;
    if (h->planning) return fail(const_cast<mfx_handle *>(h), MFX_ERR_DEVICE, "planning handle (mfx_plan_create): no device behind it");
    if (!h->batch.rs_on) return fail(const_cast<mfx_handle *>(h), MFX_ERR_STATE, "mfx_batch_resample_layout: no rates plan is in force");
    if (offsets) std::copy(h->batch.utt_off.begin(), h->batch.utt_off.end(), offsets);
    if (lengths) std::copy(h->batch.utt_len.begin(), h->batch.utt_len.end(), lengths);
    if (total) *total = h->batch.rs_total;
    return MFX_OK;
}

// rows of the spectrum slab of the batch entries' spectrum path
static constexpr int64_t kSlabRowsMax = 1 << 17;

extern "C" int mfx_batch_set_alphas(mfx_handle *h, const float *alphas, int32_t n_utt)
{
    MFX_DEVICE_ENTRY(h);
    if (!alphas && n_utt == 0) { // back to mfx_set_alpha's factor and choose_front's kernels
        h->batch.alphas_on = false;
        return MFX_OK;
    }
    if (!alphas || n_utt != h->batch.n_utt) return fail(h, MFX_ERR_ARG, "one warp factor per planned utterance");
    for (int u = 0; u < n_utt; ++u)
        if (!(alphas[u] > 0.f)) return fail(h, MFX_ERR_ARG, "alpha must be positive");
    std::vector<int64_t> frames((size_t)n_utt);
    for (int u = 0; u < n_utt; ++u) frames[u] = std::max<int64_t>(frame_count(h->batch.utt_len[u], h->W, h->S), 0);
    std::vector<float> tables;
    std::vector<int32_t> off;
    std::vector<int64_t> runs;
    build_alpha_runs(alphas, frames.data(), n_utt, tables, off, runs);
    if (tables.size() > 4096) return fail(h, MFX_ERR_ARG, "more than 4096 distinct warp factors");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = mfx_synchronize(h); // (a run in flight may read the tables and lists replaced below)
    if (rc != MFX_OK) return rc;
    h->batch.alphas_on = false;
    if (tables.empty()) return MFX_OK; // (a plan without utterances)
    rc = build_cep_tables(h, tables.data(), (int)tables.size(), h->batch.alpha_tables);
    if (rc != MFX_OK) return rc;
    if (runs.empty()) runs.assign(2, 0); // (no utterance has a frame: nothing will run; keep the buffers non-null)
    HIP_TRY(h, h->upload(h->batch.d_run_off, off));
    HIP_TRY(h, h->upload(h->batch.d_runs, runs));
    h->batch.h_run_off.swap(off);
    h->batch.h_runs.swap(runs);
    // (everything mfx_batch_run_device needs is allocated here: that entry never allocates)
    const size_t slab = (size_t)std::min<int64_t>(h->batch.total_rows, kSlabRowsMax) * h->spec_pitch;
    if (h->batch.d_spec_slab.n < slab) HIP_TRY(h, h->batch.d_spec_slab.alloc(slab));
    h->batch.alphas_on = true;
    return MFX_OK;
}

// ------------------------------------------------------------------------------------------------
// per-speaker normalisation ("Per-speaker normalisation")
// ------------------------------------------------------------------------------------------------

// normalised columns: the whole row after the deltas, else the statics
static int spk_wn(const mfx_handle *h) { return h->cfg.norm_after_dyn ? h->width : h->cols; }

extern "C" int mfx_batch_set_speakers(mfx_handle *h, const int32_t *utt_spk, int32_t n_utt, int32_t n_spk, const int64_t *prior_count,
                                      const double *prior_acc, int32_t mode)
{
    MFX_DEVICE_ENTRY(h);
    if (h->cfg.norm == MFX_NORM_NONE) return fail(h, MFX_ERR_CONFIG, "mfx_batch_set_speakers: the handle does not normalise (norm = NONE)");
    if (!utt_spk && n_utt == 0) { // back to every utterance's own statistics and run_norm's kernels
        HIP_TRY(h, hipSetDevice(h->device));
        const int rc = mfx_synchronize(h); // (a run in flight may read what a later call replaces)
        if (rc != MFX_OK) return rc;
        h->batch.spk_on = false;
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
    std::vector<int64_t> frames((size_t)n_utt);
    for (int u = 0; u < n_utt; ++u) frames[u] = std::max<int64_t>(frame_count(h->batch.utt_len[u], h->W, h->S), 0);
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
    h->batch.spk_on = false;
    h->batch.spk_ran = false;
    // (everything mfx_batch_run_device needs is allocated here: that entry never allocates)
    HIP_TRY(h, h->upload(h->batch.d_spk_off, off));
    HIP_TRY(h, h->upload(h->batch.d_spk_list, list));
    HIP_TRY(h, h->upload(h->batch.d_spk_chunk0, chunk0));
    HIP_TRY(h, h->upload(h->batch.d_spk_tiles, tiles));
    const size_t per = (size_t)4 * Wn;
    if (prior_count) {
        HIP_TRY(h, h->upload(h->batch.d_spk_prior_n, std::vector<int64_t>(prior_count, prior_count + n_spk)));
        HIP_TRY(h, h->upload(h->batch.d_spk_prior, std::vector<double>(prior_acc, prior_acc + (size_t)n_spk * per)));
    } else {
        h->batch.d_spk_prior_n.release(), h->batch.d_spk_prior.release();
    }
    HIP_TRY(h, h->batch.d_spk_partial.alloc((size_t)chunks * per));
    HIP_TRY(h, h->batch.d_spk_count.alloc((size_t)n_spk));
    HIP_TRY(h, h->batch.d_spk_acc.alloc((size_t)n_spk * per));
    HIP_TRY(h, h->batch.d_spk_stats.alloc((size_t)n_spk * 2 * Wn));
    h->batch.n_spk = n_spk;
    h->batch.spk_mode = mode;
    h->batch.spk_tiles = (int32_t)tiles.size();
    h->batch.spk_max_rows = (int32_t)max_rows;
    h->batch.spk_on = true;
    return MFX_OK;
}

extern "C" int mfx_batch_speaker_stats(mfx_handle *h, int64_t *count, double *acc, float *stats)
{
    MFX_DEVICE_ENTRY(h);
    if (!h->batch.spk_on) return fail(h, MFX_ERR_STATE, "mfx_batch_speaker_stats: no speaker list is in force");
    if (!h->batch.spk_ran) return fail(h, MFX_ERR_STATE, "mfx_batch_speaker_stats: no batch has run since the list was set");
    HIP_TRY(h, hipSetDevice(h->device));
    const int rc = mfx_synchronize(h);
    if (rc != MFX_OK) return rc;
    const size_t n = (size_t)h->batch.n_spk, Wn = (size_t)spk_wn(h);
    if (count) HIP_TRY(h, hipMemcpy(count, h->batch.d_spk_count.p, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (acc) HIP_TRY(h, hipMemcpy(acc, h->batch.d_spk_acc.p, n * 4 * Wn * sizeof(double), hipMemcpyDeviceToHost));
    if (stats) HIP_TRY(h, hipMemcpy(stats, h->batch.d_spk_stats.p, n * 2 * Wn * sizeof(float), hipMemcpyDeviceToHost));
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
    sp.mode = h->batch.spk_mode;
    sp.segs = h->batch.d_segs.p;
    sp.n_utt = h->batch.n_utt;
    sp.max_rows = h->batch.spk_max_rows;
    sp.utt_chunk0 = h->batch.d_spk_chunk0.p;
    sp.partial = h->batch.d_spk_partial.p;
    sp.spk_off = h->batch.d_spk_off.p;
    sp.spk_list = h->batch.d_spk_list.p;
    sp.n_spk = h->batch.n_spk;
    sp.prior_count = h->batch.d_spk_prior_n.p;
    sp.prior_acc = h->batch.d_spk_prior.p;
    sp.count = h->batch.d_spk_count.p;
    sp.acc = h->batch.d_spk_acc.p;
    sp.stats = h->batch.d_spk_stats.p;
    sp.tiles = h->batch.d_spk_tiles.p;
    sp.n_tiles = h->batch.spk_tiles;
    if (sp.mode == MFX_SPK_POOL) HIP_TRY(h, launch_spk_sums(sp, stream));
    HIP_TRY(h, launch_spk_finish(sp, stream));
    HIP_TRY(h, launch_spk_apply(sp, stream));
    h->batch.spk_ran = true;
    return MFX_OK;
}
} // namespace

int batch_out_width(const mfx_handle *h) { return h->batch.xf_on ? h->batch.xf_out : h->width; }

extern "C" int mfx_batch_output_width(const mfx_handle *h) { return h ? batch_out_width(h) : MFX_ERR_ARG; }

static void fill_xform(const mfx_handle *h, XformParams &p)
{
    p = XformParams{};
    p.width = h->width;
    p.left = h->batch.xf_left;
    p.right = h->batch.xf_right;
    p.out_dim = h->batch.xf_out;
    p.valu = (h->cfg.engine & MFX_ENGINE_XFORM_VALU) ? 1 : 0;
}

extern "C" int mfx_batch_set_transform(mfx_handle *h, int32_t left, int32_t right, int32_t out_dim, int32_t n_xf, const float *A,
                                       const float *b, const int32_t *utt_xf, int32_t n_utt)
{
    MFX_DEVICE_ENTRY(h);
    if (!A && n_xf == 0) { // back to the rows the handle delivered before, in the caller's d_out
        HIP_TRY(h, hipSetDevice(h->device));
        const int rc = mfx_synchronize(h); // (a run in flight may read what is released below)
        if (rc != MFX_OK) return rc;
        h->batch.xf_on = false;
        h->batch.d_xf_ops.release(), h->batch.d_xf_bias.release(), h->batch.d_xf_idx.release(), h->batch.d_xf_y.release();
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
    h->batch.xf_on = false;
    const int tiles = (out_dim + 15) / 16, steps = (int)((in_dim + 3) / 4);
    const size_t per = (size_t)steps * tiles * 64;
    std::vector<float> ops(per * n_xf), bias((size_t)n_xf * tiles * 16, 0.f);
    for (int x = 0; x < n_xf; ++x) {
        int tl = 0, st = 0;
        build_xform_operands(A + (size_t)x * out_dim * in_dim, out_dim, (int)in_dim, tl, st, ops.data() + per * x);
        if (b) std::copy(b + (size_t)x * out_dim, b + (size_t)(x + 1) * out_dim, bias.begin() + (size_t)x * tiles * 16);
    }
    HIP_TRY(h, h->upload(h->batch.d_xf_ops, ops));
    HIP_TRY(h, h->upload(h->batch.d_xf_bias, bias));
    if (utt_xf)
        HIP_TRY(h, h->upload(h->batch.d_xf_idx, std::vector<int32_t>(utt_xf, utt_xf + n_utt)));
    else
        h->batch.d_xf_idx.release();
    // (everything mfx_batch_run_device needs is allocated here: that entry never allocates)
    const size_t need = (size_t)std::max<int64_t>(h->batch.total_rows, 1) * h->width;
    if (h->batch.d_xf_y.n < need) HIP_TRY(h, h->batch.d_xf_y.alloc(need));
    h->batch.xf_left = left, h->batch.xf_right = right, h->batch.xf_out = out_dim;
    h->batch.xf_on = true;
    return MFX_OK;
}

namespace {
// utterances [u0, u1) of the planned batch (all of them: the fused-delta and overlap modes apply)
int batch_run_range(mfx_handle *h, const int16_t *d_pcm, int64_t pcm_samples_total, float *d_out, int u0, int u1);
} // namespace

extern "C" int mfx_batch_run_device(mfx_handle *h, const int16_t *d_pcm, int64_t pcm_samples_total, float *d_out)
{
    MFX_DEVICE_ENTRY(h);
    return batch_run_range(h, d_pcm, pcm_samples_total, d_out, 0, h->batch.n_utt);
}

namespace {
int batch_run_range(mfx_handle *h, const int16_t *d_pcm, int64_t pcm_samples_total, float *d_out, int u0, int u1)
{
    if (!d_pcm || !d_out || pcm_samples_total <= 0) return fail(h, MFX_ERR_ARG, "invalid argument");
    const bool whole = u0 == 0 && u1 == h->batch.n_utt;
    if (h->batch.spk_on && !whole) return fail(h, MFX_ERR_STATE, "a speaker list is in force: the batch runs as a whole");
    const int32_t rc0 = h->batch.utt_chunk0[u0], rc1 = h->batch.utt_chunk0[u1]; // chunk range of the utterance range
    if (!h->have_window) return fail(h, MFX_ERR_STATE, "set_window has not been called");
    if (h->batch.rs_on) {
        // A rates plan in force: the caller's array is converted into the handle's scratch by one launch over the tiles of
        // the utterance range, and everything below runs as it always does on the scratch and its layout.
        if (((uintptr_t)d_pcm & 3) != 0) return fail(h, MFX_ERR_ARG, "d_pcm must be 4-byte aligned");
        for (int u = u0; u < u1; ++u)
            if (h->batch.rs_in_off[u] + h->batch.rs_in_len[u] > pcm_samples_total)
                return fail(h, MFX_ERR_ARG, "utterance extends past the end of the PCM array");
        HIP_TRY(h, hipSetDevice(h->device));
        const int32_t t0 = h->batch.rs_utt_tile0[u0], t1 = h->batch.rs_utt_tile0[u1];
        ResampleParams rp{};
        rp.pcm = d_pcm;
        rp.out = h->batch.d_rs_pcm.p;
        rp.tiles = h->batch.d_rs_tiles.p + t0;
        rp.n_tiles = t1 - t0;
        rp.rates = h->batch.d_rs_rates.p;
        rp.taps = h->batch.d_rs_taps.p;
        rp.channels = h->channels;
        rp.taps_floats = h->batch.rs_taps_floats, rp.x_floats = h->batch.rs_x_floats, rp.out_elems = h->batch.rs_out_elems;
        HIP_TRY(h, launch_resample(rp, h->stream));
        d_pcm = h->batch.d_rs_pcm.p;
        pcm_samples_total = h->batch.rs_total;
    }
    if (h->batch.total_rows == 0) return MFX_OK;
    if (((uintptr_t)d_pcm & 3) != 0) return fail(h, MFX_ERR_ARG, "d_pcm must be 4-byte aligned");
    for (int u = u0; u < u1; ++u)
        if (h->batch.utt_off[u] + h->batch.utt_len[u] > pcm_samples_total)
            return fail(h, MFX_ERR_ARG, "utterance extends past the end of the PCM array");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = refresh_mel(h);
    if (rc != MFX_OK) return rc;
    if (rc1 <= rc0) return MFX_OK;
    // A transform in force: everything below runs as it always does with the handle's scratch in the place of d_out, and
    // k_splice_affine turns the scratch rows into the caller's array as the last launch.
    float *const d_final = d_out;
    if (h->batch.xf_on) {
        if (h->batch.d_xf_y.n < (size_t)h->batch.total_rows * h->width) return fail(h, MFX_ERR_STATE, "batch not planned");
        d_out = h->batch.d_xf_y.p;
    }

    FrontParams p;
    fill_front(h, p);
    p.pcm = d_pcm;
    p.pcm_total = pcm_samples_total * h->channels;
    p.chunks = h->batch.d_chunks.p + rc0;
    p.n_chunks = rc1 - rc0;
    p.row_limit = h->batch.total_rows;
    // (TRAPS: the front end's log mel rows go to the scratch; k_traps turns them into the statics of d_out)
    p.feat = h->traps ? h->batch.d_logmel.p : d_out;
    p.feat_pitch = h->traps ? h->batch.mel_pitch : h->width;
    if (h->traps && h->batch.d_logmel.n < (size_t)h->batch.total_rows * h->batch.mel_pitch)
        return fail(h, MFX_ERR_STATE, "batch not planned");

    // Which front end: the 512-point register kernel, else the fused wave-per-frame kernel when its
    // LDS fits, else spectrum through an HBM slab + melcep.
    // (per-utterance warp factors in force: always the slab)
    const FrontKind kind = batch_front(h);
    const bool fused512 = kind == kFront512, fused1024 = kind == kFront1024, fused2048 = kind == kFront2048,
               fusedgen = kind == kFrontGenFused;
    // With deltas on, the front end writes its statics as compact 64-byte rows into a scratch buffer
    // and the delta kernel emits whole [static | d | dd] rows: every HBM write is then a full line
    // (13-float row pieces at a 156-byte pitch cost 1.5x their size in 32-byte sectors).
    const bool norm_before = h->cfg.norm != MFX_NORM_NONE && !h->cfg.norm_after_dyn;
    // Overlap (opt-in, mfx_batch_overlap): the delta/normalisation tail runs on a second stream behind an
    // event, so the memory-bound tail of batch i shares the GPU with the compute-bound front end of
    // batch i+1; the statics scratch is double buffered and the front end of batch i+2 waits for tail i.
    const int sb = (h->batch.overlap && whole) ? (int)(h->batch.seq & 1) : 0;
    const bool via_scratch = ((fused512 && p.dct_mode == 1) || fused1024 || fused2048 || fusedgen) && h->l1 > 0 && h->cols <= 16 && !h->traps && !norm_before &&
                             h->batch.d_static16[sb].n >= (size_t)h->batch.total_rows * 16;
    // Fused delta stage: the 512-point kernel's last wave per block turns the statics into whole output
    // rows while the other 15 produce them; no separate delta launch.
    bool fuse = whole && h->fuse.planned && fused512 && via_scratch && ((uintptr_t)d_out & 15) == 0;
    if (fuse) {
        p.dl1 = h->l1;
        p.dl2 = h->l2;
        p.done_words = h->fuse.done_words;
        fuse = p.dct_mode == 1 && front512_delta_lds_bytes(p) <= kLdsCap;
    }
    const bool split_tail = whole && h->batch.overlap && via_scratch && !fuse;
    hipStream_t tail_stream = split_tail ? h->batch.stream2 : h->stream;
    if (via_scratch) {
        p.feat = h->batch.d_static16[sb].p;
        p.feat_pitch = 16;
    }
    if (split_tail && h->batch.tail_pending[sb]) // tail of batch i-2 still reads this scratch buffer
        HIP_TRY(h, hipStreamWaitEvent(h->stream, h->batch.ev_tail[sb], 0));
    if (fuse) {
        p.chunks = h->fuse.d_chunks.p;
        p.n_chunks = h->fuse.nchunks;
        p.blk_chunk_off = h->fuse.d_blk_chunk_off.p;
        p.blk_tile_off = h->fuse.d_blk_tile_off.p;
        p.tiles = h->fuse.d_tiles.p;
        p.out = d_out;
        p.out_pitch = h->width;
        p.n_blocks = h->fuse.blocks;
        p.err_flag = h->fuse.d_err.p;
        p.spec = h->d_spec.p; // unused by this kernel; a -DMFX_DSTAMPS dev build drops the delta wave's tick counts here
        ProfScope ps(h);
        HIP_TRY(h, launch_front512_delta(p, h->batch.aligned, h->nm16, h->stream));
    } else if (fused512) {
        p.spec = h->d_spec.p; // unused by the fused kernel; a -DMFX_STAMPS dev build drops its cycle sums here
        ProfScope ps(h);
        HIP_TRY(h, launch_front512(p, /*to_spectrum=*/false, h->batch.aligned, h->nm16, h->stream));
    } else if (fused1024) {
        ProfScope ps(h);
        HIP_TRY(h, launch_front1024(p, h->batch.aligned, h->nm16, h->stream, (h->cfg.engine & MFX_ENGINE_FRONT1024_12_WAVES) ? 12 : 16));
    } else if (fused2048) {
        p.spec = h->d_spec.p; // unused by the fused kernel; a -DMFX_STAMPS dev build drops its cycle sums here
        ProfScope ps(h);
        HIP_TRY(h, launch_front2048(p, h->num_cus, h->stream));
    } else if (fusedgen) {
        ProfScope ps(h);
        HIP_TRY(h, launch_front_generic(p, /*fused=*/true, h->stream));
    } else {
        // magnitudes go through an HBM slab, then melcep
        const int64_t slab_rows = std::min<int64_t>(h->batch.total_rows, kSlabRowsMax);
        if (h->batch.d_spec_slab.n < (size_t)slab_rows * h->spec_pitch)
            HIP_TRY(h, h->batch.d_spec_slab.alloc((size_t)slab_rows * h->spec_pitch));
        size_t c0 = (size_t)rc0;
        const size_t nchunks = (size_t)rc1;
        while (c0 < nchunks) {
            const int64_t row0 = h->batch.h_chunks[c0].out_row;
            size_t c1 = c0;
            int64_t rows = 0;
            while (c1 < nchunks && rows + h->batch.h_chunks[c1].n_frames <= slab_rows) {
                rows += h->batch.h_chunks[c1].n_frames;
                ++c1;
            }
            FrontParams q = p;
            q.chunks = h->batch.d_chunks.p + c0;
            q.n_chunks = (int32_t)(c1 - c0);
            q.spec = h->batch.d_spec_slab.p - row0 * (int64_t)h->spec_pitch; // rows are addressed absolutely
            q.spec_pitch = h->spec_pitch;
            {
                ProfScope ps(h);
                if (h->fast512)
                    HIP_TRY(h, launch_front512(q, /*to_spectrum=*/true, h->batch.aligned, h->nm16, h->stream));
                else
                    HIP_TRY(h, launch_front_generic(q, /*fused=*/false, h->stream));
            }
            if (h->batch.alphas_on) { // every table on its own rows of the slab, one launch
                RowRuns rr;
                rr.runs = h->batch.d_runs.p;
                rr.off = h->batch.d_run_off.p;
                rr.row0 = row0;
                rr.rows = rows;
                rc = launch_cepstra_runs(h, h->batch.alpha_tables, q.spec, p.feat, p.feat_pitch, rr, h->batch.h_run_off.data(),
                                         h->batch.h_runs.data(), h->stream);
            } else {
                rc = launch_cepstra(h, h->own, h->batch.d_spec_slab.p, rows, p.feat + row0 * (int64_t)p.feat_pitch, p.feat_pitch, 1, 0,
                                    nullptr, h->stream);
            }
            if (rc != MFX_OK) return rc;
            c0 = c1;
        }
    }

    if (h->traps) { // part of the front end: on the handle's stream, before anything of the tail
        TrapsParams tp;
        fill_traps(h, tp);
        tp.src = h->batch.d_logmel.p;
        tp.src_pitch = h->batch.mel_pitch;
        tp.out = d_out;
        tp.out_pitch = h->width;
        tp.segs = h->batch.d_segs.p + u0;
        tp.n_segs = u1 - u0;
        tp.tiles_per_seg_max = h->batch.tiles_max;
        HIP_TRY(h, launch_traps(tp, h->stream));
    }
    if (split_tail) {
        HIP_TRY(h, hipEventRecord(h->batch.ev_front[sb], h->stream));
        HIP_TRY(h, hipStreamWaitEvent(h->batch.stream2, h->batch.ev_front[sb], 0));
    }
    const bool norm = h->cfg.norm != MFX_NORM_NONE;
    const bool spk = norm && h->batch.spk_on; // (speakers in force: the run covers the whole batch, mfx_batch_run_host does not slice)
    if (norm && !h->cfg.norm_after_dyn) {
        rc = spk ? run_speaker_norm(h, tail_stream, d_out)
                 : run_norm(h, tail_stream, d_out, h->width, h->batch.d_segs.p + u0, u1 - u0, nullptr,
                            h->batch.d_stats.p + (size_t)u0 * 2 * h->cols, false, h->batch.tiles_max * 64);
        if (rc != MFX_OK) return rc;
    }
    if (h->l1 > 0 && !fuse) {
        DeltaParams dp{};
        dp.src = via_scratch ? h->batch.d_static16[sb].p : d_out;
        dp.src_pitch = via_scratch ? 16 : h->width;
        dp.out = d_out;
        dp.out_pitch = h->width;
        dp.segs = h->batch.d_segs.p + u0;
        dp.n_segs = u1 - u0;
        dp.cols = h->cols;
        dp.l1 = h->l1;
        dp.l2 = h->l2;
        dp.tiles_per_seg_max = h->batch.tiles_max;
        HIP_TRY(h, launch_delta(dp, tail_stream));
    }
    if (norm && h->cfg.norm_after_dyn) {
        const int groups = h->width / h->cols;
        rc = spk ? run_speaker_norm(h, tail_stream, d_out)
                 : run_norm(h, tail_stream, d_out, h->width, h->batch.d_segs.p + u0, u1 - u0, nullptr,
                            h->batch.d_stats.p + (size_t)u0 * 2 * h->cols, false, h->batch.tiles_max * 64, groups,
                            (size_t)h->batch.n_utt * 2 * h->cols);
        if (rc != MFX_OK) return rc;
    }
    if (h->batch.xf_on) { // behind the tail, on its stream: ev_tail covers it
        XformParams xp;
        fill_xform(h, xp);
        xp.src = d_out;
        xp.src_pitch = h->width;
        xp.out = d_final;
        xp.out_pitch = h->batch.xf_out;
        xp.segs = h->batch.d_segs.p + u0;
        xp.n_segs = u1 - u0;
        xp.seg_xf = h->batch.d_xf_idx.p ? h->batch.d_xf_idx.p + u0 : nullptr;
        xp.operands = h->batch.d_xf_ops.p;
        xp.bias = h->batch.d_xf_bias.p;
        xp.tiles_per_seg_max = h->batch.tiles_max;
        HIP_TRY(h, launch_xform(xp, tail_stream));
    }
    if (split_tail) {
        HIP_TRY(h, hipEventRecord(h->batch.ev_tail[sb], tail_stream));
        h->batch.tail_pending[sb] = true;
    }
    if (whole) ++h->batch.seq;
    return MFX_OK;
}
} // namespace

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
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = mfx_synchronize(h);
    if (rc != MFX_OK) return rc;
    if (enable && !h->batch.stream2) {
        HIP_TRY(h, hipStreamCreateWithFlags(&h->batch.stream2, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            HIP_TRY(h, hipEventCreateWithFlags(&h->batch.ev_front[i], hipEventDisableTiming));
            HIP_TRY(h, hipEventCreateWithFlags(&h->batch.ev_tail[i], hipEventDisableTiming));
        }
    }
    h->batch.overlap = enable != 0;
    h->batch.tail_pending[0] = h->batch.tail_pending[1] = false;
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
    const size_t n_out = (size_t)std::max<int64_t>(h->batch.total_rows, 1) * ow;
    if (h->batch.d_host_pcm.n < n_in + 8) HIP_TRY(h, h->batch.d_host_pcm.alloc(n_in + 8));
    if (h->batch.d_host_out.n < n_out) HIP_TRY(h, h->batch.d_host_out.alloc(n_out));

    // Pinned caller buffers and a batch worth slicing: the utterances go through in up to 8 slices, the upload of slice
    // k + 1 and the download of slice k - 1 running beside the kernels of slice k on their own streams (PCIe is full
    // duplex: the 320 MB in and the 156 MB out of a C2 batch overlap instead of queueing up).  Utterance offsets must
    // ascend for a slice to be one contiguous piece of the PCM array; anything else takes the plain path below.
    // (a rates plan in force: the caller's array is cut by its own layout, in input-rate samples)
    const std::vector<int64_t> &in_off = h->batch.rs_on ? h->batch.rs_in_off : h->batch.utt_off;
    const std::vector<int64_t> &in_len = h->batch.rs_on ? h->batch.rs_in_len : h->batch.utt_len;
    bool ascending = true;
    for (int u = 1; u < h->batch.n_utt && ascending; ++u) ascending = in_off[u] >= in_off[u - 1] + in_len[u - 1];
    const int K = (int)std::min<int64_t>(8, h->batch.n_utt / 4);
    // (a speaker list in force: a speaker may span slices, the batch goes through whole)
    if (K >= 2 && ascending && !h->batch.overlap && !h->fuse.planned && !h->batch.spk_on && n_in * sizeof(int16_t) >= ((size_t)32 << 20) &&
        is_pinned_host(pcm) && is_pinned_host(out)) {
        if (!h->batch.stream_up) {
            HIP_TRY(h, hipStreamCreateWithFlags(&h->batch.stream_up, hipStreamNonBlocking));
            HIP_TRY(h, hipStreamCreateWithFlags(&h->batch.stream_dn, hipStreamNonBlocking));
            for (int i = 0; i < 16; ++i) {
                HIP_TRY(h, hipEventCreateWithFlags(&h->batch.ev_up[i], hipEventDisableTiming));
                HIP_TRY(h, hipEventCreateWithFlags(&h->batch.ev_run[i], hipEventDisableTiming));
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
                HIP_TRY(h, hipMemcpyAsync(h->batch.d_host_pcm.p + s0 * ch, pcm + s0 * ch, (size_t)(s1 - s0) * ch * sizeof(int16_t),
                                          hipMemcpyHostToDevice, h->batch.stream_up));
            HIP_TRY(h, hipEventRecord(h->batch.ev_up[k], h->batch.stream_up));
            HIP_TRY(h, hipStreamWaitEvent(h->stream, h->batch.ev_up[k], 0));
            int rc = batch_run_range(h, h->batch.d_host_pcm.p, pcm_samples_total, h->batch.d_host_out.p, u0, u1);
            if (rc != MFX_OK) return rc;
            HIP_TRY(h, hipEventRecord(h->batch.ev_run[k], h->stream));
            HIP_TRY(h, hipStreamWaitEvent(h->batch.stream_dn, h->batch.ev_run[k], 0));
            const int64_t r0 = h->batch.utt_row[u0], r1 = u1 < h->batch.n_utt ? h->batch.utt_row[u1] : h->batch.total_rows;
            if (r1 > r0)
                HIP_TRY(h, hipMemcpyAsync(out + r0 * ow, h->batch.d_host_out.p + r0 * ow, (size_t)(r1 - r0) * ow * sizeof(float),
                                          hipMemcpyDeviceToHost, h->batch.stream_dn));
            return MFX_OK;
        };
        for (int k = 0; k < K; ++k) {
            const int rc = run_slice(k);
            if (rc != MFX_OK) { // nothing may still read `pcm` or write `out` once we have returned
                (void)hipStreamSynchronize(h->batch.stream_up);
                (void)hipStreamSynchronize(h->stream);
                (void)hipStreamSynchronize(h->batch.stream_dn);
                return rc;
            }
        }
        HIP_TRY(h, hipStreamSynchronize(h->batch.stream_dn));
        return mfx_synchronize(h);
    }

    HIP_TRY(h, hipMemcpyAsync(h->batch.d_host_pcm.p, pcm, n_in * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
    int rc = mfx_batch_run_device(h, h->batch.d_host_pcm.p, pcm_samples_total, h->batch.d_host_out.p);
    if (rc != MFX_OK) {
        (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    if (h->batch.stream2) HIP_TRY(h, hipStreamSynchronize(h->batch.stream2)); // overlapped tail, if any
    if (h->batch.total_rows > 0)
        HIP_TRY(h, hipMemcpyAsync(out, h->batch.d_host_out.p, (size_t)h->batch.total_rows * ow * sizeof(float), hipMemcpyDeviceToHost,
                                  h->stream));
    return mfx_synchronize(h);
}
