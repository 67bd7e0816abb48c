// mfx_sessions_host.cpp -- the session entries of include/mfx.h: many open streams, each advanced by one chunk of samples per
// push, all of them in one launch sequence (k_sess_gather -> front end -> delta, with k_onorm_sess before or after the delta
// while the online normaliser is set, and k_sess_xform as the last launch while a session transform is set).  DESIGN.md
// section 5, "Session entries" and "Session transform".
// This file owns the handle's `sess` part.  It reads the shared geometry and tables and names no field of `st`, `sweep`,
// `batch` or `fuse`: a push leaves the streaming state and the batch plan, alpha list and transform as they are.
#include "mfx_handle.h"

#include <cstdint>
#include <cstring>
#include <numeric>

using namespace mfx;

namespace {

int not_created(mfx_handle *h) { return fail(h, MFX_ERR_STATE, "mfx_sessions_create has not been called"); }

// the slot arrays' frames lie on even samples exactly when the shift is even: slot bases and pcm_stride are even
bool sess_aligned(const mfx_handle *h) { return (h->S % 2) == 0; }

bool norm_before(const mfx_handle *h) { return h->cfg.norm != MFX_NORM_NONE && !h->cfg.norm_after_dyn; }

} // namespace

extern "C" int mfx_sessions_create(mfx_handle *h, int32_t n_sessions, int32_t max_push_samples)
{
    MFX_DEVICE_ENTRY(h);
    if (h->traps)
        return fail(h, MFX_ERR_STATE, "the session entries do not serve TRAPS handles (their look-ahead is (L - 1) / 2 frames, not D)");
    if (h->stft)
        return fail(h, MFX_ERR_STATE, "the session entries do not serve STFT log-mel handles: use the batch entries (mfx_batch_plan + mfx_batch_run_device)");
    if (h->cfg.norm != MFX_NORM_NONE && !h->sess.on.set) // (mfx_sessions_set_online_norm: the one normaliser served)
        return fail(h, MFX_ERR_STATE,
                    "the session entries do not serve normalisation (norm != MFX_NORM_NONE): statistics over an open stream are not built");
    if (n_sessions < 0 || max_push_samples < 0 || (n_sessions == 0) != (max_push_samples == 0))
        return fail(h, MFX_ERR_ARG, "n_sessions and max_push_samples must both be positive (or both 0: release)");
    if (n_sessions > (1 << 20) || max_push_samples > (1 << 24)) return fail(h, MFX_ERR_ARG, "n_sessions or max_push_samples too large");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    SessState &ss = h->sess;
    ss.n = 0;
    ss.planned = false;
    ss.live.clear();
    ss.stage_used[0] = ss.stage_used[1] = false;
    if (n_sessions == 0) {
        ss.d_pcm.release(), ss.d_stat.release(), ss.d_slab.release(), ss.d_desc.release();
        ss.d_host_pcm.release(), ss.d_host_out.release();
        ss.on.d_prior.release(), ss.on.d_state.release(), ss.on.d_ring.release();
        ss.xf.d_ops.release(), ss.xf.d_bias.release(), ss.xf.d_y.release();
        for (auto &b : ss.h_stage) {
            if (b.p) (void)hipHostFree(b.p);
            b.p = nullptr, b.n = 0;
        }
        ss.max_push = 0;
        return MFX_OK;
    }
    int rc = refresh_mel(h); // (decides which front end the shape takes, and with it whether a spectrum slab is needed)
    if (rc != MFX_OK) return rc;
    const int ch = h->channels;
    ss.max_push = max_push_samples;
    ss.pcm_stride = ((int64_t)h->W + h->S + max_push_samples + 2 + 7) & ~(int64_t)7;
    ss.frames_max = max_push_samples / h->S + 1;
    ss.row_cap = 2 * h->D + ss.frames_max;
    ss.row_floats = (std::max(16, h->width) + 3) & ~3;
    const size_t pcm_elems = (size_t)2 * n_sessions * ss.pcm_stride * ch;
    HIP_TRY(h, ss.d_pcm.alloc(pcm_elems + 8));
    HIP_TRY(h, hipMemsetAsync(ss.d_pcm.p, 0, (pcm_elems + 8) * sizeof(int16_t), h->stream));
    HIP_TRY(h, ss.d_stat.alloc((size_t)2 * n_sessions * ss.row_cap * ss.row_floats));
    ss.slab_rows = 0;
    ss.d_slab.release();
    if (is_spec_kind(choose_front(h, sess_aligned(h)))) {
        ss.slab_rows = std::min<int64_t>((int64_t)2 * n_sessions * ss.row_cap, kSlabRowsMax);
        HIP_TRY(h, ss.d_slab.alloc((size_t)ss.slab_rows * h->spec_pitch));
    }
    const size_t chunks_max = (size_t)n_sessions * ((ss.frames_max + kChunkFrames - 1) / kChunkFrames);
    ss.desc_bytes = (size_t)n_sessions * (sizeof(SessDesc) + sizeof(Segment) + 2 * sizeof(int64_t) + sizeof(OnormSessDesc)) +
                    chunks_max * sizeof(Chunk) + 64;
    ss.xf.d_y.release();
    if (ss.xf.set) { // the session transform: the two y slot arrays, the operands; descriptors of either launch form
        ss.xf.y_cap = ss.xf.left + ss.xf.right + ss.frames_max + h->D;
        HIP_TRY(h, ss.xf.d_y.alloc((size_t)2 * n_sessions * ss.xf.y_cap * h->width));
        HIP_TRY(h, h->upload(ss.xf.d_ops, ss.xf.ops));
        HIP_TRY(h, h->upload(ss.xf.d_bias, ss.xf.bias));
        const size_t groups_max = (size_t)n_sessions * ((ss.frames_max + h->D + ss.xf.right) / 16 + 1);
        ss.desc_bytes += groups_max * (sizeof(SessXfGroup) + sizeof(SessXfBlock)) + (size_t)n_sessions * (sizeof(Segment) + sizeof(int64_t));
        ss.p_xsteps.reserve(n_sessions), ss.p_groups.reserve(groups_max), ss.p_blocks.reserve(groups_max);
    }
    if (h->cfg.norm != MFX_NORM_NONE) { // the online normaliser's state: 8 doubles per session and column, the ring of raw rows
        const size_t Wn = (size_t)spk_wn(h);
        HIP_TRY(h, ss.on.d_state.alloc((size_t)n_sessions * 8 * Wn));
        HIP_TRY(h, ss.on.d_ring.alloc((size_t)n_sessions * ss.on.window * Wn));
        HIP_TRY(h, h->upload(ss.on.d_prior, ss.on.prior));
        ss.p_onorm.reserve(n_sessions);
    }
    HIP_TRY(h, ss.d_desc.alloc(ss.desc_bytes));
    for (int b = 0; b < 2; ++b) {
        HIP_TRY(h, ss.h_stage[b].grow(ss.desc_bytes, ss.desc_bytes, h->stream));
        if (!ss.ev_stage[b]) HIP_TRY(h, hipEventCreateWithFlags(&ss.ev_stage[b], hipEventDisableTiming));
    }
    ss.live.assign((size_t)n_sessions, SessState::Live{});
    ss.p_seen.assign((size_t)n_sessions, 0);
    ss.p_ids.reserve(n_sessions), ss.p_end.reserve(n_sessions), ss.p_next.reserve(n_sessions), ss.p_order.reserve(n_sessions);
    ss.p_descs.reserve(n_sessions), ss.p_segs.reserve(n_sessions), ss.p_runs.reserve((size_t)2 * n_sessions);
    ss.p_chunks.reserve(chunks_max);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    ss.n = n_sessions;
    return MFX_OK;
}

extern "C" int mfx_sessions_set_online_norm(mfx_handle *h, int32_t window, int32_t prior_frames, int64_t prior_count, const double *prior_acc)
{
    MFX_DEVICE_ENTRY(h);
    int rc = check_online_norm(h, "mfx_sessions_set_online_norm", window, prior_frames, prior_count, prior_acc);
    if (rc == MFX_ERR_CONFIG) return rc;
    if (h->sess.n != 0) return fail(h, MFX_ERR_STATE, "mfx_sessions_set_online_norm: sessions exist (mfx_sessions_create(0, 0) first)");
    if (rc != MFX_OK) return rc;
    SessState::Onorm &on = h->sess.on;
    on.window = window, on.prior_frames = prior_frames, on.prior_count = prior_count;
    on.prior.clear();
    if (prior_count > 0) on.prior.assign(prior_acc, prior_acc + (size_t)2 * spk_wn(h));
    on.set = true;
    return MFX_OK;
}

extern "C" int mfx_sessions_clear_online_norm(mfx_handle *h)
{
    MFX_DEVICE_ENTRY(h);
    if (h->sess.n != 0) return fail(h, MFX_ERR_STATE, "mfx_sessions_clear_online_norm: sessions exist (mfx_sessions_create(0, 0) first)");
    h->sess.on.set = false;
    h->sess.on.prior.clear();
    return MFX_OK;
}

// the kernel parameters of the session transform at this handle's row width (pointers and work list left out)
static void fill_sess_xform(const mfx_handle *h, int left, int right, int out_dim, SessXformParams &q, XformParams &plain)
{
    q = SessXformParams{};
    q.width = h->width, q.left = left, q.right = right, q.out_dim = out_dim;
    q.src_pitch = h->width, q.out_pitch = out_dim;
    q.valu = (h->cfg.engine & MFX_ENGINE_XFORM_VALU) ? 1 : 0;
    plain = XformParams{};
    plain.width = h->width, plain.left = left, plain.right = right, plain.out_dim = out_dim;
    plain.src_pitch = h->width, plain.out_pitch = out_dim;
    plain.valu = q.valu;
}

extern "C" int mfx_sessions_set_transform(mfx_handle *h, int32_t left, int32_t right, int32_t out_dim, int32_t n_xf, const float *A,
                                          const float *b)
{
    MFX_DEVICE_ENTRY(h);
    if (h->sess.n != 0) return fail(h, MFX_ERR_STATE, "mfx_sessions_set_transform: sessions exist (mfx_sessions_create(0, 0) first)");
    if (!A) return fail(h, MFX_ERR_ARG, "no matrix");
    if (left < 0 || left > 32 || right < 0 || right > 32) return fail(h, MFX_ERR_ARG, "left and right must be 0 .. 32");
    if (out_dim < 1 || out_dim > 256) return fail(h, MFX_ERR_ARG, "out_dim must be 1 .. 256");
    if (n_xf < 1 || n_xf > 1024) return fail(h, MFX_ERR_ARG, "n_xf must be 1 .. 1024");
    const int64_t in_dim = (int64_t)(left + right + 1) * h->width;
    if (in_dim > 8192) return fail(h, MFX_ERR_ARG, "in_dim = (left + right + 1) * width is larger than 8192");
    SessXformParams probe;
    XformParams plain;
    fill_sess_xform(h, left, right, out_dim, probe, plain);
    // (the limits above leave one row group inside 160 KB at every row width a handle can have; checked all the same, with the
    // launchers' own rule)
    const int R = sess_xform_tile_rows(probe);
    if (R == 0 || xform_tile_rows(plain) == 0) return fail(h, MFX_ERR_CONFIG, "no block tiling of the session transform fits the LDS for this shape");
    SessState::Xform &xf = h->sess.xf;
    const int tiles = (out_dim + 15) / 16, steps = (int)((in_dim + 3) / 4);
    const size_t per = (size_t)steps * tiles * 64;
    xf.ops.assign(per * n_xf, 0.f), xf.bias.assign((size_t)n_xf * tiles * 16, 0.f);
    for (int x = 0; x < n_xf; ++x) {
        int tl = 0, st = 0;
        build_xform_operands(A + (size_t)x * out_dim * in_dim, out_dim, (int)in_dim, tl, st, xf.ops.data() + per * x);
        if (b) std::copy(b + (size_t)x * out_dim, b + (size_t)(x + 1) * out_dim, xf.bias.begin() + (size_t)x * tiles * 16);
    }
    xf.left = left, xf.right = right, xf.out = out_dim, xf.n_xf = n_xf, xf.G = R / 16;
    xf.set = true;
    return MFX_OK;
}

extern "C" int mfx_sessions_clear_transform(mfx_handle *h)
{
    MFX_DEVICE_ENTRY(h);
    if (h->sess.n != 0) return fail(h, MFX_ERR_STATE, "mfx_sessions_clear_transform: sessions exist (mfx_sessions_create(0, 0) first)");
    SessState::Xform &xf = h->sess.xf;
    xf.set = false;
    xf.ops.clear(), xf.bias.clear();
    xf.n_xf = 0;
    return MFX_OK;
}

extern "C" int mfx_sessions_select_transform(mfx_handle *h, int32_t session, int32_t xf)
{
    MFX_DEVICE_ENTRY(h);
    SessState &ss = h->sess;
    if (!ss.xf.set) return fail(h, MFX_ERR_STATE, "mfx_sessions_select_transform: no session transform is set");
    if (ss.n == 0) return not_created(h);
    if (session < 0 || session >= ss.n) return fail(h, MFX_ERR_ARG, "session id outside [0, n_sessions)");
    if (xf < 0 || xf >= ss.xf.n_xf) return fail(h, MFX_ERR_ARG, "transform index outside [0, n_xf)");
    if (ss.live[session].n != 0)
        return fail(h, MFX_ERR_STATE, "mfx_sessions_select_transform: the session has received samples since its last final push or reset");
    ss.live[session].xf = xf;
    ss.planned = false; // (a pending push was planned with the earlier choice)
    return MFX_OK;
}

extern "C" int mfx_sessions_output_width(const mfx_handle *h)
{
    if (!h) return MFX_ERR_ARG;
    if (h->planning) return MFX_ERR_DEVICE; // (a planning handle has no session entries)
    return sess_out_width(h);
}

extern "C" int mfx_sessions_reset(mfx_handle *h, int32_t session)
{
    MFX_DEVICE_ENTRY(h);
    SessState &ss = h->sess;
    if (ss.n == 0) return not_created(h);
    if (session < -1 || session >= ss.n) return fail(h, MFX_ERR_ARG, "session id outside [0, n_sessions)");
    // (the slots themselves need no clearing: a fresh session carries nothing out of them)
    for (int s = session < 0 ? 0 : session; s < (session < 0 ? ss.n : session + 1); ++s) {
        const int parity = ss.live[s].parity, xf = ss.live[s].xf;
        ss.live[s] = SessState::Live{}; // (the carried samples, static rows and rows y go with it)
        ss.live[s].parity = parity, ss.live[s].xf = xf;
    }
    ss.planned = false; // (a pending push was planned on the state just dropped)
    return MFX_OK;
}

extern "C" int64_t mfx_sessions_delivered(const mfx_handle *h, int32_t session)
{
    if (!h) return MFX_ERR_ARG;
    if (h->sess.n == 0) return MFX_ERR_STATE;
    if (session < 0 || session >= h->sess.n) return MFX_ERR_ARG;
    return h->sess.xf.set ? h->sess.live[session].Ex : h->sess.live[session].E;
}

extern "C" int mfx_sessions_plan(mfx_handle *h, int32_t n, const int32_t *ids, const int64_t *offsets, const int64_t *lengths,
                                 const int32_t *final_flags, int64_t *out_rows, int32_t *out_counts, int64_t *total_rows)
{
    MFX_DEVICE_ENTRY(h);
    SessState &ss = h->sess;
    if (ss.n == 0) return not_created(h);
    if (n < 0 || (n > 0 && (!ids || !offsets || !lengths))) return fail(h, MFX_ERR_ARG, "invalid argument");
    if (n > ss.n) return fail(h, MFX_ERR_ARG, "more pieces than sessions: an id is given twice or lies outside the range");
    ss.planned = false;
    // ---- checks first: nothing below them fails
    int bad = MFX_OK;
    const char *why = "";
    int marked = 0;
    for (; marked < n && bad == MFX_OK; ++marked) {
        const int32_t id = ids[marked];
        if (id < 0 || id >= ss.n) {
            bad = MFX_ERR_ARG, why = "session id outside [0, n_sessions)";
            break;
        }
        if (ss.p_seen[id]) {
            bad = MFX_ERR_ARG, why = "session id given twice in one push";
            break;
        }
        ss.p_seen[id] = 1;
        if (offsets[marked] < 0 || lengths[marked] < 0)
            bad = MFX_ERR_ARG, why = "negative offset or length";
        else if (offsets[marked] > INT64_MAX / 4 - lengths[marked]) // (the end, times the channels, stays inside int64)
            bad = MFX_ERR_ARG, why = "offset + length too large";
        else if (lengths[marked] > ss.max_push)
            bad = MFX_ERR_BUFFER_TOO_SMALL, why = "a session's piece is longer than max_push_samples (mfx_sessions_create)";
        else if (frame_count(ss.live[id].n + lengths[marked], h->W, h->S) > 0x7fffffff)
            bad = MFX_ERR_ARG, why = "stream too long";
    }
    for (int i = 0; i < n && i <= marked; ++i)
        if (ids[i] >= 0 && ids[i] < ss.n) ss.p_seen[ids[i]] = 0;
    if (bad != MFX_OK) return fail(h, bad, why);

    // ---- pass 1, the caller's order: every session's step, the output rows
    const int ch = h->channels, D = h->D;
    ss.p_ids.assign(ids, ids + n);
    ss.p_end.resize(n), ss.p_next.resize(n), ss.p_order.resize(n), ss.p_row_of.resize(n);
    std::vector<SessionStep> &steps = ss.p_steps;
    steps.resize(n);
    const bool xform = ss.xf.set;
    if (xform) ss.p_xsteps.resize(n), ss.p_xn.assign(n, 0), ss.p_xxf.assign(n, 0), ss.p_xsrc.assign(n, 0);
    int64_t row = 0;
    for (int i = 0; i < n; ++i) {
        SessState::Live nx = ss.live[ids[i]];
        const bool fin = final_flags && final_flags[i] != 0;
        (void)session_step(h->W, h->S, D, nx.n, nx.E, lengths[i], fin, steps[i]);
        ss.p_end[i] = lengths[i] > 0 ? offsets[i] + lengths[i] : 0;
        int32_t n_del = steps[i].n_out;
        if (xform) { // the rows y the push completes are the transform's input; it delivers rows [Ex_old, Ex_new)
            int64_t Ey = ss.live[ids[i]].E;
            n_del = session_xform_step(ss.xf.left, ss.xf.right, Ey, nx.Ex, steps[i].n_out, fin, ss.p_xsteps[i]);
        }
        ss.p_next[i] = nx; // (n, E and Ex advanced; the slot fields follow in pass 2)
        ss.p_row_of[i] = row;
        if (out_rows) out_rows[i] = row;
        if (out_counts) out_counts[i] = n_del;
        row += n_del;
    }
    ss.p_total_rows = row;
    if (total_rows) *total_rows = row;

    // ---- pass 2, ascending slots (the slab path walks the chunk list in windows of rows): descriptors, chunks, segments
    for (int i = 0; i < n; ++i) ss.p_order[i] = i;
    auto slot_of = [&](int i) { return (int64_t)(ss.live[ids[i]].parity ^ 1) * ss.n + ids[i]; };
    std::sort(ss.p_order.begin(), ss.p_order.end(), [&](int a, int b) { return slot_of(a) < slot_of(b); });
    ss.p_descs.clear(), ss.p_segs.clear(), ss.p_chunks.clear(), ss.p_runs.clear(), ss.p_onorm.clear();
    const bool onorm = h->cfg.norm != MFX_NORM_NONE, before = norm_before(h);
    ss.p_tiles_max = 0;
    for (int k = 0; k < n; ++k) {
        const int i = ss.p_order[k];
        const SessionStep &st = steps[i];
        const SessState::Live &cur = ss.live[ids[i]];
        SessState::Live &nx = ss.p_next[i];
        const bool fin = final_flags && final_flags[i] != 0;
        // nothing to move, compute or deliver: an empty push of an open stream, the flush of a stream without samples
        if (lengths[i] == 0 && (!fin || cur.n == 0)) continue;
        const int64_t f0 = std::max<int64_t>(cur.E - D, 0);
        const int64_t slot_prev = (int64_t)cur.parity * ss.n + ids[i], slot_cur = slot_of(i);
        SessDesc d{};
        d.carry_src = (slot_prev * ss.pcm_stride + cur.tail_off) * ch;
        d.pcm_dst = slot_cur * ss.pcm_stride * ch;
        d.new_src = offsets[i] * ch;
        d.carry_n = (int32_t)(st.carry_samples * ch);
        d.new_n = (int32_t)(lengths[i] * ch);
        d.row_src = slot_prev * ss.row_cap + (f0 - cur.f0);
        d.row_dst = slot_cur * ss.row_cap;
        d.n_rows = st.carry_rows;
        d.src_pitch = cur.pitch; // (0: nothing carried yet; the run fills in its own pitch)
        int64_t y_new0 = 0; // (session transform: the row of the current y slot the push's first new row y goes to)
        if (xform) {
            const SessionXformStep &xs = ss.p_xsteps[i];
            const int64_t c0 = std::max<int64_t>(cur.Ex - ss.xf.left, 0);
            d.y_src = slot_prev * ss.xf.y_cap + (c0 - cur.y0);
            d.y_dst = slot_cur * ss.xf.y_cap;
            d.y_rows = xs.carry_rows;
            y_new0 = d.y_dst + xs.carry_rows;
            nx.y0 = fin ? 0 : c0;
            ss.p_xn[i] = xs.n_out, ss.p_xxf[i] = cur.xf, ss.p_xsrc[i] = d.y_dst + xs.src_row0;
        }
        ss.p_descs.push_back(d);
        const int64_t new_row0 = d.row_dst + st.carry_rows;
        for (int t0 = 0; t0 < st.new_frames; t0 += kChunkFrames) {
            Chunk c;
            c.pcm_off = slot_cur * ss.pcm_stride + (int64_t)t0 * h->S; // (the carried tail starts at the slot's base)
            c.out_row = new_row0 + t0;
            c.n_frames = std::min(kChunkFrames, st.new_frames - t0);
            c.pad = 0;
            ss.p_chunks.push_back(c);
        }
        if (st.new_frames > 0) ss.p_runs.push_back(new_row0), ss.p_runs.push_back(st.new_frames);
        // the online normaliser's rows: the new frames' statics in the slot (frames T_old ..) ahead of the deltas, or the
        // rows the push delivers (rows E_old ..) behind them; a fresh session has 0 rows in front and reads no state
        if (onorm && before && st.new_frames > 0)
            ss.p_onorm.push_back(OnormSessDesc{new_row0, std::max<int64_t>(frame_count(cur.n, h->W, h->S), 0), st.new_frames, ids[i]});
        if (onorm && !before && st.n_out > 0) ss.p_onorm.push_back(OnormSessDesc{xform ? y_new0 : ss.p_row_of[i], cur.E, st.n_out, ids[i]});
        if (st.n_out > 0) {
            Segment s{};
            s.src_row0 = d.row_dst;
            s.out_row0 = xform ? y_new0 : ss.p_row_of[i];
            s.n_out = st.n_out;
            s.shift = st.shift;
            s.lo = st.lo;
            s.hi = st.hi;
            s.static_off = st.static_off;
            ss.p_segs.push_back(s);
            ss.p_tiles_max = std::max(ss.p_tiles_max, (st.n_out + 63) / 64);
        }
        nx.parity = cur.parity ^ 1;
        nx.f0 = fin ? 0 : f0;
        nx.tail_off = fin ? 0 : st.new_frames * h->S;
        nx.pitch = fin ? 0 : -1; // (-1: the pitch of the run that writes the slot)
    }
    // ---- the transform's work list: row groups packed into blocks of one transform, or one segment per delivering piece
    ss.p_groups.clear(), ss.p_blocks.clear(), ss.p_xsegs.clear(), ss.p_xseg_xf.clear();
    ss.p_xtiles_max = 0;
    if (xform && (h->cfg.engine & MFX_ENGINE_SESS_XFORM_PLAIN)) {
        for (int i = 0; i < n; ++i) {
            const SessionXformStep &xs = ss.p_xsteps[i];
            if (ss.p_xn[i] <= 0) continue;
            Segment s{};
            s.src_row0 = ss.p_xsrc[i], s.out_row0 = ss.p_row_of[i], s.n_out = xs.n_out, s.lo = xs.lo, s.hi = xs.hi;
            ss.p_xsegs.push_back(s), ss.p_xseg_xf.push_back(ss.p_xxf[i]);
            ss.p_xtiles_max = std::max(ss.p_xtiles_max, (xs.n_out + 63) / 64);
        }
    } else if (xform) {
        pack_sess_xform_groups(ss.p_xn.data(), ss.p_xxf.data(), n, ss.xf.G, ss.p_xorder, ss.p_gpiece, ss.p_gr0, ss.p_grows, ss.p_bg0, ss.p_bng, ss.p_bxf);
        for (size_t g = 0; g < ss.p_gpiece.size(); ++g) {
            const int i = ss.p_gpiece[g];
            const SessionXformStep &xs = ss.p_xsteps[i];
            ss.p_groups.push_back(SessXfGroup{ss.p_xsrc[i], ss.p_row_of[i] + ss.p_gr0[g], ss.p_gr0[g], ss.p_grows[g], xs.lo, xs.hi});
        }
        for (size_t k = 0; k < ss.p_bg0.size(); ++k) ss.p_blocks.push_back(SessXfBlock{ss.p_bg0[k], ss.p_bng[k], ss.p_bxf[k], 0});
    }
    ss.planned = true;
    return MFX_OK;
}

extern "C" int mfx_sessions_run_device(mfx_handle *h, const int16_t *d_pcm, int64_t pcm_samples_total, float *d_out)
{
    MFX_DEVICE_ENTRY(h);
    SessState &ss = h->sess;
    if (ss.n == 0) return not_created(h);
    if (!ss.planned) return fail(h, MFX_ERR_STATE, "mfx_sessions_run: no push is planned (mfx_sessions_plan), or it has run already");
    if (!h->have_window) return fail(h, MFX_ERR_STATE, "set_window has not been called");
    const int n = (int)ss.p_ids.size();
    bool any_new = false;
    for (const SessDesc &d : ss.p_descs) any_new = any_new || d.new_n > 0;
    if (pcm_samples_total < 0 || (any_new && !d_pcm) || (ss.p_total_rows > 0 && !d_out)) return fail(h, MFX_ERR_ARG, "invalid argument");
    if (((uintptr_t)d_pcm & 3) != 0) return fail(h, MFX_ERR_ARG, "d_pcm must be 4-byte aligned");
    for (int i = 0; i < n; ++i)
        if (ss.p_end[i] > pcm_samples_total) return fail(h, MFX_ERR_ARG, "a session's piece extends past the end of the PCM array");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = refresh_mel(h);
    if (rc != MFX_OK) return rc;

    // the front end of the shape, as the batch entries choose it, and the pitch batch_run_range gives the statics
    const bool aligned = sess_aligned(h);
    const FrontKind kind = choose_front(h, aligned);
    FrontParams p;
    fill_front(h, p, aligned);
    // (a normaliser before the deltas: the statics keep the row's pitch, as decide_mode of the batch runner has it)
    const bool compact = compact_statics(kind, p) && h->l1 > 0 && h->cols <= 16 && !norm_before(h);
    const int pitch = compact ? 16 : h->width;
    if (is_spec_kind(kind) && ss.slab_rows == 0)
        return fail(h, MFX_ERR_STATE, "the warp factor moved this shape to the spectrum path: call mfx_sessions_create again");

    const size_t nd = ss.p_descs.size(), ns = ss.p_segs.size(), nc = ss.p_chunks.size(), nr = ss.p_runs.size() / 2, no = ss.p_onorm.size();
    if (nd > 0) {
        int items_max = 0;
        for (SessDesc &d : ss.p_descs) {
            if (d.src_pitch <= 0) d.src_pitch = pitch;
            items_max = std::max(items_max, sess_gather_items(d, pitch, h->cols, ss.xf.set ? h->width : 0));
        }
        // ---- one upload: descriptors | segments | chunks | row runs | run offsets | the normaliser's descriptors
        const size_t o_seg = nd * sizeof(SessDesc), o_chunk = o_seg + ns * sizeof(Segment), o_run = o_chunk + nc * sizeof(Chunk),
                     o_off = o_run + nr * 2 * sizeof(int64_t), o_on = o_off + 2 * sizeof(int32_t), o_xa = o_on + no * sizeof(OnormSessDesc);
        // (session transform: | groups | blocks, or under MFX_ENGINE_SESS_XFORM_PLAIN | segments | their transforms)
        const size_t nxg = ss.p_groups.size(), nxb = ss.p_blocks.size(), nxs = ss.p_xsegs.size();
        const size_t xa_bytes = nxs ? nxs * sizeof(Segment) : nxg * sizeof(SessXfGroup), o_xb = o_xa + xa_bytes;
        const size_t bytes = o_xb + (nxs ? nxs * sizeof(int32_t) : nxb * sizeof(SessXfBlock));
        static_assert(sizeof(OnormSessDesc) % 8 == 0 && sizeof(SessXfGroup) % 8 == 0 && sizeof(SessXfBlock) % 8 == 0, "8-byte parts");
        static_assert(sizeof(SessDesc) % 8 == 0 && sizeof(Segment) % 8 == 0 && sizeof(Chunk) % 8 == 0, "8-byte parts");
        if (bytes > ss.desc_bytes) return fail(h, MFX_ERR_STATE, "session descriptors outgrew their buffer");
        const int b = ss.stage_cur;
        if (ss.stage_used[b]) HIP_TRY(h, hipEventSynchronize(ss.ev_stage[b])); // (the upload before last read this buffer)
        char *st = ss.h_stage[b].p;
        std::memcpy(st, ss.p_descs.data(), o_seg);
        if (ns) std::memcpy(st + o_seg, ss.p_segs.data(), ns * sizeof(Segment));
        if (nc) std::memcpy(st + o_chunk, ss.p_chunks.data(), nc * sizeof(Chunk));
        if (nr) std::memcpy(st + o_run, ss.p_runs.data(), nr * 2 * sizeof(int64_t));
        const int32_t h_off[2] = {0, (int32_t)nr};
        std::memcpy(st + o_off, h_off, sizeof(h_off));
        if (no) std::memcpy(st + o_on, ss.p_onorm.data(), no * sizeof(OnormSessDesc));
        if (nxs) std::memcpy(st + o_xa, ss.p_xsegs.data(), nxs * sizeof(Segment)), std::memcpy(st + o_xb, ss.p_xseg_xf.data(), nxs * sizeof(int32_t));
        if (nxg) std::memcpy(st + o_xa, ss.p_groups.data(), nxg * sizeof(SessXfGroup)), std::memcpy(st + o_xb, ss.p_blocks.data(), nxb * sizeof(SessXfBlock));
        HIP_TRY(h, hipMemcpyAsync(ss.d_desc.p, st, bytes, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipEventRecord(ss.ev_stage[b], h->stream));
        ss.stage_used[b] = true;
        ss.stage_cur = b ^ 1;
        const SessDesc *d_descs = (const SessDesc *)ss.d_desc.p;
        const Segment *d_segs = (const Segment *)(ss.d_desc.p + o_seg);
        const Chunk *d_chunks = (const Chunk *)(ss.d_desc.p + o_chunk);

        // ---- gather: carried PCM tail + new samples + carried static rows -> the current slots
        SessGatherParams gp{};
        gp.descs = d_descs;
        gp.n_descs = (int32_t)nd;
        gp.narrow = (h->cfg.engine & MFX_ENGINE_SESS_NARROW_LOADS) ? 1 : 0;
        gp.pcm = d_pcm;
        gp.pcm_elems = pcm_samples_total * h->channels;
        gp.slot_pcm = ss.d_pcm.p;
        gp.slot_elems = (int64_t)2 * ss.n * ss.pcm_stride * h->channels;
        gp.slot_stat = ss.d_stat.p;
        gp.stat_pitch = pitch;
        gp.cols = h->cols;
        gp.items_max = items_max;
        gp.slot_y = ss.xf.d_y.p;
        gp.y_width = ss.xf.set ? h->width : 0;
        HIP_TRY(h, launch_sess_gather(gp, h->stream));

        // ---- front end over the push's chunks: statics straight to their rows of the current slots
        if (nc > 0) {
            p.pcm = ss.d_pcm.p;
            p.pcm_total = gp.slot_elems;
            p.row_limit = (int64_t)2 * ss.n * ss.row_cap;
            p.feat = ss.d_stat.p;
            p.feat_pitch = pitch;
            // (spectrum kinds: k_melcep_runs / k_plp_runs on the new rows only; a push adds nothing to mfx_profile_read)
            FrontWork w;
            w.h_chunks = ss.p_chunks.data(), w.d_chunks = d_chunks, w.n_chunks = nc;
            w.slab = ss.d_slab.p, w.slab_rows = ss.slab_rows;
            w.tables = &h->own;
            w.runs = (const int64_t *)(ss.d_desc.p + o_run), w.run_off = (const int32_t *)(ss.d_desc.p + o_off);
            w.h_runs = ss.p_runs.data(), w.h_run_off = h_off;
            rc = launch_front(h, p, kind, aligned, w);
            if (rc != MFX_OK) return rc;
        }

        // ---- online normaliser: ahead of the deltas on the new frames' statics in the slots, behind them on the delivered rows
        OnormSessParams op{};
        op.Wn = spk_wn(h);
        op.window = ss.on.window, op.cvn = h->cfg.norm == MFX_NORM_CVN ? 1 : 0, op.prior_frames = ss.on.prior_frames;
        op.prior_count = ss.on.prior_count;
        op.prior_acc = ss.on.d_prior.p;
        op.descs = (const OnormSessDesc *)(ss.d_desc.p + o_on);
        op.n_descs = (int32_t)no;
        op.state = ss.on.d_state.p;
        op.ring = ss.on.d_ring.p;
        if (no > 0 && norm_before(h)) {
            op.data = ss.d_stat.p, op.pitch = pitch;
            HIP_TRY(h, launch_onorm_sess(op, h->stream));
        }

        // ---- delta: the rows every session's push completes, into the caller's array (l1 == 0: the copy form); with a session
        // transform, into the sessions' y slots behind the carried rows
        float *const d_rows = ss.xf.set ? ss.xf.d_y.p : d_out;
        if (ns > 0) {
            DeltaParams dp{};
            dp.src = ss.d_stat.p;
            dp.src_pitch = pitch;
            dp.out = d_rows;
            dp.out_pitch = h->width;
            dp.segs = d_segs;
            dp.n_segs = (int32_t)ns;
            dp.cols = h->cols;
            dp.l1 = h->l1;
            dp.l2 = h->l2;
            dp.tiles_per_seg_max = ss.p_tiles_max;
            HIP_TRY(h, launch_delta(dp, h->stream));
        }
        if (no > 0 && !norm_before(h)) {
            op.data = d_rows, op.pitch = h->width;
            HIP_TRY(h, launch_onorm_sess(op, h->stream));
        }

        // ---- session transform: the rows y in the slots -> the caller's array, [total_rows][out_dim]
        if (nxs > 0 || nxb > 0) {
            SessXformParams xp;
            XformParams pp;
            fill_sess_xform(h, ss.xf.left, ss.xf.right, ss.xf.out, xp, pp);
            if (nxs > 0) { // k_splice_affine itself, one segment per session (the measurement's comparator; same bits)
                pp.src = ss.xf.d_y.p, pp.out = d_out;
                pp.segs = (const Segment *)(ss.d_desc.p + o_xa), pp.n_segs = (int32_t)nxs;
                pp.seg_xf = (const int32_t *)(ss.d_desc.p + o_xb);
                pp.operands = ss.xf.d_ops.p, pp.bias = ss.xf.d_bias.p;
                pp.tiles_per_seg_max = ss.p_xtiles_max;
                HIP_TRY(h, launch_xform(pp, h->stream));
            } else {
                xp.src = ss.xf.d_y.p, xp.out = d_out;
                xp.groups = (const SessXfGroup *)(ss.d_desc.p + o_xa), xp.blocks = (const SessXfBlock *)(ss.d_desc.p + o_xb);
                xp.n_blocks = (int32_t)nxb;
                xp.operands = ss.xf.d_ops.p, xp.bias = ss.xf.d_bias.p;
                xp.tile_rows = 16 * ss.xf.G;
                HIP_TRY(h, launch_sess_xform(xp, h->stream));
            }
        }
    }
    // ---- the launches are queued: commit
    for (int i = 0; i < n; ++i) {
        SessState::Live &lv = ss.live[ss.p_ids[i]];
        lv = ss.p_next[i];
        if (lv.pitch < 0) lv.pitch = pitch;
    }
    ss.planned = false;
    return MFX_OK;
}

extern "C" int mfx_sessions_run_host(mfx_handle *h, const int16_t *pcm, int64_t pcm_samples_total, float *out)
{
    MFX_DEVICE_ENTRY(h);
    SessState &ss = h->sess;
    if (ss.n == 0) return not_created(h);
    if (!ss.planned) return fail(h, MFX_ERR_STATE, "mfx_sessions_run: no push is planned (mfx_sessions_plan), or it has run already");
    if (pcm_samples_total < 0 || (pcm_samples_total > 0 && !pcm) || (ss.p_total_rows > 0 && !out)) return fail(h, MFX_ERR_ARG, "invalid argument");
    HIP_TRY(h, hipSetDevice(h->device));
    // device copies of the caller's buffers, grown on demand (this entry may allocate; mfx_sessions_run_device never does)
    const size_t n_in = (size_t)pcm_samples_total * h->channels, n_out = (size_t)ss.p_total_rows * sess_out_width(h);
    if (ss.d_host_pcm.n < n_in + 8 || ss.d_host_out.n < n_out + 4) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (ss.d_host_pcm.n < n_in + 8) HIP_TRY(h, ss.d_host_pcm.alloc(n_in + 8));
        if (ss.d_host_out.n < n_out + 4) HIP_TRY(h, ss.d_host_out.alloc(n_out + 4));
    }
    if (n_in > 0) HIP_TRY(h, hipMemcpyAsync(ss.d_host_pcm.p, pcm, n_in * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
    const int64_t rows = ss.p_total_rows;
    const int rc = mfx_sessions_run_device(h, ss.d_host_pcm.p, pcm_samples_total, ss.d_host_out.p);
    if (rc != MFX_OK) {
        (void)hipStreamSynchronize(h->stream); // (nothing may still read `pcm` once we have returned)
        return rc;
    }
    if (rows > 0) HIP_TRY(h, hipMemcpyAsync(out, ss.d_host_out.p, (size_t)rows * sess_out_width(h) * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MFX_OK;
}

extern "C" int32_t mfx_host_session_step(int32_t window, int32_t shift, int32_t D, int64_t state[2], int64_t length, int32_t final_flag,
                                         int64_t *carry_samples, int32_t *carry_rows, int32_t *new_frames, int32_t seg[5])
{
    if (window <= 0 || shift <= 0 || D < 0 || !state || state[0] < 0 || state[1] < 0 || length < 0) return MFX_ERR_ARG;
    SessionStep st;
    const int32_t n_out = session_step(window, shift, D, state[0], state[1], length, final_flag != 0, st);
    if (carry_samples) *carry_samples = st.carry_samples;
    if (carry_rows) *carry_rows = st.carry_rows;
    if (new_frames) *new_frames = st.new_frames;
    if (seg) seg[0] = st.n_out, seg[1] = st.shift, seg[2] = st.lo, seg[3] = st.hi, seg[4] = st.static_off;
    return n_out;
}

extern "C" int32_t mfx_host_session_xform_step(int32_t left, int32_t right, int64_t state[2], int32_t n_y, int32_t final_flag,
                                               int32_t *carry_rows, int32_t win[3])
{
    if (left < 0 || left > 32 || right < 0 || right > 32 || !state || state[0] < 0 || state[1] < 0 || state[1] > state[0] || n_y < 0)
        return MFX_ERR_ARG;
    SessionXformStep st;
    const int32_t n_out = session_xform_step(left, right, state[0], state[1], n_y, final_flag != 0, st);
    if (carry_rows) *carry_rows = st.carry_rows;
    if (win) win[0] = st.src_row0, win[1] = st.lo, win[2] = st.hi;
    return n_out;
}

extern "C" int32_t mfx_host_sess_xform_groups(int32_t n, const int32_t *n_out, const int32_t *xf, int32_t G, int32_t *groups, int32_t groups_cap,
                                              int32_t *blocks, int32_t blocks_cap, int32_t *n_blocks)
{
    if (n < 0 || (n > 0 && (!n_out || !xf)) || (G != 1 && G != 2 && G != 4)) return MFX_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (n_out[i] < 0 || xf[i] < 0) return MFX_ERR_ARG;
    std::vector<int32_t> order, gp, gr0, gn, bg0, bng, bxf;
    pack_sess_xform_groups(n_out, xf, n, G, order, gp, gr0, gn, bg0, bng, bxf);
    if (n_blocks) *n_blocks = (int32_t)bg0.size();
    if (groups) {
        if ((size_t)groups_cap < gp.size()) return MFX_ERR_ARG;
        for (size_t g = 0; g < gp.size(); ++g) groups[3 * g] = gp[g], groups[3 * g + 1] = gr0[g], groups[3 * g + 2] = gn[g];
    }
    if (blocks) {
        if ((size_t)blocks_cap < bg0.size()) return MFX_ERR_ARG;
        for (size_t k = 0; k < bg0.size(); ++k) blocks[3 * k] = bg0[k], blocks[3 * k + 1] = bng[k], blocks[3 * k + 2] = bxf[k];
    }
    return (int32_t)gp.size();
}
