// mfx_sessions_host.cpp -- the session entries of include/mfx.h: many open streams, each advanced by one chunk of samples per
// push, all of them in one launch sequence (k_sess_gather -> front end -> delta, with k_onorm_sess before or after the delta
// while the online normaliser is set, k_sess_xform as the last launch while a session transform is set, and k_sess_resample as
// the first while session rates are set and a piece has something to convert).  DESIGN.md section 5, "Session entries",
// "Session transform", "Session sample-rate conversion" and "Session log-mel" (an STFT log-mel handle: k_sess_gather moves PCM
// only, and k_sess_stft_mel stands where front end and delta stage do).
// This file owns the handle's `sess` part.  It reads the shared geometry and tables and names no field of `st`, `sweep`,
// `batch` or `fuse`: a push leaves the streaming state and the batch plan, alpha list and transform as they are.
#include "mfx_handle.h"

#include <cstdint>
#include <cstring>
#include <iterator>
#include <numeric>
#include <string>

using namespace mfx;

namespace {

using Push = SessState::Push;
using Piece = SessState::Piece;

int not_created(mfx_handle *h) { return fail(h, MFX_ERR_STATE, "mfx_sessions_create has not been called"); }
// the refusal of the setters that are valid only while no sessions exist
int sessions_exist(mfx_handle *h, const char *who) { return fail(h, MFX_ERR_STATE, std::string(who) + ": sessions exist (mfx_sessions_create(0, 0) first)"); }
// the slot arrays' frames lie on even samples exactly when the shift is even: slot bases and pcm_stride are even
bool sess_aligned(const mfx_handle *h) { return (h->S % 2) == 0; }
bool norm_before(const mfx_handle *h) { return h->cfg.norm != MFX_NORM_NONE && !h->cfg.norm_after_dyn; }
bool xform_plain(const mfx_handle *h) { return (h->cfg.engine & MFX_ENGINE_SESS_XFORM_PLAIN) != 0; }
bool stft_plain(const mfx_handle *h) { return (h->cfg.engine & MFX_ENGINE_SESS_STFT_PLAIN) != 0; }

// The single upload of a push: descriptors | segments | chunks | row runs | run offsets | the normaliser's descriptors | the
// transform's groups | its blocks (under MFX_ENGINE_SESS_XFORM_PLAIN: | its segments | their transforms) | the converter's
// tiles (session rates) | the groups of k_sess_stft_mel (STFT log-mel), every part on an 8-byte boundary.  The constructor is the one place that lists them.  mfx_sessions_create calls it on a push whose lists have
// their largest sizes, without a staging buffer, for the bytes d_desc and the staging need; the run calls it on the planned
// push: the parts are copied into `stage` and their addresses in `dev` are the members.
struct SessUpload {
    const SessDesc *descs = nullptr;
    const Segment *segs = nullptr;
    const Chunk *chunks = nullptr;
    const int64_t *runs = nullptr;
    const int32_t *run_off = nullptr;
    const OnormSessDesc *onorm = nullptr;
    const void *xa = nullptr, *xb = nullptr;
    const SessResTile *rtiles = nullptr;
    const StftChunk *stft = nullptr;
    size_t bytes = 0;
    SessUpload() = default;
    SessUpload(const Push &ps, char *stage, char *dev)
    {
        static_assert(sizeof(OnormSessDesc) % 8 == 0 && sizeof(SessXfGroup) % 8 == 0 && sizeof(SessXfBlock) % 8 == 0, "8-byte parts");
        static_assert(sizeof(SessDesc) % 8 == 0 && sizeof(Segment) % 8 == 0 && sizeof(Chunk) % 8 == 0, "8-byte parts");
        auto put = [&](const auto &v) { // (a vector, or the two run offsets)
            const size_t off = (bytes + 7) & ~(size_t)7, part = std::size(v) * sizeof(*std::data(v));
            bytes = off + part;
            if (stage && part) std::memcpy(stage + off, std::data(v), part);
            return (decltype(std::data(v)))(stage ? dev + off : nullptr);
        };
        descs = put(ps.descs), segs = put(ps.segs), chunks = put(ps.chunks), runs = put(ps.runs), run_off = put(ps.run_off);
        onorm = put(ps.onorm);
        const bool plain = !ps.xsegs.empty();
        xa = plain ? (const void *)put(ps.xsegs) : put(ps.groups), xb = plain ? (const void *)put(ps.xseg_xf) : put(ps.blocks);
        static_assert(sizeof(SessResTile) % 8 == 0, "8-byte parts");
        rtiles = put(ps.rtiles); // (session rates: the converter's tiles)
        static_assert(sizeof(StftChunk) % 8 == 0, "8-byte parts");
        stft = put(ps.stft); // (STFT log-mel: the frame groups)
    }
};

} // namespace

extern "C" int mfx_sessions_create(mfx_handle *h, int32_t n_sessions, int32_t max_push_samples)
{
    MFX_DEVICE_ENTRY(h);
    if (h->traps)
        return fail(h, MFX_ERR_STATE, "the session entries do not serve TRAPS handles (their look-ahead is (L - 1) / 2 frames, not D)");
    if (h->stft_form == StftForm::Fft)
        return fail(h, MFX_ERR_STATE,
                    "the session entries do not serve STFT log-mel handles of DFT length 1024 / 2048 (the carried-tail rule stops at 512): "
                    "use the batch entries (mfx_batch_plan + mfx_batch_run_device / mfx_batch_run_host)");
    if (h->stft && h->cfg.logmel_post == MFX_LOGMEL_WHISPER)
        return fail(h, MFX_ERR_STATE,
                    "the session entries do not serve MFX_LOGMEL_WHISPER (its clamp needs the largest value of the whole utterance): use "
                    "the batch entries (mfx_batch_plan + mfx_batch_run_device), or MFX_LOGMEL_LOG10 / MFX_LOGMEL_LN");
    if (h->kaldi && (h->kaldi_flags & kKaldiNoSnipEdges))
        return fail(h, MFX_ERR_STATE,
                    "the session entries do not serve a Kaldi handle with MFX_KALDI_NO_SNIP_EDGES (its frames are mirrored at the true "
                    "ends of the stream: another carry and delivery rule): use the batch entries (mfx_batch_plan + mfx_batch_run_device / "
                    "mfx_batch_run_host)");
    if (h->cfg.norm != MFX_NORM_NONE && !h->sess.on.set) // (mfx_sessions_set_online_norm: the one normaliser served)
        return fail(h, MFX_ERR_STATE,
                    "the session entries do not serve normalisation (norm != MFX_NORM_NONE): statistics over an open stream are not built");
    if (n_sessions < 0 || max_push_samples < 0 || (n_sessions == 0) != (max_push_samples == 0))
        return fail(h, MFX_ERR_ARG, "n_sessions and max_push_samples must both be positive (or both 0: release)");
    if (n_sessions > (1 << 20) || max_push_samples > (1 << 24)) return fail(h, MFX_ERR_ARG, "n_sessions or max_push_samples too large");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    SessState &ss = h->sess;
    Push &ps = ss.push;
    ss.n = 0;
    ps.planned = false;
    ps.clear_lists();
    ss.live.clear();
    ss.stage_used[0] = ss.stage_used[1] = false;
    ss.rs.last_valid = false;
    if (n_sessions == 0) {
        ss.release();
        ss.max_push = ss.max_conv = 0;
        return MFX_OK;
    }
    // session rates: the largest converted piece, max over rates ceil((max_push + Wh) L / M) + 1 (a final push converts its
    // piece and the Wh samples' worth of outputs the open stream held back; this is also the bound of a flush)
    int64_t max_conv = max_push_samples;
    if (ss.rs.set)
        for (const ResRate &r : ss.rs.rates)
            if (r.tile_out > 0) max_conv = std::max(max_conv, (((int64_t)max_push_samples + r.Wh) * r.L + r.M - 1) / r.M + 1);
    if (max_conv > (1 << 24)) return fail(h, MFX_ERR_ARG, "max_push_samples too large after conversion to sample_rate");
    int rc = refresh_mel(h); // (decides which front end the shape takes, and with it whether a spectrum slab is needed)
    if (rc != MFX_OK) return rc;
    const int ch = h->channels;
    const size_t n = (size_t)n_sessions;
    ss.max_push = max_push_samples;
    ss.max_conv = (int32_t)max_conv;
    ss.pcm_stride = ((int64_t)h->W + h->S + max_conv + 2 + 7) & ~(int64_t)7;
    ss.frames_max = (int32_t)(max_conv / h->S + 1);
    ss.row_cap = 2 * h->D + ss.frames_max;
    ss.stft_G = 0;
    ss.d_stft_max.release();
    if (h->stft) { // rows of a push: its own and a final push's N / (2 S) + 1 more; no statics live in the slots
        ss.frames_max = (int32_t)session_stft_rows_max(h->W, h->S, max_conv);
        ss.row_cap = 1;
        ss.stft_G = sess_stft_groups(h->W, h->S, h->nb);
        if (ss.stft_G == 0) return fail(h, MFX_ERR_CONFIG, "no block packing of k_sess_stft_mel fits the LDS for this shape");
    }
    ss.row_floats = (std::max(16, h->width) + 3) & ~3;
    const size_t pcm_elems = (size_t)2 * n_sessions * ss.pcm_stride * ch;
    HIP_TRY(h, ss.d_pcm.alloc(pcm_elems + 8));
    HIP_TRY(h, hipMemsetAsync(ss.d_pcm.p, 0, (pcm_elems + 8) * sizeof(int16_t), h->stream));
    HIP_TRY(h, ss.d_stat.alloc((size_t)2 * n_sessions * ss.row_cap * ss.row_floats));
    ss.slab_rows = 0;
    ss.d_slab.release();
    if (!h->stft && is_spec_kind(choose_front(h, sess_aligned(h)))) {
        ss.slab_rows = std::min<int64_t>((int64_t)2 * n_sessions * ss.row_cap, kSlabRowsMax);
        HIP_TRY(h, ss.d_slab.alloc((size_t)ss.slab_rows * h->spec_pitch));
    }
    // the push's lists at their largest: resizing reserves them (a warm plan allocates nothing), SessUpload sizes their upload
    ps.pieces.reserve(n), ss.p_order.reserve(n);
    ps.descs.resize(n), ps.segs.resize(n), ps.runs.resize(2 * n);
    if (h->stft) { // groups of 16 frames, or the chunks of k_stft_mel and the slots of their maxima
        const size_t per = (size_t)ss.frames_max / (stft_plain(h) ? h->stft_R : 16) + 1;
        ps.stft.resize(n * per), ss.p_stft_rows.reserve(n), ss.p_stft_cuts.reserve(n * per);
        if (stft_plain(h)) HIP_TRY(h, ss.d_stft_max.alloc(n * per));
    } else {
        ps.chunks.resize(n * ((ss.frames_max + kChunkFrames - 1) / kChunkFrames));
    }
    ss.xf.d_y.release();
    if (ss.xf.set) { // the session transform: the two y slot arrays, the operands; the work list of the handle's launch form
        ss.xf.y_cap = ss.xf.left + ss.xf.right + ss.frames_max + h->D;
        HIP_TRY(h, ss.xf.d_y.alloc((size_t)2 * n_sessions * ss.xf.y_cap * h->width));
        HIP_TRY(h, h->upload(ss.xf.d_ops, ss.xf.ops));
        HIP_TRY(h, h->upload(ss.xf.d_bias, ss.xf.bias));
        const size_t groups_max = n * ((ss.frames_max + h->D + ss.xf.right) / 16 + 1);
        ps.xf_rows.reserve(n), ps.xf_idx.reserve(n);
        if (xform_plain(h))
            ps.xsegs.resize(n), ps.xseg_xf.resize(n);
        else
            ps.groups.resize(groups_max), ps.blocks.resize(groups_max), ss.p_cuts.reserve(groups_max), ss.p_packs.reserve(groups_max);
    }
    if (h->cfg.norm != MFX_NORM_NONE) { // the online normaliser's state: 8 doubles per session and column, the ring of raw rows
        const size_t Wn = (size_t)spk_wn(h);
        HIP_TRY(h, ss.on.d_state.alloc((size_t)n_sessions * 8 * Wn));
        HIP_TRY(h, ss.on.d_ring.alloc((size_t)n_sessions * ss.on.window * Wn));
        HIP_TRY(h, h->upload(ss.on.d_prior, ss.on.prior));
        ps.onorm.resize(n);
    }
    ss.rs.d_carry.release(), ss.rs.d_conv.release();
    if (ss.rs.set) { // the session rates: tables, the two carry slot arrays, the scratch of converted pieces; the tile list
        SessState::Rates &rs = ss.rs;
        rs.conv_stride = (max_conv + 1) & ~(int64_t)1;
        HIP_TRY(h, h->upload(rs.d_taps, rs.taps));
        HIP_TRY(h, h->upload(rs.d_rates, rs.rates));
        const size_t carry_elems = (size_t)2 * n * rs.carry_cap * ch + 8, conv_elems = n * (size_t)rs.conv_stride * ch + 8;
        HIP_TRY(h, rs.d_carry.alloc(carry_elems));
        HIP_TRY(h, hipMemsetAsync(rs.d_carry.p, 0, carry_elems * sizeof(int16_t), h->stream));
        HIP_TRY(h, rs.d_conv.alloc(conv_elems));
        HIP_TRY(h, hipMemsetAsync(rs.d_conv.p, 0, conv_elems * sizeof(int16_t), h->stream));
        ps.rtiles.resize(n * (size_t)(max_conv / rs.tile_min + 2));
        ps.c_off.reserve(n), ps.c_len.reserve(n), rs.last_off.reserve(n), rs.last_len.reserve(n);
    }
    ss.desc_bytes = SessUpload(ps, nullptr, nullptr).bytes;
    ps.clear_lists();
    HIP_TRY(h, ss.d_desc.alloc(ss.desc_bytes));
    for (int b = 0; b < 2; ++b) {
        HIP_TRY(h, ss.h_stage[b].grow(ss.desc_bytes, ss.desc_bytes, h->stream));
        if (!ss.ev_stage[b]) HIP_TRY(h, hipEventCreateWithFlags(&ss.ev_stage[b], hipEventDisableTiming));
    }
    ss.live.assign(n, SessState::Live{});
    ss.p_seen.assign(n, 0);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    ss.n = n_sessions;
    return MFX_OK;
}

extern "C" int mfx_sessions_set_online_norm(mfx_handle *h, int32_t window, int32_t prior_frames, int64_t prior_count, const double *prior_acc)
{
    MFX_DEVICE_ENTRY(h);
    int rc = check_online_norm(h, "mfx_sessions_set_online_norm", window, prior_frames, prior_count, prior_acc);
    if (rc == MFX_ERR_CONFIG) return rc;
    if (h->sess.n != 0) return sessions_exist(h, "mfx_sessions_set_online_norm");
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
    if (h->sess.n != 0) return sessions_exist(h, "mfx_sessions_clear_online_norm");
    h->sess.on.set = false;
    h->sess.on.prior.clear();
    return MFX_OK;
}

extern "C" int mfx_sessions_set_transform(mfx_handle *h, int32_t left, int32_t right, int32_t out_dim, int32_t n_xf, const float *A,
                                          const float *b)
{
    MFX_DEVICE_ENTRY(h);
    if (h->sess.n != 0) return sessions_exist(h, "mfx_sessions_set_transform");
    if (!A) return fail(h, MFX_ERR_ARG, "no matrix");
    if (left < 0 || left > 32 || right < 0 || right > 32) return fail(h, MFX_ERR_ARG, "left and right must be 0 .. 32");
    if (out_dim < 1 || out_dim > 256) return fail(h, MFX_ERR_ARG, "out_dim must be 1 .. 256");
    if (n_xf < 1 || n_xf > 1024) return fail(h, MFX_ERR_ARG, "n_xf must be 1 .. 1024");
    const int64_t in_dim = (int64_t)(left + right + 1) * h->width;
    if (in_dim > 8192) return fail(h, MFX_ERR_ARG, "in_dim = (left + right + 1) * width is larger than 8192");
    SessXformParams probe;
    XformParams plain;
    fill_xform_shape(h, probe, h->width, left, right, out_dim);
    fill_xform_shape(h, plain, h->width, left, right, out_dim);
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
    if (h->sess.n != 0) return sessions_exist(h, "mfx_sessions_clear_transform");
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
    if (ss.live[session].n != 0 || ss.live[session].n_in != 0)
        return fail(h, MFX_ERR_STATE, "mfx_sessions_select_transform: the session has received samples since its last final push or reset");
    ss.live[session].xf = xf;
    ss.push.planned = false; // (a pending push was planned with the earlier choice)
    return MFX_OK;
}

extern "C" int mfx_sessions_set_rates(mfx_handle *h, int32_t n_rates, const int32_t *rates_hz, int32_t zeros, float rolloff)
{
    MFX_DEVICE_ENTRY(h);
    if (h->sess.n != 0) return sessions_exist(h, "mfx_sessions_set_rates");
    if (n_rates < 1 || n_rates > 16 || !rates_hz) return fail(h, MFX_ERR_ARG, "n_rates must be 1 .. 16");
    // (the range first: a float outside int32 must not reach the cast)
    if (!(h->cfg.sample_rate >= 1000.f && h->cfg.sample_rate <= 768000.f))
        return fail(h, MFX_ERR_ARG, "sample rates must lie in 1000 .. 768000 Hz");
    const int32_t out_hz = (int32_t)h->cfg.sample_rate;
    if ((float)out_hz != h->cfg.sample_rate) return fail(h, MFX_ERR_CONFIG, "mfx_sessions_set_rates: sample_rate is not an integral number of Hz");
    // the tables and tile geometry of every rate, as mfx_batch_plan_rates builds them (a pass-through rate has none, but
    // zeros and rolloff are judged for it too)
    ResRateSet set;
    if (const int e = build_resample_rates(h->channels, out_hz, rates_hz, n_rates, zeros, rolloff, true, set); e != 0)
        return fail(h, MFX_ERR_ARG, kResampleWhy[e]);
    if (resample_lds_bytes(h->channels, set.lds) > kLdsCap) return fail(h, MFX_ERR_ARG, "no tile of k_sess_resample fits the LDS for this shape");
    SessState::Rates &rs = h->sess.rs;
    rs.hz.assign(rates_hz, rates_hz + n_rates);
    rs.rates.swap(set.rates), rs.taps.swap(set.taps);
    rs.lds = set.lds, rs.carry_cap = set.carry_cap, rs.tile_min = set.tile_min;
    rs.set = true;
    return MFX_OK;
}

extern "C" int mfx_sessions_clear_rates(mfx_handle *h)
{
    MFX_DEVICE_ENTRY(h);
    if (h->sess.n != 0) return sessions_exist(h, "mfx_sessions_clear_rates");
    SessState::Rates &rs = h->sess.rs;
    rs.set = false;
    rs.hz.clear(), rs.rates.clear(), rs.taps.clear();
    return MFX_OK;
}

extern "C" int mfx_sessions_select_rate(mfx_handle *h, int32_t session, int32_t rate_index)
{
    MFX_DEVICE_ENTRY(h);
    SessState &ss = h->sess;
    if (!ss.rs.set) return fail(h, MFX_ERR_STATE, "mfx_sessions_select_rate: no session rates are set");
    if (ss.n == 0) return not_created(h);
    if (session < 0 || session >= ss.n) return fail(h, MFX_ERR_ARG, "session id outside [0, n_sessions)");
    if (rate_index < 0 || rate_index >= (int32_t)ss.rs.rates.size()) return fail(h, MFX_ERR_ARG, "rate index outside [0, n_rates)");
    if (ss.live[session].n != 0 || ss.live[session].n_in != 0)
        return fail(h, MFX_ERR_STATE, "mfx_sessions_select_rate: the session has received samples since its last final push or reset");
    ss.live[session].rate = rate_index;
    ss.push.planned = false; // (a pending push was planned with the earlier choice)
    return MFX_OK;
}

extern "C" int64_t mfx_sessions_converted_read(mfx_handle *h, int16_t *dst, int64_t cap_elems, int64_t *offsets, int64_t *lengths)
{
    MFX_DEVICE_ENTRY(h);
    SessState &ss = h->sess;
    if (!ss.rs.set) return fail(h, MFX_ERR_STATE, "mfx_sessions_converted_read: no session rates are set");
    if (ss.n == 0) return not_created(h);
    if (!ss.rs.last_valid)
        return fail(h, MFX_ERR_STATE, "mfx_sessions_converted_read: the last push converted nothing (its samples are the caller's own)");
    const int ch = h->channels;
    int64_t total = 0;
    for (const int64_t len : ss.rs.last_len) total += len * ch;
    if (dst && cap_elems < total) return fail(h, MFX_ERR_BUFFER_TOO_SMALL, "mfx_sessions_converted_read: dst is too small");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int64_t at = 0;
    for (size_t i = 0; i < ss.rs.last_len.size(); ++i) {
        const int64_t len = ss.rs.last_len[i];
        if (offsets) offsets[i] = at;
        if (lengths) lengths[i] = len;
        if (dst && len > 0)
            HIP_TRY(h, hipMemcpy(dst + at * ch, ss.rs.d_conv.p + ss.rs.last_off[i] * ch, (size_t)len * ch * sizeof(int16_t), hipMemcpyDeviceToHost));
        at += len;
    }
    return total;
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
        const int parity = ss.live[s].parity, xf = ss.live[s].xf, rate = ss.live[s].rate, rs_parity = ss.live[s].rs_parity;
        ss.live[s] = SessState::Live{}; // (the carried samples, static rows, rows y and carried input go with it)
        ss.live[s].parity = parity, ss.live[s].xf = xf, ss.live[s].rate = rate, ss.live[s].rs_parity = rs_parity;
    }
    ss.push.planned = false; // (a pending push was planned on the state just dropped)
    return MFX_OK;
}

extern "C" int64_t mfx_sessions_delivered(const mfx_handle *h, int32_t session)
{
    if (!h) return MFX_ERR_ARG;
    if (h->sess.n == 0) return MFX_ERR_STATE;
    if (session < 0 || session >= h->sess.n) return MFX_ERR_ARG;
    return h->sess.xf.set ? h->sess.live[session].Ex : h->sess.live[session].E;
}

namespace {

// ---- mfx_sessions_plan: check_pieces -> plan_rates (session rates) -> plan_steps -> plan_slots -> plan_xform_work -> plan_stft_work (STFT log-mel)

// the samples the front end will have seen of session id once `length` more have arrived (session rates: after conversion)
int64_t stream_samples(const SessState &ss, int32_t id, int64_t length)
{
    const SessState::Live &lv = ss.live[id];
    if (!ss.rs.set) return lv.n + length;
    const ResRate &r = ss.rs.rates[lv.rate];
    const int64_t n = lv.n_in + length;
    if (r.tile_out == 0) return n;
    return n > INT64_MAX / r.L ? INT64_MAX : (n * r.L + r.M - 1) / r.M;
}

// ---- stage 1: the checks (lengths against max_push_samples: in input samples while session rates are set).  Nothing behind them fails; every refusal leaves p_seen clean (and no push planned)
int check_pieces(mfx_handle *h, int32_t n, const int32_t *ids, const int64_t *offsets, const int64_t *lengths)
{
    SessState &ss = h->sess;
    int bad = MFX_OK, i = 0;
    const char *why = "";
    for (; i < n && bad == MFX_OK; ++i) {
        const int32_t id = ids[i];
        if (id < 0 || id >= ss.n)
            bad = MFX_ERR_ARG, why = "session id outside [0, n_sessions)";
        else if (ss.p_seen[id])
            bad = MFX_ERR_ARG, why = "session id given twice in one push";
        else if (offsets[i] < 0 || lengths[i] < 0)
            bad = MFX_ERR_ARG, why = "negative offset or length";
        else if (offsets[i] > INT64_MAX / 4 - lengths[i]) // (the end, times the channels, stays inside int64)
            bad = MFX_ERR_ARG, why = "offset + length too large";
        else if (lengths[i] > ss.max_push)
            bad = MFX_ERR_BUFFER_TOO_SMALL, why = "a session's piece is longer than max_push_samples (mfx_sessions_create)";
        else if (utt_frame_count(h, stream_samples(ss, id, lengths[i])) > 0x7fffffff)
            bad = MFX_ERR_ARG, why = "stream too long";
        else
            ss.p_seen[id] = 1;
    }
    while (--i >= 0) // (the ids marked, and the one refused: not marked, or marked by the piece that gave it first)
        if (ids[i] >= 0 && ids[i] < ss.n) ss.p_seen[ids[i]] = 0;
    return bad == MFX_OK ? MFX_OK : fail(h, bad, why);
}

// ---- stage 2, session rates (the caller's order): every piece's input length becomes its converted length
// (session_resample_step), the converted pieces are laid out in the scratch, each on an even sample, and the converter's tiles
// are listed.  A push without a piece to convert keeps the caller's own offsets and lengths: it reads the caller's array.
void plan_rates(mfx_handle *h, int32_t n, const int32_t *ids, const int64_t *offsets, const int64_t *lengths, const int32_t *final_flags)
{
    SessState &ss = h->sess;
    Push &ps = ss.push;
    const SessState::Rates &rs = ss.rs;
    const int ch = h->channels;
    ps.pieces.resize(n);
    ps.c_off.assign(offsets, offsets + n), ps.c_len.assign(lengths, lengths + n);
    ps.convert = ps.need_pcm = false;
    ps.max_end = 0;
    for (int i = 0; i < n; ++i) {
        const SessState::Live &cur = ss.live[ids[i]];
        const bool fin = final_flags && final_flags[i] != 0;
        if (rs.rates[cur.rate].tile_out > 0 && (lengths[i] > 0 || (fin && cur.n_in > 0))) ps.convert = true;
        if (lengths[i] > 0) ps.need_pcm = true, ps.max_end = std::max(ps.max_end, offsets[i] + lengths[i]);
    }
    int64_t at = 0; // the scratch's next free sample (even)
    for (int i = 0; i < n; ++i) {
        const int32_t id = ids[i];
        const SessState::Live &cur = ss.live[id];
        const ResRate &r = rs.rates[cur.rate];
        const bool fin = final_flags && final_flags[i] != 0, pass = r.tile_out == 0;
        Piece &pc = ps.pieces[i];
        int64_t N = cur.n_in, J = cur.n;
        SessionResampleStep st;
        const int64_t n_conv = session_resample_step(pass ? 1 : r.L, pass ? 1 : r.M, pass ? 0 : r.Wh, N, J, lengths[i], fin, st);
        pc.n_in_next = N, pc.rs_parity_next = cur.rs_parity;
        if (!ps.convert) continue;
        ps.c_off[i] = at, ps.c_len[i] = n_conv;
        at += (n_conv + 1) & ~(int64_t)1;
        if (n_conv == 0 && st.carry_out == 0) continue; // (nothing to convert, nothing to carry on)
        SessResTile t{};
        t.in_off = offsets[i], t.out_off = ps.c_off[i];
        t.carry_src = ((int64_t)cur.rs_parity * ss.n + id) * rs.carry_cap * ch;
        t.carry_dst = ((int64_t)(cur.rs_parity ^ 1) * ss.n + id) * rs.carry_cap * ch;
        t.c0 = st.c0_old, t.n_old = cur.n_in, t.n_new = cur.n_in + lengths[i], t.c1 = st.c0_new;
        t.j_old = cur.n, t.j_new = cur.n + n_conv;
        t.rate = pass ? -1 : cur.rate;
        t.move = st.carry_out > 0;
        if (!pass) pc.rs_parity_next = cur.rs_parity ^ 1; // (the carry, or nothing after a final push, is in the other slot)
        const int64_t step = pass ? kResCopyTile : r.tile_out;
        t.j0 = t.j_old;
        do {
            ps.rtiles.push_back(t);
            t.move = 0, t.j0 += step;
        } while (t.j0 < t.j_new);
    }
}

// ---- stage 3 (pass 1, the caller's order): every piece's step and its output rows
void plan_steps(mfx_handle *h, int32_t n, const int32_t *ids, const int64_t *offsets, const int64_t *lengths, const int32_t *final_flags,
                int64_t *out_rows, int32_t *out_counts)
{
    SessState &ss = h->sess;
    Push &ps = ss.push;
    ps.pieces.resize(n); // (plan_rates has done so already, and left its fields)
    if (ss.xf.set) ps.xf_rows.assign(n, 0), ps.xf_idx.assign(n, 0);
    ps.total_rows = ps.max_end = 0;
    for (int i = 0; i < n; ++i) {
        Piece &pc = ps.pieces[i];
        const SessState::Live &cur = ss.live[ids[i]];
        pc.id = ids[i], pc.off = offsets[i], pc.len = lengths[i], pc.fin = final_flags && final_flags[i] != 0;
        pc.next = cur; // (n, E and Ex advance here; the slot fields follow in plan_slots)
        if (ss.rs.set) pc.next.n_in = pc.n_in_next, pc.next.rs_parity = pc.rs_parity_next; // (plan_rates has advanced them)
        int32_t n_del;
        if (h->stft) { // (no frame is computed ahead of its delivery and no static row carried: D = 0)
            n_del = session_stft_step(h->W, h->S, pc.next.n, pc.next.E, pc.len, pc.fin, pc.sstep);
            pc.step = SessionStep{};
            pc.step.carry_samples = pc.sstep.carry_in, pc.step.n_out = n_del;
        } else {
            n_del = session_step(h->W, h->S, h->D, pc.next.n, pc.next.E, pc.len, pc.fin, pc.step);
        }
        if (ss.xf.set) { // the rows y the push completes are the transform's input; it delivers rows [Ex_old, Ex_new)
            int64_t Ey = cur.E;
            n_del = session_xform_step(ss.xf.left, ss.xf.right, Ey, pc.next.Ex, pc.step.n_out, pc.fin, pc.xstep);
        }
        pc.row = ps.total_rows;
        if (pc.len > 0) ps.max_end = std::max(ps.max_end, pc.off + pc.len);
        if (out_rows) out_rows[i] = pc.row;
        if (out_counts) out_counts[i] = n_del;
        ps.total_rows += n_del;
    }
}

// ---- stage 4 (pass 2, ascending slots: the slab path walks the chunk list in windows of rows): descriptors, chunks, segments,
// the normaliser's rows, the slot fields of every piece's next state
void plan_slots(mfx_handle *h)
{
    SessState &ss = h->sess;
    Push &ps = ss.push;
    const int ch = h->channels, D = h->D;
    const bool xform = ss.xf.set, onorm = h->cfg.norm != MFX_NORM_NONE, before = norm_before(h);
    // the pieces by the slot they move to: keys (slot, piece) sorted as numbers (n_sessions <= 2^20: both parts fit)
    ss.p_order.resize(ps.pieces.size());
    for (size_t i = 0; i < ps.pieces.size(); ++i) {
        const int32_t id = ps.pieces[i].id;
        ss.p_order[i] = ((int64_t)(ss.live[id].parity ^ 1) * ss.n + id) << 20 | (int64_t)i;
    }
    std::sort(ss.p_order.begin(), ss.p_order.end());
    ps.tiles_max = 0, ps.any_new = false;
    for (const int64_t key : ss.p_order) {
        const int i = (int)(key & 0xfffff);
        Piece &pc = ps.pieces[i];
        const SessionStep &st = pc.step;
        const SessState::Live &cur = ss.live[pc.id];
        SessState::Live &nx = pc.next;
        const bool fin = pc.fin;
        // nothing to move, compute or deliver: an empty push of an open stream, the flush of a stream without samples
        if (pc.len == 0 && (!fin || cur.n == 0)) continue;
        const int64_t f0 = h->stft ? 0 : std::max<int64_t>(cur.E - D, 0); // (STFT log-mel: no static rows in the slots)
        const int64_t slot_prev = (int64_t)cur.parity * ss.n + pc.id, slot_cur = key >> 20;
        SessDesc d{};
        d.carry_src = (slot_prev * ss.pcm_stride + cur.tail_off) * ch, d.carry_n = (int32_t)(st.carry_samples * ch);
        d.new_src = pc.off * ch, d.new_n = (int32_t)(pc.len * ch);
        d.pcm_dst = slot_cur * ss.pcm_stride * ch;
        d.row_src = slot_prev * ss.row_cap + (f0 - cur.f0), d.row_dst = slot_cur * ss.row_cap, d.n_rows = st.carry_rows;
        d.src_pitch = cur.pitch; // (0: nothing carried yet; the run fills in its own pitch)
        int64_t y_row0 = pc.row; // where the delta stage puts the push's first row: d_out, or with a transform the y slot
        if (xform) {
            const SessionXformStep &xs = pc.xstep;
            const int64_t c0 = std::max<int64_t>(cur.Ex - ss.xf.left, 0);
            d.y_src = slot_prev * ss.xf.y_cap + (c0 - cur.y0);
            d.y_dst = slot_cur * ss.xf.y_cap;
            d.y_rows = xs.carry_rows;
            y_row0 = d.y_dst + xs.carry_rows; // (behind the carried rows y)
            nx.y0 = fin ? 0 : c0;
            ps.xf_rows[i] = xs.n_out, ps.xf_idx[i] = cur.xf, pc.xsrc = d.y_dst + xs.src_row0;
        }
        ps.descs.push_back(d);
        ps.any_new = ps.any_new || d.new_n > 0;
        const int64_t new_row0 = d.row_dst + st.carry_rows;
        for (int t0 = 0; t0 < st.new_frames; t0 += kChunkFrames) // (the carried tail starts at the slot's base)
            ps.chunks.push_back(Chunk{slot_cur * ss.pcm_stride + (int64_t)t0 * h->S, new_row0 + t0, std::min(kChunkFrames, st.new_frames - t0), 0});
        if (st.new_frames > 0) ps.runs.push_back(new_row0), ps.runs.push_back(st.new_frames);
        // the online normaliser's rows: the new frames' statics in the slot (frames T_old ..) ahead of the deltas, or the
        // rows the push delivers (rows E_old ..) behind them; a fresh session has 0 rows in front and reads no state
        if (onorm && before && st.new_frames > 0)
            ps.onorm.push_back(OnormSessDesc{new_row0, std::max<int64_t>(frame_count(cur.n, h->W, h->S), 0), st.new_frames, pc.id});
        if (onorm && !before && st.n_out > 0) ps.onorm.push_back(OnormSessDesc{y_row0, cur.E, st.n_out, pc.id});
        if (h->stft) { // the slot holds stream samples [c0_old, n_new) from its base on: the carried tail, then the new samples
            pc.stft_row = y_row0, pc.stft_pcm = slot_cur * ss.pcm_stride - pc.sstep.c0_old;
            nx.parity = cur.parity ^ 1, nx.f0 = 0, nx.tail_off = fin ? 0 : (int32_t)(pc.sstep.c0_new - pc.sstep.c0_old);
            nx.pitch = 0;
            continue;
        }
        if (st.n_out > 0) {
            Segment s{};
            s.src_row0 = d.row_dst, s.out_row0 = y_row0, s.n_out = st.n_out;
            s.shift = st.shift, s.lo = st.lo, s.hi = st.hi, s.static_off = st.static_off;
            ps.segs.push_back(s);
            ps.tiles_max = std::max(ps.tiles_max, (st.n_out + 63) / 64);
        }
        nx.parity = cur.parity ^ 1, nx.f0 = fin ? 0 : f0, nx.tail_off = fin ? 0 : st.new_frames * h->S;
        nx.pitch = fin ? 0 : -1; // (-1: the pitch of the run that writes the slot)
    }
    ps.run_off[0] = 0, ps.run_off[1] = (int32_t)(ps.runs.size() / 2);
}

// ---- stage 5: the transform's work list, pieces in the caller's order: row groups packed into blocks of one transform, or one
// segment per delivering piece
void plan_xform_work(mfx_handle *h)
{
    SessState &ss = h->sess;
    Push &ps = ss.push;
    ps.xtiles_max = 0;
    if (!ss.xf.set) return;
    if (xform_plain(h)) {
        for (size_t i = 0; i < ps.pieces.size(); ++i) {
            const Piece &pc = ps.pieces[i];
            if (ps.xf_rows[i] <= 0) continue;
            Segment s{};
            s.src_row0 = pc.xsrc, s.out_row0 = pc.row, s.n_out = pc.xstep.n_out, s.lo = pc.xstep.lo, s.hi = pc.xstep.hi;
            ps.xsegs.push_back(s), ps.xseg_xf.push_back(ps.xf_idx[i]);
            ps.xtiles_max = std::max(ps.xtiles_max, (pc.xstep.n_out + 63) / 64);
        }
        return;
    }
    pack_sess_xform_groups(ps.xf_rows.data(), ps.xf_idx.data(), (int)ps.pieces.size(), ss.xf.G, ss.p_cuts, ss.p_packs);
    for (const SessXfCut &g : ss.p_cuts) {
        const Piece &pc = ps.pieces[g.piece];
        ps.groups.push_back(SessXfGroup{pc.xsrc, pc.row + g.r0, g.r0, g.rows, pc.xstep.lo, pc.xstep.hi});
    }
    for (const SessXfPack &k : ss.p_packs) ps.blocks.push_back(SessXfBlock{k.g0, k.ng, k.xf, 0});
}

// ---- stage 6, STFT log-mel: the front end's work list, pieces in the caller's order: groups of at most 16 frames for
// k_sess_stft_mel (block b takes groups [G b, G b + G)), or chunks of at most stft_R frames for k_stft_mel.  A group's
// "utterance" is the session's stream: utt_off the element where its sample 0 would lie, utt_len the samples received.  The
// delivery rule keeps every read inside the slot: a negative index occurs only while the slot holds sample 0, an index >= n
// only on a final push, and its reflection lies behind c0_old.
void plan_stft_work(mfx_handle *h)
{
    SessState &ss = h->sess;
    Push &ps = ss.push;
    if (!h->stft) return;
    const int n = (int)ps.pieces.size();
    auto chunk = [&](const Piece &pc, int r0, int rows) {
        const int64_t E_old = ss.live[pc.id].E, n_new = ss.live[pc.id].n + pc.len;
        ps.stft.push_back(make_stft_chunk(pc.stft_pcm, n_new, pc.stft_row + r0, (int32_t)(E_old + r0), rows));
    };
    if (stft_plain(h)) {
        for (const Piece &pc : ps.pieces)
            for (int r0 = 0; r0 < pc.step.n_out; r0 += h->stft_R) chunk(pc, r0, std::min(h->stft_R, pc.step.n_out - r0));
        return;
    }
    ss.p_stft_rows.resize(n);
    for (int i = 0; i < n; ++i) ss.p_stft_rows[i] = ps.pieces[i].step.n_out;
    cut_sess_stft_groups(ss.p_stft_rows.data(), n, ss.p_stft_cuts);
    for (const SessStftCut &g : ss.p_stft_cuts) chunk(ps.pieces[g.piece], g.r0, g.rows);
}

} // namespace

extern "C" int mfx_sessions_plan(mfx_handle *h, int32_t n, const int32_t *ids, const int64_t *offsets, const int64_t *lengths,
                                 const int32_t *final_flags, int64_t *out_rows, int32_t *out_counts, int64_t *total_rows)
{
    MFX_DEVICE_ENTRY(h);
    SessState &ss = h->sess;
    if (ss.n == 0) return not_created(h);
    if (n < 0 || (n > 0 && (!ids || !offsets || !lengths))) return fail(h, MFX_ERR_ARG, "invalid argument");
    if (n > ss.n) return fail(h, MFX_ERR_ARG, "more pieces than sessions: an id is given twice or lies outside the range");
    ss.push.planned = false;
    const int rc = check_pieces(h, n, ids, offsets, lengths);
    if (rc != MFX_OK) return rc;
    ss.push.clear_lists(); // (a second plan replaces the first)
    if (ss.rs.set) { // the stages behind see the converted pieces; the run checks the INPUT array
        plan_rates(h, n, ids, offsets, lengths, final_flags);
        const int64_t in_end = ss.push.max_end;
        plan_steps(h, n, ids, ss.push.c_off.data(), ss.push.c_len.data(), final_flags, out_rows, out_counts);
        ss.push.max_end = in_end;
    } else {
        ss.push.convert = false;
        plan_steps(h, n, ids, offsets, lengths, final_flags, out_rows, out_counts);
    }
    if (total_rows) *total_rows = ss.push.total_rows;
    plan_slots(h);
    plan_xform_work(h);
    plan_stft_work(h);
    if (!ss.rs.set) ss.push.need_pcm = ss.push.any_new;
    ss.push.planned = true;
    return MFX_OK;
}

namespace {

// ---- mfx_sessions_run_device: check_run -> upload -> run_resample (session rates) -> run_gather -> run_front -> run_onorm (before) -> run_delta -> run_onorm
// (after) -> run_xform -> commit (an STFT log-mel handle: ... -> run_gather -> run_stft -> run_xform -> commit).  What the stages share:
struct PushRun {
    const int16_t *d_pcm;       // the entry's arguments
    int64_t pcm_total;
    float *d_out;
    bool aligned = true;        // the front end of the shape, as the batch entries choose it
    FrontKind kind = kFront512;
    FrontParams front;          // of the shape, as the batch entries fill it
    int pitch = 0;              // floats per row of the statics this run writes, as batch_run_range gives them
    int items_max = 0;          // k_sess_gather's grid
    SessUpload up;              // the uploaded lists, on the device
    float *d_rows = nullptr;    // where the delta stage writes: d_out, or with a session transform the y slots
};

// ---- stage 1: the arguments against the planned push; the front end of the shape and the statics' pitch
int check_run(mfx_handle *h, PushRun &r)
{
    SessState &ss = h->sess;
    const Push &ps = ss.push;
    if (ss.n == 0) return not_created(h);
    if (!ps.planned) return fail(h, MFX_ERR_STATE, "mfx_sessions_run: no push is planned (mfx_sessions_plan), or it has run already");
    if (!h->have_window) return fail(h, MFX_ERR_STATE, "set_window has not been called");
    if (r.pcm_total < 0 || (ps.need_pcm && !r.d_pcm) || (ps.total_rows > 0 && !r.d_out)) return fail(h, MFX_ERR_ARG, "invalid argument");
    if (((uintptr_t)r.d_pcm & 3) != 0) return fail(h, MFX_ERR_ARG, "d_pcm must be 4-byte aligned");
    if (ps.max_end > r.pcm_total) return fail(h, MFX_ERR_ARG, "a session's piece extends past the end of the PCM array");
    HIP_TRY(h, hipSetDevice(h->device));
    const int rc = refresh_mel(h);
    if (rc != MFX_OK) return rc;
    r.d_rows = ss.xf.set ? ss.xf.d_y.p : r.d_out;
    if (h->stft) { // (k_sess_stft_mel is the front end: no statics, rows of `width` floats straight to d_rows)
        r.pitch = h->width;
        return MFX_OK;
    }
    // the front end of the shape, as the batch entries choose it, and the pitch batch_run_range gives the statics
    r.aligned = sess_aligned(h);
    r.kind = choose_front(h, r.aligned);
    fill_front(h, r.front, r.aligned);
    // (a normaliser before the deltas: the statics keep the row's pitch, as decide_mode of the batch runner has it)
    const bool compact = compact_statics(r.kind, r.front) && h->l1 > 0 && h->cols <= 16 && !norm_before(h);
    r.pitch = compact ? 16 : h->width;
    if (is_spec_kind(r.kind) && ss.slab_rows == 0)
        return fail(h, MFX_ERR_STATE, "the warp factor moved this shape to the spectrum path: call mfx_sessions_create again");
    return MFX_OK;
}

// ---- stage 2: the descriptors take the run's pitch where the plan left it open; one upload of all lists (SessUpload) from the
// staging buffer that is free
int upload(mfx_handle *h, PushRun &r)
{
    SessState &ss = h->sess;
    Push &ps = ss.push;
    for (SessDesc &d : ps.descs) {
        if (d.src_pitch <= 0) d.src_pitch = r.pitch;
        r.items_max = std::max(r.items_max, sess_gather_items(d, r.pitch, h->cols, ss.xf.set ? h->width : 0));
    }
    if (SessUpload(ps, nullptr, nullptr).bytes > ss.desc_bytes) return fail(h, MFX_ERR_STATE, "session descriptors outgrew their buffer");
    const int b = ss.stage_cur;
    if (ss.stage_used[b]) HIP_TRY(h, hipEventSynchronize(ss.ev_stage[b])); // (the upload before last read this buffer)
    char *st = ss.h_stage[b].p;
    r.up = SessUpload(ps, st, ss.d_desc.p);
    const size_t bytes = r.up.bytes;
    HIP_TRY(h, hipMemcpyAsync(ss.d_desc.p, st, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipEventRecord(ss.ev_stage[b], h->stream));
    ss.stage_used[b] = true;
    ss.stage_cur = b ^ 1;
    return MFX_OK;
}

// ---- stage 3, session rates: the pieces' input (carried tail + the caller's array) -> converted pieces in the scratch, the
// new carry -> the current carry slots
int run_resample(mfx_handle *h, const PushRun &r)
{
    const SessState &ss = h->sess;
    if (ss.push.rtiles.empty()) return MFX_OK;
    SessResampleParams rp{};
    rp.pcm = r.d_pcm, rp.out = ss.rs.d_conv.p, rp.carry = ss.rs.d_carry.p;
    rp.tiles = r.up.rtiles, rp.n_tiles = (int32_t)ss.push.rtiles.size();
    rp.rates = ss.rs.d_rates.p, rp.taps = ss.rs.d_taps.p;
    rp.channels = h->channels;
    rp.lds = ss.rs.lds;
    HIP_TRY(h, launch_sess_resample(rp, h->stream));
    return MFX_OK;
}

// ---- stage 4, gather: carried PCM tail + new samples + carried static rows (+ carried rows y) -> the current slots
int run_gather(mfx_handle *h, const PushRun &r)
{
    const SessState &ss = h->sess;
    SessGatherParams gp{};
    gp.descs = r.up.descs, gp.n_descs = (int32_t)ss.push.descs.size(), gp.items_max = r.items_max;
    gp.narrow = (h->cfg.engine & MFX_ENGINE_SESS_NARROW_LOADS) ? 1 : 0;
    // (a push that converts: the new samples are the converted pieces in the scratch)
    gp.pcm = ss.push.convert ? ss.rs.d_conv.p : r.d_pcm;
    gp.pcm_elems = ss.push.convert ? (int64_t)ss.n * ss.rs.conv_stride * h->channels : r.pcm_total * h->channels;
    gp.slot_pcm = ss.d_pcm.p, gp.slot_elems = (int64_t)2 * ss.n * ss.pcm_stride * h->channels;
    gp.slot_stat = ss.d_stat.p, gp.stat_pitch = r.pitch, gp.cols = h->cols;
    gp.slot_y = ss.xf.d_y.p, gp.y_width = ss.xf.set ? h->width : 0;
    HIP_TRY(h, launch_sess_gather(gp, h->stream));
    return MFX_OK;
}

// ---- stage 5, front end over the push's chunks: statics straight to their rows of the current slots
int run_front(mfx_handle *h, PushRun &r)
{
    const SessState &ss = h->sess;
    const Push &ps = ss.push;
    if (ps.chunks.empty()) return MFX_OK;
    FrontParams &p = r.front;
    p.pcm = ss.d_pcm.p, p.pcm_total = (int64_t)2 * ss.n * ss.pcm_stride * h->channels;
    p.feat = ss.d_stat.p, p.feat_pitch = r.pitch, p.row_limit = (int64_t)2 * ss.n * ss.row_cap;
    // (spectrum kinds: k_melcep_runs / k_plp_runs on the new rows only; a push adds nothing to mfx_profile_read)
    FrontWork w;
    w.h_chunks = ps.chunks.data(), w.d_chunks = r.up.chunks, w.n_chunks = ps.chunks.size();
    w.slab = ss.d_slab.p, w.slab_rows = ss.slab_rows;
    w.tables = &h->own;
    w.runs = r.up.runs, w.run_off = r.up.run_off;
    w.h_runs = ps.runs.data(), w.h_run_off = ps.run_off;
    return launch_front(h, p, r.kind, r.aligned, w);
}

// ---- stages 5 to 8 of an STFT log-mel handle: the frames the push completes, from the current slots' PCM into d_rows -- groups
// of different sessions packed into blocks (k_sess_stft_mel), or under MFX_ENGINE_SESS_STFT_PLAIN k_stft_mel itself, one chunk
// per run of frames of one session (the measurement's comparator; same bits)
int run_stft(mfx_handle *h, const PushRun &r)
{
    const SessState &ss = h->sess;
    const Push &ps = ss.push;
    if (ps.stft.empty()) return MFX_OK;
    if (stft_plain(h)) {
        if (ss.d_stft_max.n < ps.stft.size()) return fail(h, MFX_ERR_STATE, "session chunks outgrew their buffer");
        StftParams sp{};
        sp.pcm = ss.d_pcm.p;
        sp.chunks = r.up.stft, sp.n_chunks = (int32_t)ps.stft.size(), sp.chunk_first = 0;
        sp.tile_rows = h->stft_R;
        sp.core = stft_core(h, r.d_rows, h->width);
        sp.blk_max = ss.d_stft_max.p;
        HIP_TRY(h, launch_stft(sp, h->stream));
        return MFX_OK;
    }
    SessStftParams sp{};
    sp.pcm = ss.d_pcm.p, sp.pcm_elems = (int64_t)2 * ss.n * ss.pcm_stride;
    sp.groups = r.up.stft, sp.n_groups = (int32_t)ps.stft.size(), sp.G = ss.stft_G;
    sp.core = stft_core(h, r.d_rows, h->width);
    HIP_TRY(h, launch_sess_stft(sp, h->stream));
    return MFX_OK;
}

// ---- stages 6 and 8, online normaliser: ahead of the deltas on the new frames' statics in the slots (data = the statics
// slots at the run's pitch), behind them on the rows the push completes (data = d_rows at `width`)
int run_onorm(mfx_handle *h, const PushRun &r, float *data, int pitch)
{
    const SessState &ss = h->sess;
    if (ss.push.onorm.empty()) return MFX_OK;
    OnormSessParams op{};
    op.Wn = spk_wn(h);
    op.window = ss.on.window, op.cvn = h->cfg.norm == MFX_NORM_CVN ? 1 : 0, op.prior_frames = ss.on.prior_frames;
    op.prior_count = ss.on.prior_count, op.prior_acc = ss.on.d_prior.p;
    op.descs = r.up.onorm, op.n_descs = (int32_t)ss.push.onorm.size();
    op.state = ss.on.d_state.p, op.ring = ss.on.d_ring.p;
    op.data = data, op.pitch = pitch;
    HIP_TRY(h, launch_onorm_sess(op, h->stream));
    return MFX_OK;
}

// ---- stage 7, delta: the rows every session's push completes, into d_rows (l1 == 0: the copy form)
int run_delta(mfx_handle *h, const PushRun &r)
{
    const SessState &ss = h->sess;
    if (ss.push.segs.empty()) return MFX_OK;
    DeltaParams dp;
    fill_delta(h, dp);
    dp.src = ss.d_stat.p, dp.src_pitch = r.pitch, dp.out = r.d_rows;
    dp.segs = r.up.segs, dp.n_segs = (int32_t)ss.push.segs.size(), dp.tiles_per_seg_max = ss.push.tiles_max;
    HIP_TRY(h, launch_delta(dp, h->stream));
    return MFX_OK;
}

// ---- stage 9, session transform: the rows y in the slots -> the caller's array, [total_rows][out_dim]
int run_xform(mfx_handle *h, const PushRun &r)
{
    const SessState &ss = h->sess;
    const Push &ps = ss.push;
    if (!ps.xsegs.empty()) { // k_splice_affine itself, one segment per session (the measurement's comparator; same bits)
        XformParams pp;
        fill_xform_shape(h, pp, h->width, ss.xf.left, ss.xf.right, ss.xf.out);
        pp.src = ss.xf.d_y.p, pp.out = r.d_out;
        pp.segs = (const Segment *)r.up.xa, pp.n_segs = (int32_t)ps.xsegs.size();
        pp.seg_xf = (const int32_t *)r.up.xb;
        pp.operands = ss.xf.d_ops.p, pp.bias = ss.xf.d_bias.p;
        pp.tiles_per_seg_max = ps.xtiles_max;
        HIP_TRY(h, launch_xform(pp, h->stream));
    } else if (!ps.blocks.empty()) {
        SessXformParams xp;
        fill_xform_shape(h, xp, h->width, ss.xf.left, ss.xf.right, ss.xf.out);
        xp.src = ss.xf.d_y.p, xp.out = r.d_out;
        xp.groups = (const SessXfGroup *)r.up.xa, xp.blocks = (const SessXfBlock *)r.up.xb;
        xp.n_blocks = (int32_t)ps.blocks.size();
        xp.operands = ss.xf.d_ops.p, xp.bias = ss.xf.d_bias.p;
        xp.tile_rows = 16 * ss.xf.G;
        HIP_TRY(h, launch_sess_xform(xp, h->stream));
    }
    return MFX_OK;
}

// ---- stage 10, once the launches are queued: every piece's session takes its next state; the push is consumed
void commit(mfx_handle *h, const PushRun &r)
{
    SessState &ss = h->sess;
    for (const Piece &pc : ss.push.pieces) {
        SessState::Live &lv = ss.live[pc.id];
        lv = pc.next;
        if (lv.pitch < 0) lv.pitch = r.pitch;
    }
    if (ss.rs.set) { // (what mfx_sessions_converted_read returns)
        ss.rs.last_valid = ss.push.convert;
        if (ss.push.convert) ss.rs.last_off = ss.push.c_off, ss.rs.last_len = ss.push.c_len;
    }
    ss.push.planned = false;
}

} // namespace

extern "C" int mfx_sessions_run_device(mfx_handle *h, const int16_t *d_pcm, int64_t pcm_samples_total, float *d_out)
{
    MFX_DEVICE_ENTRY(h);
    PushRun r{d_pcm, pcm_samples_total, d_out};
    const bool before = norm_before(h);
    int rc = check_run(h, r);
    if (rc != MFX_OK) return rc;
    if (!h->sess.push.descs.empty() || !h->sess.push.rtiles.empty()) { // (neither: nothing to move, compute or deliver)
        if ((rc = upload(h, r)) != MFX_OK || (rc = run_resample(h, r)) != MFX_OK || (rc = run_gather(h, r)) != MFX_OK) return rc;
        if (h->stft) {
            if ((rc = run_stft(h, r)) != MFX_OK || (rc = run_xform(h, r)) != MFX_OK) return rc;
            commit(h, r);
            return MFX_OK;
        }
        if ((rc = run_front(h, r)) != MFX_OK) return rc;
        if (before && (rc = run_onorm(h, r, h->sess.d_stat.p, r.pitch)) != MFX_OK) return rc;
        if ((rc = run_delta(h, r)) != MFX_OK) return rc;
        if (!before && (rc = run_onorm(h, r, r.d_rows, h->width)) != MFX_OK) return rc;
        if ((rc = run_xform(h, r)) != MFX_OK) return rc;
    }
    commit(h, r);
    return MFX_OK;
}

extern "C" int mfx_sessions_run_host(mfx_handle *h, const int16_t *pcm, int64_t pcm_samples_total, float *out)
{
    MFX_DEVICE_ENTRY(h);
    SessState &ss = h->sess;
    if (ss.n == 0) return not_created(h);
    if (!ss.push.planned) return fail(h, MFX_ERR_STATE, "mfx_sessions_run: no push is planned (mfx_sessions_plan), or it has run already");
    if (pcm_samples_total < 0 || (pcm_samples_total > 0 && !pcm) || (ss.push.total_rows > 0 && !out)) return fail(h, MFX_ERR_ARG, "invalid argument");
    HIP_TRY(h, hipSetDevice(h->device));
    // device copies of the caller's buffers, grown on demand (this entry may allocate; mfx_sessions_run_device never does)
    const size_t n_in = (size_t)pcm_samples_total * h->channels, n_out = (size_t)ss.push.total_rows * sess_out_width(h);
    if (ss.d_host_pcm.n < n_in + 8 || ss.d_host_out.n < n_out + 4) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (ss.d_host_pcm.n < n_in + 8) HIP_TRY(h, ss.d_host_pcm.alloc(n_in + 8));
        if (ss.d_host_out.n < n_out + 4) HIP_TRY(h, ss.d_host_out.alloc(n_out + 4));
    }
    if (n_in > 0) HIP_TRY(h, hipMemcpyAsync(ss.d_host_pcm.p, pcm, n_in * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
    const int64_t rows = ss.push.total_rows;
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
    std::vector<SessXfCut> gp;
    std::vector<SessXfPack> bl;
    pack_sess_xform_groups(n_out, xf, n, G, gp, bl);
    if (n_blocks) *n_blocks = (int32_t)bl.size();
    if (groups) {
        if ((size_t)groups_cap < gp.size()) return MFX_ERR_ARG;
        for (size_t g = 0; g < gp.size(); ++g) groups[3 * g] = gp[g].piece, groups[3 * g + 1] = gp[g].r0, groups[3 * g + 2] = gp[g].rows;
    }
    if (blocks) {
        if ((size_t)blocks_cap < bl.size()) return MFX_ERR_ARG;
        for (size_t k = 0; k < bl.size(); ++k) blocks[3 * k] = bl[k].g0, blocks[3 * k + 1] = bl[k].ng, blocks[3 * k + 2] = bl[k].xf;
    }
    return (int32_t)gp.size();
}

extern "C" int64_t mfx_host_session_resample_step(int32_t in_hz, int32_t out_hz, int32_t zeros, float rolloff, int64_t state[2], int64_t length,
                                                  int32_t final_flag, int32_t *carry_in, int32_t *carry_out)
{
    ResampleShape sh;
    if (resample_shape(in_hz, out_hz, zeros, rolloff, sh) != 0 || !state || state[0] < 0 || state[1] < 0 || length < 0) return MFX_ERR_ARG;
    if (state[0] > (INT64_MAX / 4096 - length) / 2) return MFX_ERR_ARG; // (N L stays inside int64)
    const bool pass = in_hz == out_hz;
    if (state[1] > (pass ? state[0] : (state[0] * sh.L + sh.M - 1) / sh.M)) return MFX_ERR_ARG; // (more outputs than the stream has)
    SessionResampleStep st;
    const int64_t n = session_resample_step(pass ? 1 : sh.L, pass ? 1 : sh.M, pass ? 0 : sh.Wh, state[0], state[1], length, final_flag != 0, st);
    if (carry_in) *carry_in = st.carry_in;
    if (carry_out) *carry_out = st.carry_out;
    return n;
}

extern "C" int32_t mfx_host_session_stft_step(int32_t dft_size, int32_t shift, int64_t state[2], int64_t length, int32_t final_flag,
                                              int32_t *carry_in, int32_t *carry_out)
{
    if (dft_size < 32 || dft_size > 512 || (dft_size & 1) || shift < 1 || shift > dft_size) return MFX_ERR_ARG;
    if (!state || state[0] < 0 || state[1] < 0 || length < 0 || length > (1 << 24) || state[0] > INT64_MAX / 2) return MFX_ERR_ARG;
    if (state[1] > stft_frame_count(state[0], dft_size, shift)) return MFX_ERR_ARG; // (more rows than the stream has frames)
    // (fewer rows than an open stream of n samples has delivered: no slot carries N + S samples or more)
    if (state[0] - std::max<int64_t>(state[1] * shift - dft_size / 2, 0) >= dft_size + shift) return MFX_ERR_ARG;
    SessionStftStep st;
    const int32_t n_out = session_stft_step(dft_size, shift, state[0], state[1], length, final_flag != 0, st);
    if (carry_in) *carry_in = st.carry_in;
    if (carry_out) *carry_out = st.carry_out;
    return n_out;
}

extern "C" int64_t mfx_host_sess_stft_lds_bytes(int32_t dft_size, int32_t shift, int32_t num_banks, int32_t *groups)
{
    if (stft_form(dft_size) != StftForm::Matrix || !stft_shape_ok(dft_size, shift, num_banks)) return MFX_ERR_ARG;
    const int G = groups && *groups > 0 ? *groups : sess_stft_groups(dft_size, shift, num_banks);
    if (G != 1 && G != 2 && G != 4) return MFX_ERR_ARG;
    if (groups) *groups = G;
    return (int64_t)sess_stft_lds_bytes(dft_size, shift, num_banks, G);
}
