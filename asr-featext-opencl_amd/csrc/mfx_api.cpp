// mfx_api.cpp -- the C ABI of include/mfx.h, entry file: handle lifetime and tables, THE dispatch rule (choose_front),
// profiling, the test taps.  The streaming interface is mfx_stream.cpp, the batch interface mfx_batch*.cpp; the handle they
// share is mfx_handle.h.
//
// All arithmetic on samples and features happens in the HIP kernels of mfx_front*.hip / mfx_tail.hip / mfx_plp.hip, all
// arithmetic on tables in mfx_tables.cpp.  There is deliberately no CPU compute path in these three files.
#include "mfx_handle.h"

#include <cmath>
#include <cstring>
#include <memory>

using namespace mfx;

namespace {

// k_melcep parameters that do not depend on the caller, for the tables `t` (the handle's own or the sweep's)
void fill_melcep(const mfx_handle *h, const CepTables &t, MelcepParams &mp)
{
    std::memset(&mp, 0, sizeof(mp));
    mp.spec_pitch = h->spec_pitch;
    mp.fft_size = h->W2;
    mp.mel_w = t.mel_w.p;
    mp.mel_beg = t.mel_beg.p;
    mp.mel = t.plan64.tables_arg();
    mp.mag_floats = std::max(h->W2, (h->spec_pitch + 3) & ~3);
    mp.dct = h->ceps > 0 ? h->d_dct.p : nullptr;
    mp.dct_b4 = h->ceps > 0 ? h->d_dct_b4.p : nullptr;
    mp.dct_ksteps = h->dct_ksteps;
    mp.num_banks = h->nb;
    mp.dct_len = h->dl;
    mp.cols = h->fcols;
    mp.mel_w_stride = (int64_t)2 * h->W2;
    mp.mel_beg_stride = h->nb + 2;
}

// k_plp parameters that do not depend on the caller (the PLP twin of fill_melcep)
void fill_plp(const mfx_handle *h, const CepTables &t, PlpParams &pp)
{
    std::memset(&pp, 0, sizeof(pp));
    pp.spec_pitch = h->spec_pitch;
    pp.fft_size = h->W2;
    pp.num_banks = h->nb;
    pp.lpc_order = h->lpc;
    pp.ceps_len = h->ceps;
    pp.want_c0 = h->cfg.want_c0 ? 1 : 0;
    pp.cols = h->cols;
    pp.mel = t.plan64.tables_arg();
    pp.mag_floats = std::max(h->W2, (h->spec_pitch + 3) & ~3);
    pp.eql = t.eql.p;
    pp.idft = h->d_plp_idft.p;
    pp.lift = h->d_plp_lift.p;
}

} // namespace

// (Re)build `t` for the n warp factors `alphas` (nothing to do when it holds them already): mel tables, 64-lane plans
// (MelPlanBuf pads them to one row stride) and PLP's equal-loudness weights.  first (optional) receives table 0's mel table.
int build_cep_tables(mfx_handle *h, const float *alphas, int n, CepTables &t, MelTable *first)
{
    if (t.holds(alphas, n)) return MFX_OK;
    t.alphas.clear(); // (until every table below is in place)
    t.plan64.ok = false;
    const size_t wstride = (size_t)2 * h->W2, bstride = (size_t)h->nb + 2;
    std::vector<float> w(wstride * n), eql_all;
    std::vector<int32_t> b(bstride * n);
    std::vector<MelPlan> plans((size_t)n);
    for (int a = 0; a < n; ++a) {
        MelTable mt;
        build_mel_table(h->nb, h->W2, h->cfg.sample_rate, h->cfg.low_freq, h->cfg.high_freq, alphas[a], mt);
        // every filter edge must address a computed bin
        for (int v : mt.beg)
            if (v < 0 || v > h->W2 / 2) return fail(h, MFX_ERR_CONFIG, "mel filter edge outside [0, fft_size/2]");
        // (the kernels' magnitude buffers hold W2 floats: bins 0 .. W2/2, finite words beyond)
        if (!build_mel_plan(mt, h->nb, h->W2, /*max_read_bin=*/h->W2 - 1, /*lanes=*/64, /*align=*/2, plans[a]))
            return fail(h, MFX_ERR_CONFIG, "mel filterbank does not fit the kernels' lane plan (more than 512 filters?)");
        std::copy(mt.weights.begin(), mt.weights.end(), w.begin() + wstride * a);
        std::copy(mt.beg.begin(), mt.beg.end(), b.begin() + bstride * a);
        if (h->plp) {
            std::vector<float> eql, idft;
            build_plp_tables(h->nb, h->cfg.sample_rate, h->cfg.low_freq, h->cfg.high_freq, alphas[a], h->lpc, eql, idft);
            eql_all.insert(eql_all.end(), eql.begin(), eql.end());
        }
        if (a == 0 && first) *first = std::move(mt);
    }
    t.plan64.shape(plans.data(), n);
    {   // k_melcep / k_plp stage the weight rows (one per filter-carrying lane) + one wave's buffers in LDS.  rows x row
        // stride is at most ~4 x W2 floats for the reference's triangular banks, so every transform up to 4096 points fits
        // whatever the filter count (4096 points, 48 kHz, 20 filters: 20 rows of 600 floats = 48 KB); 8192 points and more
        // with few, wide filters do not: refuse here (a CONFIG error at the call, not a launch failure later)
        MelcepParams mp;
        fill_melcep(h, t, mp);
        if (melcep_lds_bytes(mp, 1) > kLdsCap)
            return fail(h, MFX_ERR_CONFIG, "mel filterbank does not fit the kernels' LDS (very wide filters on a long transform)");
        if (h->plp) {
            PlpParams pp;
            fill_plp(h, t, pp);
            if (plp_lds_bytes(pp, 1) > kLdsCap) return fail(h, MFX_ERR_CONFIG, "mel filterbank does not fit the PLP kernel's LDS");
        }
    }
    if (!h->planning) HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, h->upload(t.mel_w, w));
    HIP_TRY(h, h->upload(t.mel_beg, b));
    if (h->plp) HIP_TRY(h, h->upload(t.eql, eql_all));
    if (const int rc = t.plan64.set(h, plans.data(), n); rc != MFX_OK) return rc;
    t.alphas.assign(alphas, alphas + n);
    return MFX_OK;
}

// rebuild the tables of the handle's alpha if needed (the reference re-derives them on every apply(), mfcccpu.cpp:194; here
// only when alpha actually changed).  The 64-lane plan serves every configuration (k_melcep / k_plp for the streaming
// apply(), sweeps and the spectrum path of the batch entry; k_front_reg / k_front_wave fused); the fused front ends'
// own lane plans are derived here too.
int refresh_mel(mfx_handle *h)
{
    if (h->stft || h->kaldi) return MFX_OK; // (its one table does not depend on alpha)
    if (h->own.holds(&h->alpha, 1)) return MFX_OK;
    h->plan16.ok = h->plan32.ok = false;
    MelTable t;
    const int rc = build_cep_tables(h, &h->alpha, 1, h->own, &t);
    if (rc != MFX_OK) return rc;
    // the fused front ends' own plans: build -> set -> the kernel's LDS sum on a fill_front()ed probe decides `ok`
    auto build_set = [&](MelPlanBuf &buf, int lanes, int align, int max_read_bin) {
        MelPlan plan;
        return build_mel_plan(t, h->nb, h->W2, max_read_bin, lanes, align, plan) ? buf.set(h, &plan, 1) : (int)MFX_OK;
    };
    FrontParams probe;
    // the 16-lane plan of k_front512, or of k_front1024 (starts at multiples of 4 bins; bins up to 527 may be read (times zero
    // weights): the slot keeps 264 words for each of the even / odd arrays)
    if (h->fast512 || h->fast1024) {
        if (const int e = build_set(h->plan16, 16, h->fast512 ? 2 : 4, h->fast512 ? 511 - 32 : 527); e != MFX_OK) return e;
        fill_front(h, probe);
        h->plan16.ok = h->plan16.ok && (h->fast512 ? front512_lds_bytes(probe) : front1024_lds_bytes(probe)) <= kLdsCap;
    }
    if (h->fast2048) { // k_front2048 walks the filters on the 32 lanes of each of a wave's two frames
        if (const int e = build_set(h->plan32, 32, 2, 1039); e != MFX_OK) return e;
        fill_front(h, probe);
        h->plan32.ok = h->plan32.ok && front2048_lds_bytes(probe) <= kLdsCap;
    }
    return MFX_OK;
}

void fill_front(const mfx_handle *h, FrontParams &p) { fill_front(h, p, h->batch.aligned); }

// (aligned: every chunk of the launch starts on an even sample -- the batch plan's flag, or the session slots' layout)
void fill_front(const mfx_handle *h, FrontParams &p, bool aligned)
{
    std::memset(&p, 0, sizeof(p));
    p.channels = h->channels;
    p.pair_ok = (h->channels == 1 && (h->S % 2) == 0 && (h->W % 2) == 0 && aligned) ? 1 : 0;
    p.window_size = h->W;
    p.shift = h->S;
    p.fft_size = h->W2;
    p.window = h->d_window.p;
    p.winpair = h->d_winpair.p;
    p.win1024o = h->d_win1024o.p;
    p.twid_pass = h->d_twid_pass.p;
    p.twid_half = h->d_twid_half.p;
    p.twid_reg = h->d_twid_reg.p;
    p.twid_split = h->d_twid_split.p;
    p.mel_w = h->own.mel_w.p;
    p.mel_beg = h->own.mel_beg.p;
    p.dct = h->ceps > 0 ? h->d_dct.p : nullptr;
    p.num_banks = h->nb;
    p.dct_len = h->dl;
    p.cols = h->fcols;
    p.scale = 0.5f / (float)h->W2;
    p.mel16 = h->plan16.arg();
    p.dct_t = h->d_dct_t.p;
    p.dct_mode = (h->ceps > 0 && h->fcols <= 16 && h->nb <= 40) ? 1 : 0; // DCT on the matrix pipe
    p.mel64 = h->own.plan64.arg();
    p.mel32 = h->plan32.arg();
    p.dct_b = h->ceps > 0 ? h->d_dct_b.p : nullptr;
    p.stuff = h->stuff256 ? 512 / h->W2 : 0;
    p.dct_b4 = h->ceps > 0 ? h->d_dct_b4.p : nullptr;
    p.dct_b4s = (h->ceps > 0 && h->dct_split) ? h->d_dct_b4s.p : nullptr;
    p.dct_split = h->ceps > 0 ? h->dct_split : 0;
    p.dct_tiles = h->dct_tiles;
    p.dct_ksteps = h->dct_ksteps;
    p.dct_stride = h->dct_stride;
    p.nb_pad = h->nb_pad > 0 ? h->nb_pad : ((h->nb + 3) & ~3);
}

// k_traps parameters that do not depend on the caller
void fill_traps(const mfx_handle *h, TrapsParams &p)
{
    std::memset(&p, 0, sizeof(p));
    p.num_banks = h->nb;
    p.L = h->traps_L;
    p.K = h->traps_K;
    p.valu = (h->cfg.engine & MFX_ENGINE_TRAPS_VALU) ? 1 : 0;
    p.operands = h->d_traps_b.p;
}

namespace {

int prof_collect(mfx_handle *h)
{
    if (h->prof.used == 0) return MFX_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < h->prof.used; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->prof.events[i].first, h->prof.events[i].second) == hipSuccess) {
            h->prof.ms += ms;
            ++h->prof.launches;
        }
    }
    h->prof.used = 0;
    return MFX_OK;
}

} // namespace

// ---- normalisation helper: stats (unless reused) + apply over one column group
// groups > 1: the column groups g * cols (g < groups) each with statistics at stats + g * group_stats_stride
int run_norm(mfx_handle *h, hipStream_t stream, float *data, int pitch, const Segment *segs, int n_segs, const Segment *seg0,
             float *stats, bool use_last, int max_rows, int groups, size_t group_stats_stride)
{
    NormParams np{};
    np.max_rows = max_rows;
    const size_t need = norm_partial_doubles(seg0 ? 1 : n_segs, max_rows, h->cols);
    if (need > h->d_norm_partial.n) { // (sized at create / plan time for the usual shapes: not reached in a timed loop)
        HIP_TRY(h, hipStreamSynchronize(stream));
        HIP_TRY(h, h->d_norm_partial.alloc(need));
    }
    np.partial = h->d_norm_partial.p;
    np.data = data;
    np.pitch = pitch;
    np.col0 = 0;
    np.cols = h->cols;
    np.segs = segs;
    np.n_segs = n_segs;
    np.row_off = 0;
    np.norm_type = h->cfg.norm;
    np.stats = stats;
    if (seg0) {
        np.inline_seg = 1;
        np.seg0 = *seg0;
        np.n_segs = 1;
    }
    if (!use_last && !(h->cfg.engine & MFX_ENGINE_NORM_TWO_KERNELS) && norm_fused_fits(max_rows, h->cols)) {
        np.groups = groups;
        np.group_stats_stride = (int64_t)group_stats_stride;
        HIP_TRY(h, launch_norm_fused(np, stream)); // short segments: one read of the rows, ONE launch for all groups
        return MFX_OK;
    }
    for (int g = 0; g < groups; ++g) {
        np.col0 = g * h->cols;
        np.stats = stats + (size_t)g * group_stats_stride;
        if (!use_last) HIP_TRY(h, launch_norm_stats(np, stream));
        HIP_TRY(h, launch_norm_apply(np, stream));
    }
    return MFX_OK;
}

// filterbank + log + DCT (k_melcep), or PLP (k_plp), of n_rows magnitude rows at `spec` with each of the n_tables tables of
// `t`; table a writes feat + a * feat_table_stride.  r_out: PLP's autocorrelation tap (table 0), or nullptr.
int launch_cepstra(mfx_handle *h, const CepTables &t, const float *spec, int64_t n_rows, float *feat, int feat_pitch,
                   int n_tables, int64_t feat_table_stride, float *r_out, hipStream_t stream)
{
    if (h->plp) {
        PlpParams pp;
        fill_plp(h, t, pp);
        pp.spec = spec;
        pp.n_rows = n_rows;
        pp.feat = feat;
        pp.feat_pitch = feat_pitch;
        pp.n_tables = n_tables;
        pp.feat_table_stride = feat_table_stride;
        pp.r_out = r_out;
        HIP_TRY(h, launch_plp(pp, stream));
    } else {
        MelcepParams mp;
        fill_melcep(h, t, mp);
        mp.spec = spec;
        mp.n_rows = n_rows;
        mp.feat = feat;
        mp.feat_pitch = feat_pitch;
        mp.n_tables = n_tables;
        mp.feat_table_stride = feat_table_stride;
        HIP_TRY(h, launch_melcep(mp, stream));
    }
    return MFX_OK;
}

int launch_cepstra_runs(mfx_handle *h, const CepTables &t, const float *spec, float *feat, int feat_pitch, const RowRuns &rr,
                        const int32_t *h_off, const int64_t *h_runs, hipStream_t stream)
{
    const int n_tables = (int)t.alphas.size();
    if (h->plp) {
        PlpParams pp;
        fill_plp(h, t, pp);
        pp.spec = spec;
        pp.feat = feat;
        pp.feat_pitch = feat_pitch;
        pp.n_tables = n_tables;
        HIP_TRY(h, launch_plp_runs(pp, rr, h_off, h_runs, stream));
    } else {
        MelcepParams mp;
        fill_melcep(h, t, mp);
        mp.spec = spec;
        mp.feat = feat;
        mp.feat_pitch = feat_pitch;
        mp.n_tables = n_tables;
        HIP_TRY(h, launch_melcep_runs(mp, rr, h_off, h_runs, stream));
    }
    return MFX_OK;
}

// ------------------------------------------------------------------------------------------------
// lifetime
// ------------------------------------------------------------------------------------------------

extern "C" int mfx_abi_version(void) { return MFX_ABI_VERSION; }
extern "C" int mfx_method_supported(int32_t method)
{
    return method == MFX_METHOD_MFCC || method == MFX_METHOD_PLP || method == MFX_METHOD_TRAPS || method == MFX_METHOD_STFT_LOGMEL ||
                   method == MFX_METHOD_KALDI
               ? 1
               : 0;
}

extern "C" const char *mfx_status_string(int status)
{
    switch (status) {
    case MFX_OK: return "ok";
    case MFX_ERR_BUFFER_TOO_SMALL: return kMsgBuffer;
    case MFX_ERR_WINDOW_COUNT: return kMsgWindow;
    case MFX_ERR_PROCESSED: return kMsgProcessed;
    case MFX_ERR_WINDOW_HIGH: return kMsgHigh;
    case MFX_ERR_CONFIG: return "invalid configuration";
    case MFX_ERR_DEVICE: return "HIP device error";
    case MFX_ERR_ARG: return "invalid argument";
    case MFX_ERR_STATE: return "call out of sequence";
    default: return "unknown status";
    }
}

extern "C" const char *mfx_last_error(const mfx_handle *h) { return h ? h->err.c_str() : "null handle"; }

extern "C" void mfx_destroy(mfx_handle *h)
{
    if (!h) return;
    if (!h->planning) { // (a planning handle has no device behind it)
        (void)hipSetDevice(h->device);
        for (hipStream_t s : {h->stream, h->batch.ov.stream2, h->batch.host.stream_up, h->batch.host.stream_dn})
            if (s) (void)hipStreamSynchronize(s);
    }
    delete h; // ~mfx_handle, then the buffers free themselves
}

namespace {
int create_impl(const mfx_config *cfg, int hip_device, bool planning, mfx_handle **out, int kaldi_flags = 0, float kaldi_energy_floor = 0.f);
}

extern "C" int mfx_create(const mfx_config *cfg, int hip_device, mfx_handle **out) { return create_impl(cfg, hip_device, false, out); }

/* A planning handle: see mfx_handle::planning.  No device is touched; only mfx_dominant_kernel_name, the geometry accessors
 * (mfx_get_output_data_width, mfx_get_input_buffer_size, mfx_estimated_window_count, mfx_max_frames_out, mfx_fft_size),
 * mfx_last_error and mfx_destroy are meaningful on it. */
extern "C" int mfx_plan_create(const mfx_config *cfg, mfx_handle **out) { return create_impl(cfg, -1, true, out); }

/* the two with the options of a Kaldi handle (include/mfx.h, method 7, "Options") */
extern "C" int mfx_create_kaldi(const mfx_config *cfg, int32_t kaldi_flags, float kaldi_energy_floor, int hip_device, mfx_handle **out)
{
    if (cfg && out && cfg->method != MFX_METHOD_KALDI) return *out = nullptr, MFX_ERR_CONFIG;
    return create_impl(cfg, hip_device, false, out, kaldi_flags, kaldi_energy_floor);
}
extern "C" int mfx_plan_create_kaldi(const mfx_config *cfg, int32_t kaldi_flags, float kaldi_energy_floor, mfx_handle **out)
{
    if (cfg && out && cfg->method != MFX_METHOD_KALDI) return *out = nullptr, MFX_ERR_CONFIG;
    return create_impl(cfg, -1, true, out, kaldi_flags, kaldi_energy_floor);
}

namespace {
struct HandleDeleter {
    void operator()(mfx_handle *h) const { mfx_destroy(h); }
};

// the limits of an STFT log-mel handle (include/mfx.h): everything sized from N, S and M fits the kernel's LDS by them
bool stft_config_ok(const mfx_config *cfg)
{
    const int N = cfg->window_size;
    if (!stft_shape_ok(N, cfg->shift, cfg->num_banks) || (cfg->fft_size != 0 && cfg->fft_size != N)) return false;
    if (!(cfg->low_freq >= 0.f) || !(cfg->low_freq < cfg->high_freq) || !(cfg->high_freq <= cfg->sample_rate / 2)) return false;
    if (cfg->ceps_len != 0 || cfg->want_c0 != 0 || cfg->dyn != MFX_DYN_NONE || cfg->norm != MFX_NORM_NONE || cfg->channels > 1) return false;
    if (cfg->logmel_post < MFX_LOGMEL_WHISPER || cfg->logmel_post > MFX_LOGMEL_LN) return false;
    return true;
}

// the rest of mfx_create for an STFT log-mel handle: geometry, the Slaney table, the LDS check; the basis waits for the window
int create_stft(mfx_handle *h, bool planning, std::unique_ptr<mfx_handle, HandleDeleter> &owner, mfx_handle **out)
{
    const mfx_config &cfg = h->cfg;
    h->W2 = h->W;
    h->input_window_limit = estimated_window_count_f32(cfg.input_buffer_size, h->W, h->S);
    h->input_buffer_size = h->input_window_limit * h->S + h->W - h->S;
    h->window_limit = h->input_window_limit + 2;
    if (h->input_window_limit <= 0) return MFX_ERR_CONFIG;
    h->cap_rows = h->window_limit + h->W / h->S + 4;
    h->spec_pitch = ((h->W2 / 2 + 1) + 3) & ~3;
    h->stft_form = stft_form(h->W);
    // (the matrix form: 16 frames fit for every shape inside the limits, 512 / 512 / 128 takes 74 KB then; the FFT form: 4 do,
    // 2048 / 2048 / 128 takes 104 KB then)
    h->stft_R = stft_tile_rows(h->W, h->S, h->nb);
    if (h->stft_R == 0) return MFX_ERR_CONFIG;
    if (!planning) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) h->num_cus = prop.multiProcessorCount;
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return MFX_ERR_DEVICE;
        h->own_stream = true;
    }
    std::vector<float> w;
    std::vector<int32_t> meta;
    build_slaney_spans(h->nb, h->W, cfg.sample_rate, cfg.low_freq, cfg.high_freq, w, meta);
    if (h->upload(h->d_span_melw, w) != hipSuccess || h->upload(h->d_span_mel, meta) != hipSuccess ||
        h->alloc(h->st.d_stats, (size_t)3 * 2 * h->cols) != hipSuccess)
        return MFX_ERR_DEVICE;
    *out = owner.release();
    return MFX_OK;
}

// the limits of a Kaldi handle (include/mfx.h): everything sized from W, S, M and C fits the kernel's LDS by them
bool kaldi_config_ok(const mfx_config *cfg, int kaldi_flags, float kaldi_energy_floor)
{
    const int W = cfg->window_size;
    if (!kaldi_shape_ok(W, cfg->shift, cfg->num_banks, cfg->ceps_len) || (cfg->fft_size != 0 && cfg->fft_size != kaldi_fft_size(W))) return false;
    if (!kaldi_freqs_ok(cfg->sample_rate, cfg->low_freq, cfg->high_freq)) return false;
    if (cfg->want_c0 != 0 || cfg->channels > 1 || !(cfg->lift_coef >= 0.f) || !std::isfinite(cfg->lift_coef)) return false;
    // the options: known bits, the windowed energy only with the energy column, a floor Kaldi's log can take
    if (!kaldi_flags_ok(kaldi_flags) || !(kaldi_energy_floor >= 0.f) || !std::isfinite(kaldi_energy_floor)) return false;
    return kaldi_lds_bytes(W, cfg->shift, cfg->num_banks, cfg->ceps_len, kaldi_flags) <= kLdsCap;
}

// the rest of mfx_create for a Kaldi handle: geometry, the mel table and G, what the normalisers of both interfaces share; the
// window and the FFT tables wait for mfx_set_window
int create_kaldi(mfx_handle *h, bool planning, std::unique_ptr<mfx_handle, HandleDeleter> &owner, mfx_handle **out)
{
    const mfx_config &cfg = h->cfg;
    h->W2 = kaldi_fft_size(h->W);
    h->input_window_limit = estimated_window_count_f32(cfg.input_buffer_size, h->W, h->S);
    h->input_buffer_size = h->input_window_limit * h->S + h->W - h->S;
    h->window_limit = h->input_window_limit + 2 + (cfg.dyn != MFX_DYN_NONE ? 3 * h->D : 0);
    if (h->input_window_limit <= 0) return MFX_ERR_CONFIG;
    h->cap_rows = h->window_limit + h->W / h->S + 4;
    h->spec_pitch = ((h->W2 / 2 + 1) + 3) & ~3;
    if (!planning) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) h->num_cus = prop.multiProcessorCount;
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return MFX_ERR_DEVICE;
        h->own_stream = true;
    }
    double high = 0.0;
    (void)kaldi_freqs_ok(cfg.sample_rate, cfg.low_freq, cfg.high_freq, &high);
    std::vector<float> w, gt;
    std::vector<int32_t> meta;
    build_kaldi_spans(h->nb, h->W2, cfg.sample_rate, cfg.low_freq, high, w, meta);
    if (w.size() > (size_t)h->W2) return MFX_ERR_CONFIG; // (a bin lies in two bands at most: the kernel keeps N weights in LDS)
    if (h->ceps > 0) { // G [C][M] -> [M][C]: the cepstra's threads read one band's row together
        std::vector<float> g((size_t)h->ceps * h->nb);
        build_kaldi_dct(h->nb, h->ceps, cfg.lift_coef, g.data());
        gt.resize(g.size());
        for (int i = 0; i < h->ceps; ++i)
            for (int m = 0; m < h->nb; ++m) gt[(size_t)m * h->ceps + i] = g[(size_t)i * h->nb + m];
    }
    if (h->upload(h->d_span_melw, w) != hipSuccess || h->upload(h->d_span_mel, meta) != hipSuccess || h->upload(h->d_kaldi_dct_t, gt) != hipSuccess ||
        h->alloc(h->st.d_stats, (size_t)3 * 2 * h->cols) != hipSuccess)
        return MFX_ERR_DEVICE;
    *out = owner.release();
    return MFX_OK;
}

int create_impl(const mfx_config *cfg, int hip_device, bool planning, mfx_handle **out, int kaldi_flags, float kaldi_energy_floor)
{
    if (!cfg || !out) return MFX_ERR_ARG;
    *out = nullptr;
    if (cfg->window_size <= 0 || cfg->shift <= 0 || cfg->num_banks <= 0 || cfg->ceps_len < 0 ||
        cfg->sample_rate <= 0 || cfg->norm < 0 || cfg->norm > 3 || cfg->dyn < 0 || cfg->dyn > 2 ||
        cfg->channels < 0 || cfg->channels > 2)
        return MFX_ERR_CONFIG;
    const bool kaldi = cfg->method == MFX_METHOD_KALDI; // (its lifter Q = 0 means none)
    if (cfg->ceps_len > 0 && cfg->lift_coef == 0.f && !kaldi) return MFX_ERR_CONFIG; // reference divides by lift_coef
    if (cfg->dyn != MFX_DYN_NONE && cfg->delta_l1 <= 0) return MFX_ERR_CONFIG;
    if (cfg->dyn == MFX_DYN_ACC && cfg->delta_l2 <= 0) return MFX_ERR_CONFIG;
    if (!mfx_method_supported(cfg->method)) return MFX_ERR_CONFIG;
    if (cfg->method == MFX_METHOD_PLP) { // PLP has no log-energy form; the recursion runs in registers up to kPlpMaxOrder
        const int p = cfg->lpc_order == 0 ? 8 : cfg->lpc_order;
        if (cfg->ceps_len <= 0 || cfg->lpc_order < 0 || p > std::min(kPlpMaxOrder, (int)cfg->num_banks)) return MFX_ERR_CONFIG;
    }
    const bool traps = cfg->method == MFX_METHOD_TRAPS;
    const int traps_L = cfg->traps_len == 0 ? 31 : cfg->traps_len, traps_K = cfg->traps_dct_len == 0 ? 10 : cfg->traps_dct_len;
    if (traps) {
        // the log-energy form feeds it; the output row holds num_banks * K statics, and 256 columns is what the normaliser's
        // statistics kernels take (k_norm_stats / k_norm_seg: one thread per column of a 256-thread block)
        if (cfg->ceps_len != 0 || cfg->want_c0 != 0) return MFX_ERR_CONFIG;
        if (cfg->traps_len < 0 || !(traps_L & 1) || traps_L < 3 || traps_L > 101) return MFX_ERR_CONFIG;
        if (cfg->traps_dct_len < 0 || traps_K > 32 || traps_K > traps_L) return MFX_ERR_CONFIG;
        if ((int64_t)cfg->num_banks * traps_K > 256) return MFX_ERR_CONFIG;
    }
    const bool stft = cfg->method == MFX_METHOD_STFT_LOGMEL;
    if (stft && !stft_config_ok(cfg)) return MFX_ERR_CONFIG;
    if (kaldi && !kaldi_config_ok(cfg, kaldi_flags, kaldi_energy_floor)) return MFX_ERR_CONFIG;

    if (!planning) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hip_device < 0 || hip_device >= ndev)
            return MFX_ERR_DEVICE; // no CPU fallback by design
        if (hipSetDevice(hip_device) != hipSuccess) return MFX_ERR_DEVICE;
    }

    // (every return below destroys the handle, except the last)
    std::unique_ptr<mfx_handle, HandleDeleter> owner(new mfx_handle());
    mfx_handle *h = owner.get();
    h->cfg = *cfg;
    h->device = hip_device;
    h->planning = planning;
    h->W = cfg->window_size;
    h->S = cfg->shift;
    h->nb = cfg->num_banks;
    h->ceps = cfg->ceps_len;
    h->plp = cfg->method == MFX_METHOD_PLP;
    h->lpc = h->plp ? (cfg->lpc_order == 0 ? 8 : cfg->lpc_order) : 0;
    h->l1 = cfg->dyn != MFX_DYN_NONE ? cfg->delta_l1 : 0;
    h->l2 = cfg->dyn == MFX_DYN_ACC ? cfg->delta_l2 : 0;
    h->D = h->l1 + h->l2;
    h->dl = cfg->want_c0 ? cfg->ceps_len + 1 : cfg->ceps_len;
    h->traps = traps;
    h->stft = stft;
    h->kaldi = kaldi;
    if (kaldi) {
        h->kaldi_flags = kaldi_flags;
        if (kaldi_energy_floor > 0.f) h->kaldi_log_floor = (float)std::log((double)kaldi_energy_floor);
    }
    h->traps_L = traps ? traps_L : 0;
    h->traps_K = traps ? traps_K : 0;
    h->fcols = kaldi ? kaldi_static_cols(h->nb, h->ceps, h->kaldi_flags) : h->ceps > 0 ? h->dl : h->nb; // (the energy column of a Kaldi fbank)
    h->cols = traps ? h->nb * traps_K : h->fcols;
    h->width = h->cols * (cfg->dyn == MFX_DYN_ACC ? 3 : cfg->dyn == MFX_DYN_DELTA ? 2 : 1);
    h->channels = cfg->channels == 2 ? 2 : 1;
    if (h->l1 > 0) {
        // the delta stage's LDS holds (R + 2 D) + (R + 2 l2) + R rows (launch_delta: R = 64 rows of 16 floats up to 16 columns,
        // else 32 rows of `cols` floats): an order beyond it is refused here, not by a failed launch.  At 256 columns the
        // limit is l1 = l2 = 10.
        const int64_t R = h->cols <= 16 ? 64 : 32, cw = h->cols <= 16 ? 16 : h->cols;
        const int64_t rows = 3 * R + 2 * ((int64_t)h->l1 + h->l2) + 2 * (int64_t)h->l2;
        if (rows * cw * (int64_t)sizeof(float) > (int64_t)kLdsCap) return MFX_ERR_CONFIG;
    }
    if (stft) return create_stft(h, planning, owner, out);
    if (kaldi) return create_kaldi(h, planning, owner, out);
    h->W2 = (int)ceil_pow2((uint32_t)h->W);
    if (cfg->fft_size != 0) {
        if (cfg->fft_size < h->W || (cfg->fft_size & (cfg->fft_size - 1)) != 0) return MFX_ERR_CONFIG;
        h->W2 = cfg->fft_size;
    }
    if (h->W2 < 64 || h->W2 > 4096) return MFX_ERR_CONFIG;
    // ParamBase ctor (parambase.cpp:4-14)
    h->input_window_limit = estimated_window_count_f32(cfg->input_buffer_size, h->W, h->S);
    h->input_buffer_size = h->input_window_limit * h->S + h->W - h->S;
    // MfccCpu ctor (mfcccpu.cpp:95-103)
    h->window_limit = h->input_window_limit + 2 + (cfg->dyn != MFX_DYN_NONE ? 3 * h->D : 0);
    if (h->input_window_limit <= 0 || h->window_limit <= 0) return MFX_ERR_CONFIG;
    h->spec_pitch = ((h->W2 / 2 + 1) + 3) & ~3;
    h->fast512 = front512_supported(h->W2, h->W, h->nb, h->fcols, h->channels) && !(h->W2 < 512 && (h->cfg.engine & MFX_ENGINE_NO_STUFF256));
    h->stuff256 = h->fast512 && h->W2 < 512; // (256, 128 or 64 points: stuff factor 512 / W2)
    h->fast2048 = !(h->cfg.engine & MFX_ENGINE_NO_FRONT2048) && front2048_supported(h->W2, h->W, h->nb, h->fcols, h->channels);
    h->fast1024 = !(h->cfg.engine & MFX_ENGINE_NO_FRONT1024) &&
                  front1024_supported(h->W2, h->W, h->nb, h->fcols, h->channels, h->ceps);
    {
        hipDeviceProp_t prop;
        if (!planning && hipGetDeviceProperties(&prop, hip_device) == hipSuccess && prop.multiProcessorCount > 0)
            h->num_cus = prop.multiProcessorCount;
        h->fuse.off = (h->cfg.engine & MFX_ENGINE_NO_FUSE_DELTA) != 0;
        h->fuse.enabled = !h->fuse.off && (h->cfg.engine & MFX_ENGINE_FUSE_DELTA) != 0;
        h->fuse.share = (h->cfg.engine & MFX_ENGINE_FUSE_NO_SHARE) ? 0 : (h->cfg.engine & MFX_ENGINE_FUSE_SHARE_ALL) ? 2 : 1;
    }
    // rows of the frame that carry window taps: 32 samples per row, or 16 / 8 / 4 in the zero-stuffed forms
    h->nm16 = h->stuff256 ? (h->W + h->W2 / 16 - 1) / (h->W2 / 16) : (h->W + 31) / 32;

    if (!planning) {
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return MFX_ERR_DEVICE;
        h->own_stream = true;
    }
#define DEV_OK(expr)                                     \
    do {                                                 \
        if ((expr) != hipSuccess) return MFX_ERR_DEVICE; \
    } while (0)

    // ---- constant tables (layouts: mfx_tables.h)
    {
        std::vector<float> t;
        build_twiddles(h->W2 / 2, h->W2 / 2, t); // W_M^k, k < M (radix-4 stages use k, 2k, 3k)
        DEV_OK(h->upload(h->d_twid_half, t));
        build_split_twiddles(h->W2, h->stuff256, t);
        DEV_OK(h->upload(h->d_twid_split, t));
        if (h->W2 >= 1024) { // k_front_reg
            build_reg_pass_twiddles(h->W2, t);
            DEV_OK(h->upload(h->d_twid_reg, t));
        }
        if (h->fast512 || h->fast1024) {
            build_pass256_twiddles(t);
            DEV_OK(h->upload(h->d_twid_pass, t));
        }
        if (h->ceps > 0) {
            std::vector<float> m, ob;
            build_dct_matrix(h->nb, h->ceps, cfg->want_c0 != 0, cfg->lift_coef, m);
            DEV_OK(h->upload(h->d_dct, m));
            h->h_dct = m;
            build_dct_mfma_operands(m, h->nb, h->dl, h->dct_tiles, h->dct_ksteps, ob);
            DEV_OK(h->upload(h->d_dct_b, ob));
            build_dct_mfma_operands4(m, h->nb, h->dl, ob); // the 4x4x1 form: k_front2048, k_front_wave, k_melcep
            DEV_OK(h->upload(h->d_dct_b4, ob));
            h->dct_split = (h->cfg.engine & MFX_ENGINE_NO_DCT_SPLIT) ? 0 : dct_split_mode(h->nb, h->dl);
            if (h->dct_split) {
                build_dct_mfma_operands4_split(m, h->nb, h->dl, ob);
                DEV_OK(h->upload(h->d_dct_b4s, ob));
            }
            if (h->fast512) {
                build_dct_transposed(m, h->nb, h->dl, h->dct_stride, h->nb_pad, ob);
                DEV_OK(h->upload(h->d_dct_t, ob));
            }
        }
    }
    if (h->plp) {
        std::vector<float> eql, idft, lift;
        build_plp_tables(h->nb, cfg->sample_rate, cfg->low_freq, cfg->high_freq, 1.f, h->lpc, eql, idft);
        build_plp_lifter(h->ceps, cfg->lift_coef, lift);
        DEV_OK(h->upload(h->d_plp_idft, idft));
        DEV_OK(h->upload(h->d_plp_lift, lift));
    }
    if (h->traps) {
        std::vector<float> basis, ob;
        build_traps_basis(h->traps_L, h->traps_K, basis);
        int a = 0, b = 0;
        if (h->cfg.engine & MFX_ENGINE_TRAPS_VALU)
            build_traps_valu_operands(basis, h->traps_L, h->traps_K, a, ob);
        else
            build_traps_mfma_operands(basis, h->traps_L, h->traps_K, a, b, ob);
        DEV_OK(h->upload(h->d_traps_b, ob));
        TrapsParams tp;
        fill_traps(h, tp);
        if (traps_tile_rows(tp) == 0) return MFX_ERR_CONFIG;
    }
    if (const int rc = refresh_mel(h); rc != MFX_OK) return rc;

    // ---- streaming buffers (capacity as the reference: segmentercpu.cpp:40-41, mfcccpu.cpp:104-112)
    // The reference sizes these from window_limit alone (segmentercpu.cpp:40-41, mfcccpu.cpp:104-112); a
    // steady-state block can need up to ~W/S more frames and W more samples than that (it writes past
    // its buffers when W - S > 2S or dyn is off), so capacity here carries that slack.
    StreamState &st = h->st;
    h->cap_rows = h->window_limit + h->W / h->S + 4;
    st.carry_capacity = (size_t)h->cap_rows * h->S + 2 * (size_t)h->W;
    const size_t carry_alloc = (st.carry_capacity + h->W2 + 8) & ~(size_t)1;
    // (a TRAPS handle has no streaming entries: no carry, no block buffers)
    for (int i = 0; i < 2 && !h->traps; ++i) {
        DEV_OK(h->alloc(st.d_carry[i], carry_alloc));
        if (!planning) DEV_OK(hipMemset(st.d_carry[i].p, 0, carry_alloc * sizeof(int16_t)));
    }
    DEV_OK(h->alloc(h->d_spec, (size_t)h->cap_rows * h->spec_pitch));
    if (!h->traps) {
        DEV_OK(h->alloc(st.d_src, (size_t)h->cap_rows * h->cols));
        DEV_OK(h->alloc(st.d_blk, (size_t)h->cap_rows * h->width));
    }
    DEV_OK(h->alloc(st.d_stats, (size_t)3 * 2 * h->cols));
    if (h->plp) DEV_OK(h->alloc(st.d_plp_r, (size_t)h->cap_rows * (h->lpc + 1)));
    if (cfg->norm != MFX_NORM_NONE) { // chunk results of the statistics over a long streaming block
        const size_t need = norm_partial_doubles(1, h->cap_rows, h->cols);
        if (need > 0) DEV_OK(h->alloc(h->d_norm_partial, need));
    }
    if (!planning) DEV_OK(hipMemset(st.d_stats.p, 0, (size_t)3 * 2 * h->cols * sizeof(float)));
    {
        // work items of a streaming block: 16 frames, or 4 where a whole block is only a few thousand frames (one 10-s
        // utterance = 62 items of 16 frames would occupy 4 of 256 CUs, every wave running 4 iterations back to back)
        st.chunk_frames = h->cap_rows <= 16384 ? 4 : kChunkFrames;
        const int cf = st.chunk_frames;
        st.n_chunks_max = (h->cap_rows + cf - 1) / cf;
        std::vector<Chunk> ch(st.n_chunks_max);
        for (int i = 0; i < st.n_chunks_max; ++i) {
            ch[i].pcm_off = (int64_t)i * cf * h->S;
            ch[i].out_row = (int64_t)i * cf;
            ch[i].n_frames = cf;
            ch[i].pad = 0;
        }
        DEV_OK(h->upload(st.d_chunks, ch));
    }
    st.host_tail = !(h->cfg.engine & MFX_ENGINE_DMA_SMALL_BLOCKS) && (st.carry_capacity + 8) * sizeof(int16_t) < kSmallBlock;
    // (+ 16 bytes: small blocks are staged at the destination's alignment; host_tail: tail + block, up to the carry capacity)
    const size_t stage_n = (st.host_tail ? st.carry_capacity : (size_t)h->input_buffer_size) + 8;
    if (!planning && !h->traps) DEV_OK(st.h_stage.grow(stage_n, stage_n, h->stream));
#undef DEV_OK

    *out = owner.release();
    return MFX_OK;
}
} // namespace

// ------------------------------------------------------------------------------------------------
// simple accessors
// ------------------------------------------------------------------------------------------------

extern "C" int mfx_get_output_data_width(const mfx_handle *h) { return h ? h->width : MFX_ERR_ARG; }
extern "C" int mfx_get_input_buffer_size(const mfx_handle *h) { return h ? h->input_buffer_size : MFX_ERR_ARG; }
extern "C" int mfx_estimated_window_count(const mfx_handle *h, int32_t samples)
{
    return h ? estimated_window_count_f32(samples, h->W, h->S) : MFX_ERR_ARG;
}
extern "C" int mfx_max_frames_out(const mfx_handle *h) { return h ? h->input_window_limit + h->W / h->S + 3 : MFX_ERR_ARG; }
extern "C" int mfx_fft_size(const mfx_handle *h) { return h ? h->W2 : MFX_ERR_ARG; }

extern "C" int mfx_set_alpha(mfx_handle *h, float alpha)
{
    if (!h) return MFX_ERR_ARG;
    h->alpha = alpha;
    return MFX_OK;
}

extern "C" int mfx_set_stream(mfx_handle *h, void *hip_stream)
{
    MFX_DEVICE_ENTRY(h);
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->stream) HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    h->stream = (hipStream_t)hip_stream;
    h->own_stream = false;
    return MFX_OK;
}

extern "C" int mfx_synchronize(mfx_handle *h)
{
    MFX_DEVICE_ENTRY(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->batch.ov.stream2) HIP_TRY(h, hipStreamSynchronize(h->batch.ov.stream2));
    h->batch.ov.tail_pending[0] = h->batch.ov.tail_pending[1] = false;
    if (h->fuse.d_err.p) { // the fused delta stage reports a wait that ran out (never expected) instead of hanging
        int32_t flag = 0;
        HIP_TRY(h, hipMemcpy(&flag, h->fuse.d_err.p, sizeof(flag), hipMemcpyDeviceToHost));
        if (flag != 0) {
            (void)hipMemset(h->fuse.d_err.p, 0, sizeof(flag));
            return fail(h, MFX_ERR_DEVICE, "fused delta stage gave up waiting for its statics");
        }
    }
    return MFX_OK;
}

extern "C" int mfx_profile_enable(mfx_handle *h, int enable)
{
    MFX_DEVICE_ENTRY(h);
    int rc = prof_collect(h);
    h->prof.on = enable != 0;
    return rc;
}

extern "C" int mfx_profile_read(mfx_handle *h, int32_t *launches, double *kernel_ms, int reset)
{
    MFX_DEVICE_ENTRY(h);
    int rc = prof_collect(h);
    if (rc != MFX_OK) return rc;
    if (launches) *launches = h->prof.launches;
    if (kernel_ms) *kernel_ms = h->prof.ms;
    if (reset) {
        h->prof.launches = 0;
        h->prof.ms = 0;
    }
    return MFX_OK;
}

// Which front-end kernel the BATCH entries run for this handle -- the ONE place that decides it (batch_run_range launches what
// this returns; mfx_dominant_kernel_name prints it; DESIGN.md section 5 tabulates it; tests/test_host.py pins the table
// through planning handles).  Order of preference: the three register kernels (4 frames per wave at 512 points and the
// short-window 1024-point case, 2 frames per wave at 2048 points), then the fused one-wave-per-frame kernels while their LDS
// fits (<= 2048 points), then spectrum through an HBM slab + k_melcep.
FrontKind choose_front(const mfx_handle *h) { return choose_front(h, h->batch.aligned); }

FrontKind choose_front(const mfx_handle *h, bool aligned)
{
    if (h->kaldi) return kKaldi; // (one kernel, whatever the alignment and the engine bits)
    // (else: the streaming interface's kernels; PLP has no fused front end: spectrum through HBM, then k_plp.  TRAPS takes
    // whatever the fbank handle of its shape takes: its front end IS that handle's, k_traps follows it)
    const bool allow_fused = !(h->cfg.engine & MFX_ENGINE_STREAM_KERNELS) && !h->plp;
    if (allow_fused && h->fast512 && h->plan16.ok) return kFront512;
    // (k_front1024, windows longer than 512 samples: aligned frames only)
    if (allow_fused && h->fast1024 && h->plan16.ok && (h->W <= 512 || aligned)) return kFront1024;
    // (2048 points, any window: stereo, mono on aligned sample pairs, mono at any alignment -- three builds)
    if (allow_fused && h->fast2048 && h->plan32.ok) return kFront2048;
    // (up to 2048 points the fused form saves the spectrum's round trip through HBM -- 8 KB per frame at 2048 points; at 4096
    // points the tables + per-wave buffers no longer leave enough waves per CU)
    if (allow_fused && h->W2 <= 2048 && h->own.plan64.ok) {
        FrontParams probe;
        fill_front(h, probe, aligned);
        if (front_wave_lds_bytes(probe, true) <= kLdsCap) return kFrontGenFused;
    }
    return h->fast512 ? kSpec512 : kSpecGen;
}

// With per-utterance warp factors in force (mfx_batch_set_alphas) the fused front ends, which know one filterbank, are
// out: the spectrum goes through the slab and k_melcep_runs / k_plp_runs apply each table to its own rows.
FrontKind batch_front(const mfx_handle *h)
{
    if (h->kaldi) return kKaldi; // (mfx_batch_set_alphas is refused on such a handle)
    if (h->batch.va.on) return h->fast512 ? kSpec512 : kSpecGen;
    return choose_front(h);
}

// The front end `kind` over the chunks of `w`, on h->stream -- the ONE place that launches it for the batch and the session
// entries.  Fused kinds: one launch.  Spectrum kinds: magnitudes go through the slab in windows of its rows (bounded by row
// span: chunk rows ascend), then k_melcep / k_plp per window.
int launch_front(mfx_handle *h, FrontParams &p, FrontKind kind, bool aligned, const FrontWork &w)
{
    p.chunks = w.d_chunks;
    p.n_chunks = (int32_t)w.n_chunks;
    if (!is_spec_kind(kind)) {
        if (kind == kFront512 || kind == kFront2048)
            p.spec = h->d_spec.p; // unused by the fused kernels; a -DMFX_STAMPS dev build drops its cycle sums here
        ProfScope ps(h, w.profile);
        switch (kind) {
        case kFront512: HIP_TRY(h, launch_front512(p, /*to_spectrum=*/false, aligned, h->nm16, h->stream)); break;
        case kFront1024:
            HIP_TRY(h, launch_front1024(p, aligned, h->nm16, h->stream, (h->cfg.engine & MFX_ENGINE_FRONT1024_12_WAVES) ? 12 : 16));
            break;
        case kFront2048: HIP_TRY(h, launch_front2048(p, h->num_cus, h->stream)); break;
        case kKaldi: {
            // (centred frames: the plan's own utterance count, and only while the bounds uploaded with that plan hold exactly
            // its utterances -- upload() sizes the buffer to the list; anything else is 0, which launch_kaldi refuses)
            const int32_t centred_utts =
                (h->kaldi_flags & kKaldiNoSnipEdges) && h->d_kaldi_bounds.n == 2 * (size_t)h->batch.n_utt ? h->batch.n_utt : 0;
            KaldiParams kp{p.pcm, p.pcm_total, p.chunks, p.n_chunks, p.row_limit, h->W, h->S, h->W2, h->nb, h->ceps, h->kaldi_preemph,
                           h->kaldi_remove_dc ? 1 : 0, h->kaldi_use_power ? 1 : 0, h->d_kaldi_ops.p, mel_spans(h), (int32_t)h->d_span_melw.n,
                           h->d_kaldi_dct_t.p, p.feat, p.feat_pitch, h->kaldi_flags, h->kaldi_log_floor,
                           h->d_kaldi_bounds.p, centred_utts};
            HIP_TRY(h, launch_kaldi(kp, h->stream));
            break;
        }
        default: HIP_TRY(h, launch_front_generic(p, /*fused=*/true, h->stream)); break;
        }
        return MFX_OK;
    }
    for (size_t c0 = 0, c1; c0 < w.n_chunks; c0 = c1) {
        const int64_t row0 = w.h_chunks[c0].out_row;
        int64_t rows = 0;
        for (c1 = c0; c1 < w.n_chunks && w.h_chunks[c1].out_row + w.h_chunks[c1].n_frames - row0 <= w.slab_rows; ++c1)
            rows = w.h_chunks[c1].out_row + w.h_chunks[c1].n_frames - row0;
        FrontParams q = p;
        q.chunks = w.d_chunks + c0;
        q.n_chunks = (int32_t)(c1 - c0);
        q.spec = w.slab - row0 * (int64_t)h->spec_pitch; // rows are addressed absolutely
        q.spec_pitch = h->spec_pitch;
        {
            ProfScope ps(h, w.profile);
            if (kind == kSpec512)
                HIP_TRY(h, launch_front512(q, /*to_spectrum=*/true, aligned, h->nm16, h->stream));
            else
                HIP_TRY(h, launch_front_generic(q, /*fused=*/false, h->stream));
        }
        int rc;
        if (w.runs) { // every table on its own rows of the window, one launch
            RowRuns rr;
            rr.runs = w.runs;
            rr.off = w.run_off;
            rr.row0 = row0;
            rr.rows = rows;
            rc = launch_cepstra_runs(h, *w.tables, q.spec, p.feat, p.feat_pitch, rr, w.h_run_off, w.h_runs, h->stream);
        } else {
            rc = launch_cepstra(h, h->own, w.slab, rows, p.feat + row0 * (int64_t)p.feat_pitch, p.feat_pitch, 1, 0, nullptr, h->stream);
        }
        if (rc != MFX_OK) return rc;
    }
    return MFX_OK;
}

extern "C" const char *mfx_dominant_kernel_name(const mfx_handle *h)
{
    if (!h) return "";
    if (h->stft) return h->stft_form == StftForm::Fft ? "k_stft_fft_mel" : "k_stft_mel";
    if (h->kaldi) return h->kaldi_flags != 0 ? "k_kaldi_front_opts" : "k_kaldi_front";
    switch (batch_front(h)) { // names as rocprofv3 prints them
    case kFront512:
    case kSpec512: return "k_front512";
    case kFront1024: return "k_front1024";
    case kFront2048: return "k_front2048";
    default: return h->W2 >= 1024 ? "k_front_reg" : "k_front_wave";
    }
}

/* planning handles only: frames of the batch on aligned sample pairs (even offsets and shift) or not -- what mfx_batch_plan
 * derives from the caller's offsets on a real handle */
extern "C" int mfx_plan_set_aligned(mfx_handle *h, int aligned)
{
    if (!h || !h->planning) return MFX_ERR_ARG;
    h->batch.aligned = aligned != 0;
    return MFX_OK;
}

// ------------------------------------------------------------------------------------------------
// the analysis window (both interfaces)
// ------------------------------------------------------------------------------------------------

extern "C" int mfx_set_window(mfx_handle *h, const float *window)
{
    MFX_DEVICE_ENTRY(h);
    if (!window) return fail(h, MFX_ERR_ARG, "invalid argument");
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->stft) { // the windowed basis as k_stft_mel streams it; the FFT form: the window and the FFT tables, no basis
        std::vector<float> ops;
        build_stft_form_operands(h->stft_form, h->W, window, ops);
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (h->batch.ov.stream2) HIP_TRY(h, hipStreamSynchronize(h->batch.ov.stream2));
        HIP_TRY(h, h->upload(h->d_stft_ops, ops));
        h->have_window = true;
        return MFX_OK;
    }
    if (h->kaldi) { // the window's W taps zero padded to N, and the FFT tables
        std::vector<float> ops;
        build_kaldi_operands(h->W, h->W2, window, ops);
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (h->batch.ov.stream2) HIP_TRY(h, hipStreamSynchronize(h->batch.ov.stream2));
        HIP_TRY(h, h->upload(h->d_kaldi_ops, ops));
        h->have_window = true;
        return MFX_OK;
    }
    std::vector<float> padded((size_t)h->W2, 0.f);
    std::memcpy(padded.data(), window, sizeof(float) * h->W);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, h->upload(h->d_window, padded));
    // window layouts of the register front ends (mfx_tables.h)
    std::vector<float> t, tw;
    if (h->fast1024 && h->W > 512) {
        build_front1024_long_window(padded, h->W2, t, tw);
        HIP_TRY(h, h->upload(h->d_win1024o, t));
        HIP_TRY(h, h->upload(h->d_winpair, tw));
    } else if (h->fast1024) {
        build_front1024_phase_o(padded, h->W2, t);
        HIP_TRY(h, h->upload(h->d_win1024o, t));
    }
    if (h->fast512 || (h->fast1024 && h->W <= 512)) {
        build_window_pairs(padded, h->W2, h->stuff256, t);
        HIP_TRY(h, h->upload(h->d_winpair, t));
    }
    h->have_window = true;
    return MFX_OK;
}

// ------------------------------------------------------------------------------------------------
// test taps
// ------------------------------------------------------------------------------------------------

extern "C" int64_t mfx_debug_read(mfx_handle *h, int kind, void *dst, int64_t dst_bytes)
{
    MFX_DEVICE_ENTRY(h);
    if (!dst) return fail(h, MFX_ERR_ARG, "invalid argument");
    if (hipSetDevice(h->device) != hipSuccess) return MFX_ERR_DEVICE;
    const void *src = nullptr;
    int64_t count = 0, esz = 4;
    if ((h->stft || h->kaldi) && kind != 8 && kind != 6) return kind >= 0 && kind <= 7 ? 0 : MFX_ERR_ARG; // (none of those tables or blocks exists)
    if (h->stft && kind == 6) return 0;
    switch (kind) {
    case 0:
        if (refresh_mel(h) != MFX_OK) return MFX_ERR_DEVICE;
        src = h->own.mel_w.p;
        count = 2 * (int64_t)h->W2;
        break;
    case 1:
        if (refresh_mel(h) != MFX_OK) return MFX_ERR_DEVICE;
        src = h->own.mel_beg.p;
        count = h->nb + 2;
        break;
    case 2:
        src = h->d_dct.p;
        count = h->ceps > 0 ? (int64_t)h->nb * h->dl : 0;
        break;
    case 3:
        src = h->d_spec.p;
        count = (int64_t)h->st.block_wcnd * h->spec_pitch;
        break;
    case 4: // raw head of the spectrum buffer (dev builds park in-kernel stamps there)
        src = h->d_spec.p;
        count = std::min<int64_t>(dst_bytes / 4, (int64_t)h->d_spec.n);
        break;
    case 5: // normaliser statistics of the last streaming apply(): [groups][2][cols] = (mean, multiplier) per column
            // group (static, delta, delta-delta when normalising after the deltas; statics only before)
        src = h->st.d_stats.p;
        count = h->cfg.norm == MFX_NORM_NONE ? 0 : (int64_t)(h->cfg.norm_after_dyn ? h->width / h->cols : 1) * 2 * h->cols;
        break;
    case 6: // normaliser statistics of the last batch run: [groups][n_utt][2][cols] (none while a speaker list is in force:
            // mfx_batch_speaker_stats returns those; none with the online normaliser: every row has its own)
        src = h->batch.d_stats.p;
        count = h->cfg.norm == MFX_NORM_NONE || h->batch.spk.on || h->batch.on.on ? 0
                                             : (int64_t)(h->cfg.norm_after_dyn ? h->width / h->cols : 1) * h->batch.n_utt * 2 * h->cols;
        break;
    case 7: // PLP autocorrelations of the last plain streaming apply(): [frames_with_context][lpc_order + 1]
        src = h->st.d_plp_r.p;
        count = h->plp ? (int64_t)h->st.block_wcnd * (h->lpc + 1) : 0;
        break;
    case 8: // converted PCM of the last batch run under a rates plan: int16, scratch layout (mfx_batch_resample_layout)
        src = h->batch.rs.d_pcm.p;
        count = h->batch.rs.on ? h->batch.rs.total * h->channels : 0;
        esz = 2;
        break;
    default:
        return MFX_ERR_ARG;
    }
    if (count * esz > dst_bytes) return MFX_ERR_ARG;
    if (count == 0) return 0;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return MFX_ERR_DEVICE;
    if (hipMemcpy(dst, src, (size_t)(count * esz), hipMemcpyDeviceToHost) != hipSuccess) return MFX_ERR_DEVICE;
    return count;
}

// ------------------------------------------------------------------------------------------------
// host-side table builders (no device)
// ------------------------------------------------------------------------------------------------

extern "C" int mfx_host_traps_basis(int32_t traps_len, int32_t traps_dct_len, float *basis)
{
    if (traps_len < 2 || traps_dct_len < 1 || !basis) return MFX_ERR_ARG;
    std::vector<float> b;
    build_traps_basis(traps_len, traps_dct_len, b);
    std::copy(b.begin(), b.end(), basis);
    return MFX_OK;
}

extern "C" int mfx_host_plp_tables(int32_t num_banks, int32_t fft_size, float sample_rate, float low_freq, float high_freq,
                                   float alpha, int32_t lpc_order, float *eql, float *idft)
{
    if (num_banks <= 0 || fft_size <= 0 || sample_rate <= 0 || lpc_order < 0 || !eql || !idft) return MFX_ERR_ARG;
    std::vector<float> e, b;
    build_plp_tables(num_banks, sample_rate, low_freq, high_freq, alpha, lpc_order, e, b);
    std::copy(e.begin(), e.end(), eql);
    std::copy(b.begin(), b.end(), idft);
    return MFX_OK;
}

extern "C" int mfx_host_mel_table(int32_t num_banks, int32_t fft_size, float sample_rate, float low_freq,
                                  float high_freq, float alpha, float *weights, int32_t *beg)
{
    if (num_banks <= 0 || fft_size <= 0 || !weights || !beg) return MFX_ERR_ARG;
    MelTable t;
    build_mel_table(num_banks, fft_size, sample_rate, low_freq, high_freq, alpha, t);
    std::memcpy(weights, t.weights.data(), sizeof(float) * t.weights.size());
    std::memcpy(beg, t.beg.data(), sizeof(int32_t) * t.beg.size());
    return MFX_OK;
}

// Lane plan of the mel walk (mfx::MelPlan; lanes = 16: the 512-point kernel's, max_read_bin 479; lanes = 64: the
// long-transform kernels').  Returns the number of rounds (<= 8), or an error.  Outputs (any may be NULL to
// query): L[8] bins per lane and round, *row_stride, start / fid [rounds][lanes], w [lanes][row_stride].
extern "C" int mfx_host_mel_lane_plan(int32_t lanes, int32_t num_banks, int32_t fft_size, const float *weights,
                                      const int32_t *beg, int32_t max_read_bin, int32_t *L, int32_t *row_stride,
                                      int32_t *start, int32_t *fid, float *w, int64_t w_cap)
{
    if ((lanes != 16 && lanes != 32 && lanes != 64) || num_banks <= 0 || fft_size <= 0 || !weights || !beg) return MFX_ERR_ARG;
    MelTable t;
    t.weights.assign(weights, weights + (size_t)2 * fft_size);
    t.beg.assign(beg, beg + num_banks + 2);
    for (int v : t.beg)
        if (v < 0 || v > fft_size / 2) return MFX_ERR_ARG;
    // (a 1024-point table on 16 lanes is k_front1024's plan: starts at multiples of 4 bins)
    MelPlan pl;
    if (!build_mel_plan(t, num_banks, fft_size, max_read_bin, lanes, lanes == 16 && fft_size == 1024 ? 4 : 2, pl)) return MFX_ERR_CONFIG;
    if (L) std::memcpy(L, pl.L, sizeof(int32_t) * 8);
    if (row_stride) *row_stride = pl.row_stride;
    if (start) std::memcpy(start, pl.start.data(), sizeof(int32_t) * pl.start.size());
    if (fid) std::memcpy(fid, pl.fid.data(), sizeof(int32_t) * pl.fid.size());
    if (w) {
        if ((int64_t)pl.w.size() > w_cap) return MFX_ERR_ARG;
        std::memcpy(w, pl.w.data(), sizeof(float) * pl.w.size());
    }
    return pl.rounds;
}

// Operands of the DCT on the matrix pipe: out[(tile * ksteps + j) * 64 + lane] (build_dct_mfma_operands); returns
// tiles * ksteps * 64, or the size needed when out is NULL.
extern "C" int64_t mfx_host_dct_mfma_operands(int32_t num_banks, int32_t dct_len, const float *matrix, float *out,
                                              int64_t out_cap, int32_t *tiles, int32_t *ksteps)
{
    if (num_banks <= 0 || dct_len <= 0 || !matrix) return MFX_ERR_ARG;
    std::vector<float> m(matrix, matrix + (size_t)num_banks * dct_len), ob;
    int tl = 0, ks = 0;
    build_dct_mfma_operands(m, num_banks, dct_len, tl, ks, ob);
    if (tiles) *tiles = tl;
    if (ksteps) *ksteps = ks;
    if (out) {
        if ((int64_t)ob.size() > out_cap) return MFX_ERR_ARG;
        std::memcpy(out, ob.data(), sizeof(float) * ob.size());
    }
    return (int64_t)ob.size();
}

extern "C" int mfx_host_dct_matrix(int32_t num_banks, int32_t ceps_len, int32_t want_c0, float lift_coef,
                                   float *matrix)
{
    if (num_banks <= 0 || ceps_len <= 0 || !matrix) return MFX_ERR_ARG;
    std::vector<float> m;
    build_dct_matrix(num_banks, ceps_len, want_c0 != 0, lift_coef, m);
    std::memcpy(matrix, m.data(), sizeof(float) * m.size());
    return MFX_OK;
}

extern "C" int64_t mfx_host_alpha_runs(int32_t n_utt, const float *alphas, const int64_t *frames, int64_t win_row0, int64_t win_rows,
                                       float *tables, int32_t *off, int64_t *runs)
{
    if (n_utt < 0 || (n_utt > 0 && (!alphas || !frames))) return MFX_ERR_ARG;
    std::vector<float> t;
    std::vector<int32_t> o;
    std::vector<int64_t> r;
    build_alpha_runs(alphas, frames, n_utt, t, o, r);
    if (win_rows >= 0) clip_alpha_runs(win_row0, win_rows, o, r);
    if (tables) std::copy(t.begin(), t.end(), tables);
    if (off) std::copy(o.begin(), o.end(), off);
    if (runs) std::copy(r.begin(), r.end(), runs);
    return (int64_t)t.size();
}

// Operands of k_splice_affine for one transform: out[(s * tiles + tile) * 64 + lane] (build_xform_operands); returns
// steps * tiles * 64, or the size needed when out is NULL.
extern "C" int64_t mfx_host_xform_operands(int32_t out_dim, int32_t in_dim, const float *A, float *out, int64_t out_cap,
                                           int32_t *tiles, int32_t *steps)
{
    if (out_dim < 1 || out_dim > 256 || in_dim < 1 || in_dim > 8192 || !A) return MFX_ERR_ARG;
    const int tl = (out_dim + 15) / 16, st = (in_dim + 3) / 4;
    const int64_t n = (int64_t)st * tl * 64;
    if (tiles) *tiles = tl;
    if (steps) *steps = st;
    if (out) {
        if (n > out_cap) return MFX_ERR_ARG;
        int a = 0, b = 0;
        build_xform_operands(A, out_dim, in_dim, a, b, out);
    }
    return n;
}

// ALL the LDS bytes of a block of the form's batch kernel at the tile mfx_create takes; a shape of another form is no argument
static int64_t host_stft_lds_bytes(StftForm form, int32_t N, int32_t S, int32_t M, int32_t *tile_rows)
{
    if (stft_form(N) != form || !stft_shape_ok(N, S, M)) return MFX_ERR_ARG;
    const int R = stft_tile_rows(N, S, M);
    if (tile_rows) *tile_rows = R;
    return R > 0 ? (int64_t)stft_lds_bytes(N, S, M, R) : MFX_ERR_CONFIG;
}

extern "C" int64_t mfx_host_stft_lds_bytes(int32_t dft_size, int32_t shift, int32_t num_banks, int32_t *tile_rows)
{
    return host_stft_lds_bytes(StftForm::Matrix, dft_size, shift, num_banks, tile_rows);
}

extern "C" int64_t mfx_host_stft_fft_lds_bytes(int32_t dft_size, int32_t shift, int32_t num_banks, int32_t *tile_rows)
{
    return host_stft_lds_bytes(StftForm::Fft, dft_size, shift, num_banks, tile_rows);
}

extern "C" int64_t mfx_host_stft_frame_count(int64_t samples, int32_t dft_size, int32_t shift)
{
    if (samples < 0 || stft_form(dft_size) == StftForm::None || shift < 1 || shift > dft_size) return MFX_ERR_ARG;
    return stft_frame_count(samples, dft_size, shift);
}

// FFT form: the tables as mfx_set_window uploads them behind the window: twid [dft_size / 2] complex, split [dft_size / 2 + 1]
// complex
extern "C" int mfx_host_stft_fft_tables(int32_t dft_size, float *twid, float *split)
{
    if (stft_form(dft_size) != StftForm::Fft || !twid || !split) return MFX_ERR_ARG;
    build_stft_fft_tables(dft_size, twid, split);
    return MFX_OK;
}

extern "C" int mfx_host_stft_basis(int32_t dft_size, const float *window, float *cos_sin)
{
    if (stft_form(dft_size) != StftForm::Matrix || !window || !cos_sin) return MFX_ERR_ARG;
    build_stft_basis(dft_size, window, cos_sin);
    return MFX_OK;
}

extern "C" int mfx_host_slaney_mel_table(int32_t num_banks, int32_t dft_size, float sample_rate, float low_freq, float high_freq,
                                         float *weights, int32_t *beg, int32_t *len)
{
    if (num_banks < 1 || num_banks > 128 || stft_form(dft_size) == StftForm::None || !weights || !beg || !len) return MFX_ERR_ARG;
    if (!(sample_rate > 0.f) || !(low_freq >= 0.f) || !(low_freq < high_freq) || !(high_freq <= sample_rate / 2)) return MFX_ERR_ARG;
    build_slaney_mel(num_banks, dft_size, sample_rate, low_freq, high_freq, weights, beg, len);
    return MFX_OK;
}

// ---- Kaldi front end: the three frame options; the tables as uploaded and the kernel's LDS, for tests (no device needed)
extern "C" int mfx_kaldi_set_options(mfx_handle *h, float preemph_coeff, int32_t remove_dc_offset, int32_t use_power)
{
    if (!h) return MFX_ERR_ARG;
    if (!h->kaldi) return fail(h, MFX_ERR_CONFIG, "mfx_kaldi_set_options: not a Kaldi handle (method != MFX_METHOD_KALDI)");
    if (!std::isfinite(preemph_coeff) || preemph_coeff < 0.f || preemph_coeff > 1.f)
        return fail(h, MFX_ERR_ARG, "mfx_kaldi_set_options: preemph_coeff must lie in [0, 1]");
    if ((remove_dc_offset != 0 && remove_dc_offset != 1) || (use_power != 0 && use_power != 1))
        return fail(h, MFX_ERR_ARG, "mfx_kaldi_set_options: remove_dc_offset and use_power are 0 or 1");
    if (h->sess.n > 0)
        return fail(h, MFX_ERR_STATE, "mfx_kaldi_set_options: sessions exist (an open stream's rows must not change under it): mfx_sessions_create(h, 0, 0) first");
    if (!h->planning) { // (runs in flight were queued with the options they were called under: they are kernel arguments)
        const int rc = sync_device(h);
        if (rc != MFX_OK) return rc;
    }
    h->kaldi_preemph = preemph_coeff;
    h->kaldi_remove_dc = remove_dc_offset != 0;
    h->kaldi_use_power = use_power != 0;
    return MFX_OK;
}

extern "C" int mfx_host_kaldi_mel_table(int32_t num_banks, int32_t fft_size, float sample_rate, float low_freq, float high_freq,
                                        float *weights, int32_t *beg, int32_t *len)
{
    double high = 0.0;
    if (num_banks < 1 || num_banks > 128 || (fft_size != 128 && fft_size != 256 && fft_size != 512) || !(sample_rate > 0.f) ||
        !kaldi_freqs_ok(sample_rate, low_freq, high_freq, &high) || !weights || !beg || !len)
        return MFX_ERR_ARG;
    build_kaldi_mel(num_banks, fft_size, sample_rate, low_freq, high, weights, beg, len);
    return MFX_OK;
}

extern "C" int mfx_host_kaldi_dct(int32_t num_banks, int32_t ceps_len, float lifter, float *matrix)
{
    if (num_banks < 1 || num_banks > 128 || ceps_len < 1 || ceps_len > num_banks || !(lifter >= 0.f) || !std::isfinite(lifter) || !matrix)
        return MFX_ERR_ARG;
    build_kaldi_dct(num_banks, ceps_len, lifter, matrix);
    return MFX_OK;
}

extern "C" int64_t mfx_host_kaldi_lds_bytes(int32_t window_size, int32_t shift, int32_t num_banks, int32_t ceps_len)
{
    if (!kaldi_shape_ok(window_size, shift, num_banks, ceps_len)) return MFX_ERR_ARG;
    return (int64_t)kaldi_lds_bytes(window_size, shift, num_banks, ceps_len);
}

extern "C" int32_t mfx_kaldi_flags_supported(void) { return kKaldiFlagsAll; }

extern "C" int64_t mfx_host_kaldi_lds_bytes_flags(int32_t window_size, int32_t shift, int32_t num_banks, int32_t ceps_len, int32_t flags)
{
    if (!kaldi_shape_ok(window_size, shift, num_banks, ceps_len) || !kaldi_flags_ok(flags)) return MFX_ERR_ARG;
    return (int64_t)kaldi_lds_bytes(window_size, shift, num_banks, ceps_len, flags);
}

extern "C" int64_t mfx_host_kaldi_frame_count(int64_t samples, int32_t window_size, int32_t shift, int32_t flags)
{
    if (samples < 0 || !kaldi_shape_ok(window_size, shift, 1, 0) || !kaldi_flags_ok(flags)) return MFX_ERR_ARG;
    return std::max<int64_t>(kaldi_frame_count(samples, window_size, shift, flags), 0);
}

extern "C" int mfx_host_kaldi_frame_samples(int64_t samples, int32_t window_size, int32_t shift, int32_t flags, int64_t t, int64_t *idx)
{
    if (samples < 0 || !kaldi_shape_ok(window_size, shift, 1, 0) || !kaldi_flags_ok(flags) || !idx) return MFX_ERR_ARG;
    if (t < 0 || t >= kaldi_frame_count(samples, window_size, shift, flags)) return MFX_ERR_ARG;
    kaldi_frame_samples(samples, window_size, shift, flags, t, idx);
    return MFX_OK;
}

extern "C" int64_t mfx_host_frame_count(int64_t samples, int32_t window_size, int32_t shift)
{
    if (window_size <= 0 || shift <= 0) return MFX_ERR_ARG;
    return frame_count(samples, window_size, shift);
}

// Sample-rate conversion: the table as mfx_batch_plan_rates uploads it, [L][P]; returns L * P (taps may be NULL to query)
extern "C" int64_t mfx_host_resample_taps(int32_t in_hz, int32_t out_hz, int32_t zeros, float rolloff, float *taps, int64_t cap,
                                          int32_t *L, int32_t *M, int32_t *P)
{
    ResampleShape sh;
    if (resample_shape(in_hz, out_hz, zeros, rolloff, sh) != 0) return MFX_ERR_ARG;
    const int64_t n = (int64_t)sh.L * sh.P;
    if (L) *L = sh.L;
    if (M) *M = sh.M;
    if (P) *P = sh.P;
    if (taps) {
        if (n > cap) return MFX_ERR_ARG;
        build_resample_taps(sh, taps);
    }
    return n;
}

extern "C" int64_t mfx_host_resampled_length(int64_t samples, int32_t in_hz, int32_t out_hz)
{
    if (samples < 0 || in_hz < 1000 || in_hz > 768000 || out_hz < 1000 || out_hz > 768000) return MFX_ERR_ARG;
    return resampled_length(samples, in_hz, out_hz);
}

extern "C" int64_t mfx_host_resample_layout(int32_t n_utt, const int64_t *lengths, const int32_t *rates_hz, int32_t out_hz,
                                            int64_t *offsets, int64_t *out_lengths)
{
    if (n_utt < 0 || (n_utt > 0 && (!lengths || !rates_hz)) || out_hz < 1000 || out_hz > 768000) return MFX_ERR_ARG;
    const int64_t total = resample_layout(n_utt, lengths, rates_hz, out_hz, offsets, out_lengths);
    return total < 0 ? MFX_ERR_ARG : total;
}

// Output samples per tile of k_resample for one rate pair (a multiple of 2; 4096 for in_hz == out_hz, whose samples are
// copied).  Test / inspection aid: utterance lengths around a tile edge.
extern "C" int32_t mfx_host_resample_tile(int32_t in_hz, int32_t out_hz, int32_t zeros, float rolloff, int32_t channels)
{
    if (channels < 0 || channels > 2) return MFX_ERR_ARG;
    ResRateSet set;
    if (build_resample_rates(channels, out_hz, &in_hz, 1, zeros, rolloff, true, set) != 0) return MFX_ERR_ARG;
    return set.tile_min; // (the one rate's tile_out, or kResCopyTile)
}
