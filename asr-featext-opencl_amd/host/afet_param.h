// afet_param.h -- source-compatible mirror of the reference's parameterizer interface, for C++
// callers that want to swap `new MfccOpenCL(...)` for `new MfccHip(...)` and change nothing else.
//
// Mirrors (interface only -- names, argument order and meaning, defaults, error behaviour):
//     Normalizer::norm_t          normalizer.h:5
//     class ParamBase             parambase.h:6-33   (+ parambase.cpp:4-19)
//     class MfccBase              mfccbase.h:6-52    (+ mfccbase.cpp:3-43)
//     class MfccOpenCL            mfccopencl.h:12-74 -> class MfccHip here
// All compute happens behind the C ABI of include/mfx.h (libmfcchip.so); nothing in this header
// or in mfcchip.cpp does arithmetic on samples or features.
#ifndef AFET_PARAM_H
#define AFET_PARAM_H

#include <stdexcept>

// -DAFET_USE_REFERENCE_HEADERS: take ParamBase / MfccBase / Normalizer from the reference's OWN headers
// (parambase.h:6-33, mfccbase.h:6-52, normalizer.h:5; add -I<reference>) and link the reference's parambase.cpp /
// mfccbase.cpp -- this is how MfccHip drops into the reference tree itself (INTEGRATION.md section 1;
// tests/test_host.py::test_mfcchip_builds_against_reference_headers).  Without it the mirror below stands in.
#ifdef AFET_USE_REFERENCE_HEADERS
#include "mfccbase.h"
struct mfx_handle;
#else

struct mfx_handle;

namespace Normalizer {
enum norm_t { NORM_NONE, NORM_CMN, NORM_CVN, NORM_MINMAX };
}

// Abstract streaming feature extractor: set_window once, then per file
//   while (samples) { n = set_input(pcm, cnt); set_alpha(a); apply(); get_output_data(out, n); }
//   n = flush(); if (n > 0) { set_alpha(a); apply(); get_output_data(out, n); }
// exactly as the reference driver does (ASR_OCL.cpp:152-301).
class ParamBase {
public:
    enum dyn_t { DYN_NONE, DYN_DELTA, DYN_ACC };

    ParamBase(int input_buffer_size, int window_size, int shift, Normalizer::norm_t norm, dyn_t dyn);
    virtual ~ParamBase() {}

    // largest block set_input accepts: whole frames that fit in the requested size (parambase.cpp:12-13)
    int get_input_buffer_size() const { return m_input_buffer_size; }
    // floor(float(samples - (W - S)) / S), float32 arithmetic as the reference (parambase.cpp:16-19)
    int estimated_window_count(int samples) const;
    void set_alpha(float alpha) { m_alpha = alpha; }   // not virtual (parambase.h:25): apply() forwards m_alpha

    virtual void set_window(const float *window) = 0;
    virtual int set_input(const short *data, int samples) = 0;
    virtual int flush() = 0;
    virtual void apply() = 0;
    virtual int get_output_data_width() const = 0;
    virtual void get_output_data(float *data_out, int window_count) = 0;

protected:
    int m_input_buffer_size, m_input_window_limit, m_window_size, m_shift;
    float m_alpha;
    Normalizer::norm_t m_norm;
    dyn_t m_dyn;
    bool m_last_block;
};

class MfccBase : public ParamBase {
public:
    MfccBase(int input_buffer_size, int window_size, int shift, int num_banks, float sample_rate, float low_freq,
             float high_freq, int ceps_len, bool want_c0, float lift_coef,
             Normalizer::norm_t norm = Normalizer::NORM_NONE, dyn_t dyn = DYN_NONE, int delta_l1 = 1,
             int delta_l2 = 1, bool norm_after_dyn = true);
    virtual ~MfccBase() {}

    int get_output_data_width() const override;

protected:
    int m_num_banks, m_ceps_len, m_dct_len, m_delta_l1, m_delta_l2;
    float m_sample_rate, m_low_freq, m_high_freq, m_lift_coef;
    bool m_want_c0, m_norm_after_dyn;
};

#endif // AFET_USE_REFERENCE_HEADERS

// The MI355X back end.  `hip_device` takes the place of MfccOpenCL's trailing cl_device_id
// (mfccopencl.h:60).  Errors surface as std::runtime_error with the reference's messages.
class MfccHip : public MfccBase {
public:
    MfccHip(int input_buffer_size, int window_size, int shift, int num_banks, float sample_rate, float low_freq,
            float high_freq, int ceps_len, bool want_c0, float lift_coef,
            Normalizer::norm_t norm = Normalizer::NORM_NONE, dyn_t dyn = DYN_NONE, int delta_l1 = 1,
            int delta_l2 = 1, bool norm_after_dyn = true, int hip_device = 0, bool bug_compat = true, int engine = 0);
    ~MfccHip() override;
    MfccHip(const MfccHip &) = delete;
    MfccHip &operator=(const MfccHip &) = delete;

    // set_alpha is ParamBase's own (non-virtual, stores m_alpha): apply() hands m_alpha to the library
    void set_window(const float *window) override;
    int set_input(const short *data, int samples) override;
    int flush() override;
    void apply() override;
    void get_output_data(float *data_out, int window_count) override;

    // VTLN sweep over the current block's spectrum (the caller's alpha loop, ASR_OCL.cpp:236-243, in
    // one call); block i of the result is read with get_output_data_alpha(i, ...)
    void apply_alphas(const float *alphas, int n_alpha);
    void get_output_data_alpha(int alpha_index, float *data_out, int window_count);

    // Many files in one launch sequence (mfx_batch_plan / mfx_batch_run_host): utterance u = samples [offsets[u],
    // offsets[u] + lengths[u]) of one PCM array, its rows start at out_rows[u]; returns the total number of rows
    long long batch_plan(int n_utt, const long long *offsets, const long long *lengths, long long *out_rows);
    // the same for files at their own sample rates (mfx_batch_plan_rates): offsets / lengths in input-rate samples, one rate
    // per utterance; the run converts them to the extractor's rate on the device first.  conv_lengths (may be null): the
    // converted lengths
    long long batch_plan_rates(int n_utt, const long long *offsets, const long long *lengths, const int *rates_hz, int zeros,
                               long long *out_rows, long long *conv_lengths = nullptr);
    void batch_run_host(const short *pcm, long long samples_total, float *out);
    // one warp factor per utterance of the planned batch (mfx_batch_set_alphas); nullptr / 0 clears the list, and so does
    // the next batch_plan
    void batch_set_alphas(const float *alphas, int n_utt);
    // per-speaker normalisation of the planned batch (mfx_batch_set_speakers): one speaker id per utterance; the prior (both
    // arrays or neither) carries the accumulators of earlier batches; prior_only: statistics from the prior alone.
    // nullptr / 0 clears the list, and so does the next batch_plan
    void batch_set_speakers(const int *utt_spk, int n_utt, int n_spk, const long long *prior_count = nullptr,
                            const double *prior_acc = nullptr, bool prior_only = false);
    // what the last run used: count [n_spk], acc [n_spk][4][Wn] (S, S2, min, max), stats [n_spk][2][Wn]; any may be null
    void batch_speaker_stats(long long *count, double *acc, float *stats);
    // online (causal, sliding-window) CMN / CVN of the planned batch (mfx_batch_set_online_norm): window in frames (0:
    // cumulative), the prior's reach and its accumulators [2][Wn] (nullptr with count 0: none); the next batch_plan clears it
    void batch_set_online_norm(int window, int prior_frames, long long prior_count = 0, const double *prior_acc = nullptr);
    // sliding-window CMN / CVN of the planned batch (mfx_batch_set_sliding_norm; norm = NONE handles): window and min_window in
    // frames, center and norm_vars 0 / 1; the next batch_plan clears it
    void batch_set_sliding_norm(int window, int min_window, int center, int norm_vars);
    // energy VAD + voiced-frame selection as the last stage of the planned batch's runs (mfx_batch_set_vad; mode MFX_VAD_*);
    // the next batch_plan clears it, and so does batch_clear_vad
    void batch_set_vad(int column, float energy_threshold, float energy_mean_scale, int frames_context, float proportion_threshold,
                       int mode);
    void batch_clear_vad();
    // pitch track of the planned batch (mfx_batch_set_pitch) and Kaldi's pitch features from it (mfx_batch_set_pitch_feats;
    // columns MFX_PF_*, 0: POV, normalised log-pitch, delta), pasted behind every row of a run when `paste`; the next
    // batch_plan clears both
    void batch_set_pitch(int window, int lag_min, int lag_max, float ballast, float lag_cost, float penalty, int max_jump);
    void batch_set_pitch_feats(int columns, int left, int right, int delta_window, float pov_scale, float pov_offset, float pitch_scale,
                               float delta_scale, bool paste);
    // what the last run decided: flags [total_rows], voiced [n_utt], threshold [n_utt]; any may be null.  Returns the batch's
    // voiced rows
    long long batch_vad_read(unsigned char *flags, int *voiced, float *threshold);
    // mfx_set_alpha at once, for the batch entries (there is no apply() to carry m_alpha there)
    void set_warp(float alpha);
    long long batch_frames(long long samples) const;

    // upper bound on the rows one set_input()/flush() can deliver (the reference's own bound,
    // estimated_window_count(get_input_buffer_size()), can be exceeded: SURVEY B6)
    int max_frames_out() const;
    mfx_handle *handle() const { return m_handle; }

protected:
    // method: MFX_METHOD_* of include/mfx.h (PlpHip passes MFX_METHOD_PLP and its model order, TrapsHip MFX_METHOD_TRAPS
    // and its two lengths, LogmelHip MFX_METHOD_STFT_LOGMEL and logmel_post, KaldiHip MFX_METHOD_KALDI and its two option fields)
    MfccHip(int input_buffer_size, int window_size, int shift, int num_banks, float sample_rate, float low_freq,
            float high_freq, int ceps_len, bool want_c0, float lift_coef, Normalizer::norm_t norm, dyn_t dyn, int delta_l1,
            int delta_l2, bool norm_after_dyn, int hip_device, bool bug_compat, int engine, int method, int lpc_order,
            int traps_len = 0, int traps_dct_len = 0, int logmel_post = 0, int kaldi_flags = 0, float kaldi_energy_floor = 0.f);

private:
    void check(int status) const;
    mfx_handle *m_handle;
};

// PLP cepstra (PLP) behind the same interface: MfccHip's arguments with the LPC model order after lift_coef
// (0 = 8, the reference CLI's --model-order default).  Same output width and row layout as the MFCC configuration.
class PlpHip : public MfccHip {
public:
    PlpHip(int input_buffer_size, int window_size, int shift, int num_banks, float sample_rate, float low_freq,
           float high_freq, int ceps_len, bool want_c0, float lift_coef, int lpc_order,
           Normalizer::norm_t norm = Normalizer::NORM_NONE, dyn_t dyn = DYN_NONE, int delta_l1 = 1, int delta_l2 = 1,
           bool norm_after_dyn = true, int hip_device = 0, bool bug_compat = true, int engine = 0);
};

// TRAPS temporal patterns (TRAPS) of the log mel energies: traps_dct_len DCT coefficients (0 = 10) of the
// traps_len frames (0 = 31) around each frame, per band; num_banks * traps_dct_len statics per row.  BATCH ENTRIES ONLY
// (batch_plan / batch_run_host): set_input, flush, apply and get_output_data throw "TRAPS handles have no streaming
// entries".  The warp factor is set with MfccHip::set_warp (there is no apply() to carry set_alpha's).
class TrapsHip : public MfccHip {
public:
    TrapsHip(int input_buffer_size, int window_size, int shift, int num_banks, float sample_rate, float low_freq,
             float high_freq, int traps_len, int traps_dct_len, Normalizer::norm_t norm = Normalizer::NORM_NONE,
             dyn_t dyn = DYN_NONE, int delta_l1 = 1, int delta_l2 = 1, bool norm_after_dyn = true, int hip_device = 0,
             int engine = 0);
    int get_output_data_width() const override; // num_banks * traps_dct_len * (1 + deltas): the library's own answer
};

// STFT log-mel spectrogram of the Whisper family ("STFT log-mel"; MFX_METHOD_STFT_LOGMEL): dft_size-point DFT of
// centred, reflect-padded frames, num_banks Slaney mel bands, log10, and what logmel_post (MFX_LOGMEL_*) names.  Set the
// periodic Hann window with set_window.  BATCH ENTRIES ONLY, as TrapsHip; no deltas, no normaliser.
class LogmelHip : public MfccHip {
public:
    LogmelHip(int input_buffer_size, int dft_size, int shift, int num_banks, float sample_rate, float low_freq, float high_freq,
              int logmel_post = 0 /* MFX_LOGMEL_WHISPER */, int hip_device = 0);
};

// Kaldi-compatible fbank / MFCC ("Kaldi front end"; MFX_METHOD_KALDI): ceps_len 0 delivers num_banks log mel
// energies, 1 .. num_banks Kaldi's cepstra with c0 first; lift_coef is cepstral_lifter (0: none); high_freq <= 0 is the offset
// from Nyquist.  Set the Povey window with set_window, the three frame options with set_options (Kaldi's defaults until then).
// kaldi_flags (MFX_KALDI_* of include/mfx.h: snip_edges = false, use_energy, raw_energy = false, htk_compat) and
// kaldi_energy_floor are creation-time: fbank with the energy column is num_banks + 1 wide.
// Batch entries (and the session entries of include/mfx.h); set_input, flush, apply and get_output_data throw.
class KaldiHip : public MfccHip {
public:
    KaldiHip(int input_buffer_size, int window_size, int shift, int num_banks, float sample_rate, float low_freq, float high_freq,
             int ceps_len, float lift_coef, Normalizer::norm_t norm = Normalizer::NORM_NONE, dyn_t dyn = DYN_NONE, int delta_l1 = 1,
             int delta_l2 = 1, bool norm_after_dyn = true, int hip_device = 0, int kaldi_flags = 0, float kaldi_energy_floor = 0.f);
    void set_options(float preemph_coeff, bool remove_dc_offset, bool use_power);
    int get_output_data_width() const override; // the static columns * (1 + deltas): the library's own answer
    // pow(0.5 - 0.5 cos(2 pi i / (n - 1)), 0.85), in double, rounded once
    static void povey_window(int n, float *window);
};

#endif // AFET_PARAM_H
