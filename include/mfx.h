/*
 * mfx.h -- C ABI of libmfcchip.so, the MI355X (gfx950) MFCC front end.
 *
 * This is the drop-in boundary for the reference's OpenCL back end (MfccOpenCL + SegmenterOpenCL +
 * clFFT/AppleFFT + NormalizerOpenCL + DeltaOpenCL).  Every entry point replaces one method of the
 * reference's parameterizer interface; the reference file:line it stands for is cited next to it
 * (paths relative to the reference repository).  Plain C types only: pointers, sizes, POD structs.
 *
 * Conventions
 *   - Every function returns MFX_OK (0) or a negative mfx_status; nothing throws.
 *   - mfx_last_error(h) returns the message for the last failure on that handle; the strings are
 *     the ones the reference throws as std::runtime_error, so a C++ wrapper can re-throw them.
 *   - A handle is bound to one HIP device and one stream and must be used from one thread at a
 *     time (the reference has no locking either: ASR_OCL.cpp:52,365-366).  Handles are independent.
 *   - Host pointers passed to the streaming calls are consumed before the call returns, so the
 *     caller may reuse one buffer for PCM-in and features-out as the reference driver does
 *     (ASR_OCL.cpp:160-161,231,243).
 *   - There is no CPU fallback: if the HIP runtime or a gfx950 device is missing, mfx_create fails.
 */
#ifndef MFX_H
#define MFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: mfx_config.batch_norm_stats (default 0 = the reference's block statistics; version 1 libraries took them over all T
 *    rows) and mfx_config.engine / tail_split, all carved out of reserved[] -- a zeroed reserved[] is still valid. */
#define MFX_ABI_VERSION 2

typedef enum {
    MFX_OK = 0,
    MFX_ERR_BUFFER_TOO_SMALL = -1, /* "Can't process data, buffer is too small"           mfcccpu.cpp:339, mfccopencl.cpp:473 */
    MFX_ERR_WINDOW_COUNT = -2,     /* "Can't process data, window count is too small"     segmentercpu.cpp:65, mfcccpu.cpp:396 */
    MFX_ERR_PROCESSED = -3,        /* "Processed samples <= 0, this should never happen"  segmentercpu.cpp:71 */
    MFX_ERR_WINDOW_HIGH = -4,      /* "Window count too high"                             mfcccpu.cpp:430 */
    MFX_ERR_CONFIG = -5,           /* invalid mfx_config                                                     */
    MFX_ERR_DEVICE = -6,           /* HIP runtime / device error (message carries hipGetErrorString)         */
    MFX_ERR_ARG = -7,              /* NULL or out-of-range argument                                          */
    MFX_ERR_STATE = -8             /* call out of sequence (e.g. get_output_data before apply)               */
} mfx_status;

/* Normalizer::norm_t, normalizer.h:5 */
enum { MFX_NORM_NONE = 0, MFX_NORM_CMN = 1, MFX_NORM_CVN = 2, MFX_NORM_MINMAX = 3 };
/* ParamBase::dyn_t, parambase.h:9 */
enum { MFX_DYN_NONE = 0, MFX_DYN_DELTA = 1, MFX_DYN_ACC = 2 };

/* Constructor arguments of MfccBase (mfccbase.h:21-35) / MfccOpenCL (mfccopencl.h:45-60), in the
 * same order, followed by extensions (all zero = reference behaviour). */
typedef struct mfx_config {
    int32_t input_buffer_size; /* "sample_limit": max samples per set_input (ASR_OCL.cpp:132,563)    */
    int32_t window_size;       /* W, samples                                                         */
    int32_t shift;             /* S, samples                                                         */
    int32_t num_banks;         /* mel filters                                                        */
    float sample_rate;
    float low_freq;
    float high_freq;
    int32_t ceps_len;          /* 0 = output log mel energies                                        */
    int32_t want_c0;           /* c0 appended as LAST column (mfcccpu.cpp:133-135)                   */
    float lift_coef;
    int32_t norm;              /* MFX_NORM_*                                                         */
    int32_t dyn;               /* MFX_DYN_*                                                          */
    int32_t delta_l1;          /* regression orders; (3 R + 2 (l1 + l2) + 2 l2) rows of the delta stage must fit  */
    int32_t delta_l2;          /* 160 KB of LDS (R = 64 rows of 16 floats up to 16 columns, else 32 rows of the
                                  column count: l1 = l2 <= 10 at 256 columns), else MFX_ERR_CONFIG      */
    int32_t norm_after_dyn;
    /* ---- extensions ---- */
    int32_t fft_size;          /* 0 = ceil2(window_size) as the reference (mfcccpu.cpp:94); else a
                                  power of two >= window_size (zero padded)                          */
    int32_t channels;          /* 0/1 = mono; 2 = interleaved stereo, downmixed (L+R)>>1 (batch API) */
    int32_t bug_compat;        /* 1 = reproduce reference behaviour B1 (static rows of a flush that
                                  follows exactly one set_input are read D rows early,
                                  mfcccpu.cpp:439 + segmentercpu.cpp:97-106); 0 = correct rows       */
    int32_t batch_norm_stats;  /* batch entries, norm after dyn: 0 = statistics as the reference computes them for
                                  an utterance it consumes as one block -- over the T - D rows that block delivers,
                                  re-used for the D flush rows (mfcccpu.cpp:377-388,395-407, normalizercpu.cpp:22-27);
                                  1 = over all T rows of the utterance.  Reference parity holds for utterances of at
                                  most input_buffer_size samples (longer files are several blocks in the reference,
                                  each with its own statistics: use the streaming entries for those)                  */
    int32_t engine;            /* MFX_ENGINE_* bits: which of two equivalent kernels serves a configuration (0 = the
                                  library's choice).  For cross-checks between kernels and A/B measurements; results
                                  agree to float32 rounding either way                                               */
    int32_t tail_split;        /* fused batch front ends: the last `tail_split` chunks of every wave of the grid are cut
                                  into 4-frame pieces so that the launch ends evenly; 0 = default (2), -1 = off        */
    int32_t method;            /* MFX_METHOD_*: 0 = MFCC; 1 = PLP cepstra (PLP): the same spectrum and mel
                                  table on power, equal loudness, cube root, LPC of order lpc_order, its cepstrum with the
                                  MFCC lifter; ceps_len >= 1 (no log-energy form); same output width and layout.  Check
                                  mfx_method_supported first: a library older than this field ignores it (returns MFCC) */
    int32_t lpc_order;         /* PLP: model order p, 1 .. min(32, num_banks); 0 = 8 (the reference CLI's default).
                                  Ignored for MFCC                                                                   */
    int32_t traps_len;         /* TRAPS: trajectory length L in frames, odd, 3 .. 101; 0 = 31 (the reference CLI's default).
                                  Ignored unless method is MFX_METHOD_TRAPS                                          */
    int32_t traps_dct_len;     /* TRAPS: DCT coefficients K kept per band, 1 .. min(32, L); 0 = 10 (the reference CLI's
                                  default).  Ignored unless method is MFX_METHOD_TRAPS                               */
    int32_t logmel_post;       /* STFT log-mel: MFX_LOGMEL_* -- what follows the log.  Ignored unless method is
                                  MFX_METHOD_STFT_LOGMEL                                                              */
} mfx_config;

/* kaldi_flags of mfx_create_kaldi / mfx_plan_create_kaldi (below); any other bit is MFX_ERR_CONFIG */
#define MFX_KALDI_NO_SNIP_EDGES 1   /* snip_edges = false: frames centred on the hops, the utterance mirrored at its ends */
#define MFX_KALDI_USE_ENERGY 2      /* use_energy = true: the frame's log-energy is a column of the row                   */
#define MFX_KALDI_ENERGY_WINDOWED 4 /* raw_energy = false (needs MFX_KALDI_USE_ENERGY, else MFX_ERR_CONFIG)               */
#define MFX_KALDI_HTK_COMPAT 8      /* htk_compat = true: HTK's column order                                              */

/* mfx_config.method.  3 = TRAPS temporal patterns (TRAPS): the log mel energies of the MFCC path (ceps_len = 0,
 * want_c0 = 0 required; lift_coef ignored), per band a Hamming-windowed DCT-II over the traps_len frames around each frame,
 * traps_dct_len coefficients kept; static row band-major, num_banks * traps_dct_len columns (at most 256).  BATCH ENTRIES
 * ONLY: on a TRAPS handle mfx_set_input, mfx_flush, mfx_apply, mfx_apply_alphas, mfx_get_output_data and
 * mfx_get_output_data_alpha return MFX_ERR_STATE.  The value 2 is unassigned and stays refused (mfx_method_supported(2) == 0):
 * libraries in the field answer for it, so TRAPS did not take it. */
enum { MFX_METHOD_MFCC = 0, MFX_METHOD_PLP = 1, MFX_METHOD_TRAPS = 3, MFX_METHOD_STFT_LOGMEL = 5, MFX_METHOD_KALDI = 7 };

/* mfx_config.method 5 = the log-mel spectrogram neural recognisers of the Whisper family feed on ("STFT log-mel"):
 * an exact-length DFT of centred, reflect-padded frames, Slaney mel bands, log10, and Whisper's clamp and map.  The value 4
 * is unassigned and stays refused, as 2 does.  The streaming entries (mfx_set_input ...) return MFX_ERR_STATE on such a handle;
 * the batch entries serve it, and the session entries do for logmel_post = MFX_LOGMEL_LOG10 or MFX_LOGMEL_LN (below, "Sessions").
 * Configuration (anything else: MFX_ERR_CONFIG).  window_size = N, the DFT length: even, 32 .. 512, or 1024 / 2048 (the FFT
 * form, below: every other length, odd or even, 514 included, stays refused); fft_size 0 or N
 * (mfx_fft_size returns N); shift = S in 1 .. N; num_banks = M in 1 .. 128, the output width; 0 <= low_freq < high_freq <=
 * sample_rate / 2; ceps_len = 0, want_c0 = 0, dyn = NONE, norm = NONE, channels 0 or 1.  lift_coef, the delta orders and
 * bug_compat are ignored.  The window is the caller's through mfx_set_window: the periodic Hann for Whisper.
 * Definition, per utterance of n samples (K1 = N / 2 + 1):
 *   Frames.  T = 0 when n <= N / 2, else T = n div S.  Frame t, tap j in [0, N) reads sample i = t S + j - N / 2; i < 0 reads
 *     sample -i, i >= n reads sample 2 (n - 1) - i: neither leaves [0, n).  That is torch.stft(center=True,
 *     pad_mode="reflect") with its last frame dropped, which is what Whisper keeps.  The reflection happens at the ends of the
 *     UTTERANCE, never into a neighbour's samples.
 *   Samples.  x[j] = (float)pcm * 2^-15 (exact).
 *   Basis.   Ck[k][j] = (float)(w[j] cos(2 pi ((k j) mod N) / N)), Sk[k][j] = (float)(-w[j] sin(2 pi ((k j) mod N) / N)), k <
 *     K1: in double from the float32 window, rounded once; rebuilt by mfx_set_window (which waits for the handle's streams
 *     and allocates there).
 *   DFT.     re[k] = 0, then for j = 0 .. N - 1 ascending re = fmaf(x[j], Ck[k][j], re); im[k] likewise with Sk.  The UNFOLDED
 *     form: N taps per chain, the frame is not folded first.  One float32 FMA chain per value, whose order does not depend on
 *     the tiling or on the batch.
 *   Power.   P[k] = fmaf(im, im, re * re) (no |X| / W2 scaling).
 *   Mel.     The table of librosa filters.mel(htk=False, norm="slaney"), in double, rounded once.  Hz to mel: f / (200 / 3)
 *     below 1000 Hz, else 15 + ln(f / 1000) / (ln 6.4 / 27).  Edges p[0 .. M + 1]: M + 2 points equally spaced in mel between
 *     low_freq and high_freq, mapped back to Hz.  f_k = k sample_rate / N.  Wm[m][k] = max(0, min((f_k - p[m]) / (p[m+1] -
 *     p[m]), (p[m+2] - f_k) / (p[m+2] - p[m+1]))) * 2 / (p[m+2] - p[m]).  mel[m] = 0, then over the row's non-zero span
 *     ascending mel = fmaf(Wm[m][k], P[k], mel).  A band narrower than a bin may have an empty span: it is 0 and takes the
 *     floor.  (Whisper ships this table as a file; the pin here is the formula.)
 *   Log.     v = max(mel, 1e-10f); L = log10(v) for WHISPER and LOG10, -10.0f when v is the floor itself (the correctly rounded
 *     value there); L = ln(v) for LN.
 *   Post.    WHISPER: mx = the largest L of all T * M values of the utterance; L = max(L, mx - 8.0f); out = (L + 4.0f) *
 *     0.25f.  LOG10 and LN deliver L.
 *   Output.  Rows [T][M], frame-major, at out_rows[u] (Whisper's own layout is the transpose, [M][T]).
 * Rows are an exact function of the utterance's samples, the window and the configuration: they do not depend on the other
 * utterances, on the run, on buffer placement, or on whether the utterance starts at an odd sample.
 * FFT form, N = 1024 or 2048 ("STFT log-mel, FFT form").  Frames, Samples, Power, Mel, Log, Post and Output are as
 * above, S in 1 .. N, M in 1 .. 128; the reflection never leaves [0, n) for these N either.  In place of Basis and DFT:
 *   Window.  z[j] = x[j] * w[j], one float32 product, w the caller's N floats from mfx_set_window -- which uploads the window
 *     and the FFT tables and builds no basis.  A window shorter than the DFT (win_length L < n_fft = N) is passed centred in N
 *     taps with zeros around it, left pad (N - L) div 2: torch.stft's rule.
 *   DFT.     X[k] = sum_j z[j] e^(-2 pi i j k / N), k < K1, by a float32 FFT (half-length complex FFT and real split).  It is
 *     NOT pinned to a summation order.  Its twiddle and split tables are built on the host in double and rounded once
 *     (mfx_host_stft_fft_tables); the sequence of float32 operations applied to a frame depends on N alone -- not on the tile,
 *     the wave, the frame's place in its block, or the batch; the factor 2 of the real split is removed by an exact 0.5.
 *   Contract.  Rows are a deterministic function of the utterance's samples, the window and the configuration: the same bits
 *     alone or in a batch, at an even or odd sample offset, on a second run, through the device or the host entry, at any
 *     4-byte placement of d_out, and nothing is written outside [d_out, d_out + total_rows M).  Accuracy against float64 is the
 *     project's bar (1e-4 of scale, 1e-5 relative L2), not a bit pin.
 *   Entries.  The batch entries as listed below.  The streaming entries AND mfx_sessions_create answer MFX_ERR_STATE with a
 *     message that names the batch entries: the carried-tail rule of the session entries stays limited to N <= 512.
 * Entries.  mfx_batch_frames, mfx_batch_plan and mfx_batch_plan_rates use the frame rule above; mfx_batch_run_device / _host,
 * mfx_batch_overlap, mfx_batch_set_transform and mfx_batch_set_vad work as on any handle; mfx_batch_set_alphas is refused with
 * MFX_ERR_CONFIG (there is no warped Slaney table) and mfx_set_alpha has no effect; the speaker list and the online
 * normaliser are refused as on any norm = NONE handle.
 * Sessions.  mfx_sessions_create serves LOG10 and LN handles; MFX_LOGMEL_WHISPER stays refused with MFX_ERR_STATE (its clamp
 * needs the largest value of the whole utterance, which an open stream does not have: use the batch entries).
 *   Delivery rule.  n = samples the session has received since it was opened (with mfx_sessions_set_rates: converted samples,
 *     n = J), T(n) = mfx_batch_frames(n).  A session has delivered rows [0, E): while open E = 0 when n <= N / 2, else E =
 *     min(n div S, (n - N / 2) div S + 1) -- the frames whose samples have all arrived without a right reflection (frame 0
 *     reads sample N / 2 through its left reflection) and that no later sample can take out of the utterance; once a push is
 *     final E = T(n), the flush (a final push without samples) included.  E never decreases, E <= T(n), and a final push
 *     delivers at most N / (2 S) + 1 rows beyond its own samples'.  A stream that ends with n <= N / 2 delivers nothing.
 *   Bits.  The rows of a push are the bits mfx_batch_run_device writes for the whole stream as one utterance on a handle of
 *     the same configuration: however the stream is cut (pushes of 0 or 1 samples, pushes across n = N / 2, pushes shorter
 *     than a hop, pieces at odd offsets of the caller's array), wherever d_out lies (any 4-byte alignment; nothing outside
 *     [d_out, d_out + total_rows * width) is written), with or without MFX_ENGINE_SESS_STFT_PLAIN.  The reflections happen
 *     at the true start and end of the stream only.  After a final push the id is fresh and may be reused at once.
 *   Composition.  No static rows are carried (D = 0).  mfx_sessions_set_transform reads the delivered rows: its Ex rule and
 *     bits are those of mfx_batch_set_transform on the batch twin.  mfx_sessions_set_rates converts in front: bits of the
 *     mfx_batch_plan_rates twin.  The online normaliser stays refused (norm = NONE is required); mfx_set_alpha has no
 *     effect.  mfx_sessions_run_device allocates nothing; a push leaves the batch plan and the streaming state alone. */
enum { MFX_LOGMEL_WHISPER = 0, MFX_LOGMEL_LOG10 = 1, MFX_LOGMEL_LN = 2 };

/* mfx_config.method 7 = the Kaldi-compatible front end ("Kaldi front end"): what compute-fbank-feats /
 * compute-mfcc-feats and torchaudio.compliance.kaldi.fbank define -- per-frame DC removal, pre-emphasis, the Povey window, power
 * spectrum, Kaldi's mel table, log, and for MFCC Kaldi's DCT and lifter with c0 in column 0.  The value 6 is unassigned and stays
 * refused, as 2 and 4 do.  The definition below is restated from Kaldi's feature-window.cc, mel-computations.cc, feature-fbank.cc
 * and feature-mfcc.cc; agreement with a Kaldi or torchaudio binary has NOT been measured (neither is available to the build).
 * Configuration (anything else: MFX_ERR_CONFIG, from mfx_create and mfx_plan_create).  window_size = W in 65 .. 512; N = the next
 * power of two >= W (128, 256 or 512); fft_size 0 or N (mfx_fft_size returns N); shift = S in 1 .. W; num_banks = M in 1 .. 128;
 * channels 0 or 1; low_freq >= 0; high_freq > 0 is absolute, high_freq <= 0 is Kaldi's offset from Nyquist (sample_rate / 2 +
 * high_freq); then low < high <= sample_rate / 2.  ceps_len = C: 0 delivers the M log mel energies (fbank), 1 .. M Kaldi's
 * num_ceps cepstra WITH c0 IN COLUMN 0; want_c0 must be 0 (c0 is already in).  lift_coef = Kaldi's cepstral_lifter Q >= 0, 0
 * meaning none (ignored at C = 0; the rule that refuses lift_coef == 0 does not apply to this method).  norm, dyn, delta_l1 / l2,
 * norm_after_dyn and batch_norm_stats are as on an MFCC handle; bug_compat, engine, lpc_order, traps_* and logmel_post are
 * ignored.  Width = (C or M) * (1 + dyn).  The three frame options come through mfx_kaldi_set_options (below).
 * Definition, per utterance of n samples: T = mfx_batch_frames = floor((n - W) / S) + 1 for n >= W, else 0 (Kaldi's snip_edges =
 * true).  For frame t and taps i in [0, W):
 *   Samples.  x[i] = (float)pcm[t S + i], not scaled: Kaldi works in the int16 range.
 *   DC.       s = the exact integer sum of the frame's W samples (it fits int32); mean = (float)s / (float)W, one conversion and
 *     one float32 division; d[i] = x[i] - mean.  With DC removal off d = x.
 *   Pre-emphasis, c = preemph_coeff.  e[i] = fmaf(-c, d[i - 1], d[i]) for i >= 1, e[0] = fmaf(-c, d[0], d[0]): the frame's first
 *     sample stands for its predecessor, so no sample outside the frame is read.  With c = 0, e = d.
 *   Window.   z[i] = e[i] * w[i], w the caller's W floats from mfx_set_window; z[i] = 0 for W <= i < N.  The Povey window is
 *     pow(0.5 - 0.5 cos(2 pi i / (W - 1)), 0.85), in double, rounded once.
 *   DFT.      X[k] = sum_i z[i] e^(-2 pi i i k / N), k in [0, N / 2), by a float32 FFT (half-length complex FFT and real split).
 *     It is NOT pinned to a summation order.  Its tables are built on the host in double and rounded once; the float32
 *     operations a frame sees depend on N alone -- not on the chunk, the wave, the frame's place in its block, the batch or the
 *     entry.
 *   Power.    P[k] = fmaf(im, im, re * re); with use_power = 0, P[k] = sqrtf(P[k]).
 *   Mel.      Kaldi's table, in double, rounded once (mfx_host_kaldi_mel_table).  mel(f) = 1127 ln(1 + f / 700), f_k = k
 *     sample_rate / N; only bins k < N / 2 enter (the Nyquist bin has no weight).  ml = mel(low), mh = mel(high), delta = (mh -
 *     ml) / (M + 1); band m has l = ml + m delta, c = l + delta, r = l + 2 delta; Wm[m][k] = 0 unless l < mel(f_k) < r, else
 *     (mel - l) / (c - l) when mel <= c, else (r - mel) / (r - c).  mel[m] = 0, then over the band's non-zero span in ascending
 *     k mel = fmaf(Wm[m][k], P[k], mel).  An empty band is 0 and takes the floor.
 *   Log.      L[m] = logf(max(mel[m], 0x1p-23f)): the floor is Kaldi's FLT_EPSILON; silence gives -15.9424.
 *   Cepstra (C > 0).  D[0][m] = sqrt(1 / M), D[i][m] = sqrt(2 / M) cos(pi / M (m + 1/2) i); l[i] = 1 + (Q / 2) sin(pi i / Q), or 1
 *     at Q = 0; G[i][m] = (float)(l[i] D[i][m]), in double, rounded once (mfx_host_kaldi_dct); c[i] = 0, then in ascending m
 *     c = fmaf(G[i][m], L[m], c).
 *   Contract.  Rows are a deterministic function of the utterance's samples, the window, the configuration and the three
 *     options: the same bits alone or in a batch, at an even or odd sample offset, on a second run, through the device or the
 *     host entry, at any 4-byte placement of d_out with nothing written outside the rows, and through the session entries however
 *     the stream is cut.  Accuracy against float64 is the project's bar (1e-4 of scale, 1e-5 relative L2), not a bit pin.
 * Entries.  The batch entries and the session entries serve the method exactly as they serve an MFCC handle of the same W, S,
 * width, dyn and norm: D, the carried rows, mfx_sessions_set_online_norm, _set_transform and _set_rates are unchanged, and all
 * batch attachments work (mfx_batch_set_vad's default column -1 is the last static column: callers who want c0 pass column =
 * 0).  Refused: mfx_batch_set_alphas with MFX_ERR_CONFIG (there is no Kaldi VTLN warp; mfx_set_alpha has no effect), and the
 * streaming entries (mfx_set_input, mfx_flush, mfx_apply, mfx_apply_alphas, mfx_get_output_data[_alpha]) with MFX_ERR_STATE
 * and a message that names the batch entries.
 * Options (kaldi_flags and kaldi_energy_floor of mfx_create_kaldi / mfx_plan_create_kaldi; restated from Kaldi's
 * feature-window.cc, feature-fbank.cc and feature-mfcc.cc).  They are creation-time arguments, not arguments of
 * mfx_kaldi_set_options, because they change the output width and the frame count, which size buffers at creation; and they
 * are arguments of a creation entry of their own, not fields of mfx_config, whose size and last field stay what libraries and
 * callers in the field agree on.  mfx_create is mfx_create_kaldi with both zero: the definition above and its bits.  Unknown bits,
 * ENERGY_WINDOWED without USE_ENERGY, a negative or non-finite floor, or a shape whose rows no longer fit the kernel's LDS
 * (mfx_host_kaldi_lds_bytes_flags): MFX_ERR_CONFIG.
 *   Width.    fbank (C = 0): M + 1 static columns with USE_ENERGY, else M.  MFCC: C columns.  mfx_get_output_data_width and
 *     every buffer follow.
 *   Frames, NO_SNIP_EDGES.  T = mfx_batch_frames = (n + S div 2) div S, 0 for n = 0.  Frame t, tap i reads utterance sample
 *     r(t S + S div 2 - W div 2 + i), r being Kaldi's loop `while s < 0 or s >= n: s = -s - 1 if s < 0 else 2 n - 1 - s`, that
 *     is the symmetric reflection of period 2 n: m = s mod 2 n (non-negative), r = m if m < n else 2 n - 1 - m.  The kernel
 *     uses the closed form (mfx_host_kaldi_frame_samples restates it).  The reflection happens at the ends of the UTTERANCE,
 *     never into a neighbour's samples: nothing outside [offset, offset + n) is read.  DC removal, pre-emphasis (the frame's
 *     first tap still stands for its predecessor), window, DFT and everything after see the W gathered samples exactly as they
 *     see a frame above.
 *   Energy, USE_ENERGY.  E = sum over i < W of d[i]^2, d after DC removal and before pre-emphasis and window (Kaldi's
 *     raw_energy = true); with ENERGY_WINDOWED E = sum of z[i]^2, z after the window.  The sum is float32: per-lane ascending
 *     FMA chains, then a wave reduction; it is NOT pinned to a summation order, but its operation sequence depends on W alone.
 *     logE = logf(max(E, 0x1p-23f)); if kaldi_energy_floor > 0, logE = max(logE, lf), lf = (float)log((double)floor), built
 *     once on the host.
 *   Columns.  fbank + USE_ENERGY: logE in column 0, the log mel energies in 1 .. M; with HTK_COMPAT the bands in 0 .. M - 1 and
 *     logE in column M.  HTK_COMPAT without USE_ENERGY changes nothing on fbank.  MFCC + USE_ENERGY: column 0 is logE instead
 *     of c0.  MFCC + HTK_COMPAT: columns 1 .. C - 1 move to 0 .. C - 2 and column C - 1 takes logE with USE_ENERGY, else
 *     (float)((double)c0 * 1.4142135623730951) (Kaldi's M_SQRT2 on c0).  The lifter is applied before the move, as in Kaldi.
 *     mfx_batch_set_vad's default column -1 (the last static column) therefore lands on the energy under HTK_COMPAT +
 *     USE_ENERGY, which is the column Kaldi's VAD reads.
 *   Contract. As above: the same bits alone or in a batch, at any sample offset, on a second run, through the device or the host
 *     entry, at any 4-byte placement of d_out, nothing written outside the rows.
 *   Entries.  The batch entries and all their attachments see rows and T and work unchanged, mfx_batch_plan_rates included (its
 *     frame rule acts on the converted lengths).  mfx_batch_set_pitch (and so _set_pitch_feats) on a NO_SNIP_EDGES handle is
 *     refused with MFX_ERR_CONFIG: the track's frames follow the snip-edged rule and would not line up with the rows.  The session
 *     entries serve USE_ENERGY, ENERGY_WINDOWED and HTK_COMPAT with no change of the step rule, as the batch twin's bits;
 *     mfx_sessions_create on a NO_SNIP_EDGES handle answers MFX_ERR_STATE with a message that names the batch entries (the
 *     carry and delivery rule differs: left reflection at the stream start, W / 2 + S / 2 more samples held back, final-push
 *     frames; it is not served yet).
 * Not served: dither, vtln_warp, W > 512, stereo; sessions with snip_edges = false. */

/* mfx_config.engine bits */
#define MFX_ENGINE_NO_FRONT1024 1 /* 1024-point short-window configurations stay on the generic long-transform kernel  */
#define MFX_ENGINE_NO_FRONT2048 4 /* 2048-point short-window configurations stay on the generic long-transform kernel  */
#define MFX_ENGINE_STREAM_KERNELS 8 /* batch entries run the streaming interface's kernels (spectrum through HBM, then the
                                      mel / DCT kernel) instead of the fused front ends: the rows are then the SAME BITS
                                      that set_input / apply / get_output_data deliver for a file consumed as one block
                                      (the fused kernels agree with them to float32 rounding, ~1e-6 of scale)           */
#define MFX_ENGINE_FUSE_DELTA 2   /* 512-point batch path: delta / delta-delta computed inside the front-end kernel (a delta
                                     wave per block, idle front-end waves sharing its tiles) instead of the separate delta
                                     kernel, on a batch of any size that qualifies (the same bits)  */
#define MFX_ENGINE_FUSE_NO_SHARE 16384  /* fused delta stage: the delta wave alone works the block's tiles off              */
#define MFX_ENGINE_FUSE_SHARE_ALL 32768 /* fused delta stage: the delta wave claims nothing, front-end waves that have run out
                                           of frames take every tile (orders whose 16-row sub-tile does not fit a wave's frame
                                           slots: as MFX_ENGINE_FUSE_NO_SHARE)                                             */
#define MFX_ENGINE_NO_FUSE_DELTA 65536  /* the separate delta kernel always (wins over MFX_ENGINE_FUSE_DELTA)               */

#define MFX_ENGINE_NORM_TWO_KERNELS 16 /* normaliser: statistics and apply as two launches also where one block's LDS holds a
                                          segment's rows (the one-launch form computes the same bits)                    */
#define MFX_ENGINE_DMA_SMALL_BLOCKS 32  /* streaming interface: blocks under 1 MB are copied by DMA commands (as larger ones are)
                                           instead of by a copy kernel through the pinned staging buffers                 */
#define MFX_ENGINE_NO_DCT_SPLIT 64      /* 2048-point fused kernel: the DCT as one 64-column tile also where at most 40 columns
                                           are wanted (else: column groups x band parts, summed across the wave)          */
#define MFX_ENGINE_NO_STUFF256 128      /* 256-point transforms stay on the one-wave-per-frame kernel instead of the zero-stuffed
                                           form of the 512-point kernel                                                   */

#define MFX_ENGINE_TRAPS_VALU 512        /* TRAPS: the trajectory DCT on the vector ALUs instead of the matrix pipe (the same
                                           ascending float32 FMA chain per output: the same bits)                        */

#define MFX_ENGINE_XFORM_VALU 1024       /* splice + affine transform (mfx_batch_set_transform): the FMA chains on the vector
                                           ALUs instead of the matrix pipe (the same chain per output: the same bits)     */

#define MFX_ENGINE_SESS_NARROW_LOADS 2048 /* session entries: k_sess_gather reads its sources with 2-byte loads throughout instead
                                            of whole 32-bit words and a byte-align step (the same bits; the comparator of
                                            the measurement in DESIGN.md, "Session entries")                             */

#define MFX_ENGINE_SESS_XFORM_PLAIN 4096 /* session entries with mfx_sessions_set_transform: the transform of a push runs
                                           k_splice_affine itself, one segment per session, instead of k_sess_xform, which packs
                                           row groups of different sessions into one block (the same bits; the comparator of
                                           tools/sess_xform_bench.py) */
#define MFX_ENGINE_SESS_STFT_PLAIN 8192 /* session entries on an STFT log-mel handle: a push runs k_stft_mel itself, one chunk per
                                           run of frames of one session, instead of k_sess_stft_mel, which packs 16-frame groups
                                           of different sessions into one block (the same bits; the comparator of
                                           tools/sess_stft_bench.py) */
#define MFX_ENGINE_FRONT1024_12_WAVES 256 /* 1024-point fused kernel: the 12-waves-per-CU build also where the 16-wave build fits
                                            (aligned frames, window <= 512 samples, tables small enough): the same bits      */

typedef struct mfx_handle mfx_handle;

/* ---- lifetime: replaces `new MfccOpenCL(..., cl_device_id)` (ASR_OCL.cpp:140-143,
 *      mfccopencl.cpp:98-233) and `delete param` (ASR_OCL.cpp:323) ---- */
int mfx_create(const mfx_config *cfg, int hip_device, mfx_handle **out);
void mfx_destroy(mfx_handle *h);
const char *mfx_last_error(const mfx_handle *h);
/* message for a status code when no handle exists (mfx_create failure) */
const char *mfx_status_string(int status);
int mfx_abi_version(void);
/* 1 when this library computes mfx_config.method `method` (MFX_METHOD_*), else 0 */
int mfx_method_supported(int32_t method);
/* The three frame options of a Kaldi handle (MFX_METHOD_KALDI); after mfx_create Kaldi's defaults are in force: 0.97f, 1, 1.
 * MFX_ERR_CONFIG on a handle of another method; MFX_ERR_ARG for a preemph_coeff outside [0, 1] or not finite, or a flag other
 * than 0 / 1; MFX_ERR_STATE while sessions exist (an open stream's bits must not change under it: mfx_sessions_create(h, 0, 0)
 * first).  It works on a planning handle, waits for the handle's streams, and allocates nothing. */
int mfx_kaldi_set_options(mfx_handle *h, float preemph_coeff, int32_t remove_dc_offset, int32_t use_power);
/* mfx_create / mfx_plan_create for a Kaldi handle (cfg->method == MFX_METHOD_KALDI, else MFX_ERR_CONFIG) with the options of
 * method 7, "Options": kaldi_flags = MFX_KALDI_* bits, kaldi_energy_floor = Kaldi's energy_floor (0 = none; must be >= 0 and
 * finite).  Unknown bits, MFX_KALDI_ENERGY_WINDOWED without MFX_KALDI_USE_ENERGY or a bad floor: MFX_ERR_CONFIG.  (0, 0.f) is
 * mfx_create / mfx_plan_create itself. */
int mfx_create_kaldi(const mfx_config *cfg, int32_t kaldi_flags, float kaldi_energy_floor, int hip_device, mfx_handle **out);
int mfx_plan_create_kaldi(const mfx_config *cfg, int32_t kaldi_flags, float kaldi_energy_floor, mfx_handle **out);
/* the MFX_KALDI_* bits this library serves (15); a library older than the options has neither this symbol nor
 * mfx_create_kaldi */
int32_t mfx_kaldi_flags_supported(void);

/* ---- streaming parameterizer interface, one function per ParamBase method (parambase.h:23-32) ---- */

/* ParamBase::set_window (parambase.h:27; SegmenterOpenCL::set_window segmenteropencl.cpp:110-118):
 * window_size floats, copied. */
int mfx_set_window(mfx_handle *h, const float *window);
/* ParamBase::set_input (parambase.h:28; MfccOpenCL::set_input mfccopencl.cpp:472-480): uploads
 * `samples` int16 samples, frames + windows them and runs the FFT.  *frames_out = frames that the
 * next apply()/get_output_data() will deliver (0 when the block is still too short). */
int mfx_set_input(mfx_handle *h, const int16_t *pcm, int32_t samples, int32_t *frames_out);
/* ParamBase::flush (parambase.h:29; mfccopencl.cpp:482-493) */
int mfx_flush(mfx_handle *h, int32_t *frames_out);
/* ParamBase::set_alpha (parambase.h:25): VTLN warp factor used by the next apply() */
int mfx_set_alpha(mfx_handle *h, float alpha);
/* ParamBase::apply (parambase.h:30; mfccopencl.cpp:495-549): filterbank -> log -> DCT -> delta ->
 * normalisation for the current block; may be repeated with different alpha on one FFT result
 * (ASR_OCL.cpp:236-243). */
int mfx_apply(mfx_handle *h);
/* ParamBase::get_output_data_width (parambase.h:31; mfccbase.cpp:33-43) */
int mfx_get_output_data_width(const mfx_handle *h);
/* ParamBase::get_output_data (parambase.h:32; mfccopencl.cpp:551-569): `frames` rows of
 * get_output_data_width() floats, row-major [static | delta | delta-delta]. */
int mfx_get_output_data(mfx_handle *h, float *data_out, int32_t frames);
/* VTLN sweep: the reference's alpha loop (ASR_OCL.cpp:236-243: one set_input, then set_alpha + apply +
 * get_output_data per warp factor; warp mfcccpu.cpp:36-38) as ONE call.  All n_alpha warped filterbanks
 * are applied to the stored spectrum of the current block in one launch per stage; results are the
 * same as n_alpha rounds of mfx_set_alpha + mfx_apply.  Read block a with mfx_get_output_data_alpha.
 * The handle's own alpha (mfx_set_alpha) is not changed.  Normalisation statistics are kept per
 * alpha, so a flush block re-uses the statistics of the same alpha (normalizercpu.cpp use_last_stats).
 * The plain rows and the sweep's rows of a block are kept apart, and may be read in any order and more than
 * once: a sweep does not change what mfx_get_output_data returns for the block's plain apply, and a plain
 * apply does not change what mfx_get_output_data_alpha returns.  mfx_set_input and mfx_flush end both:
 * mfx_get_output_data_alpha on a block that has had no sweep returns MFX_ERR_STATE. */
int mfx_apply_alphas(mfx_handle *h, const float *alphas, int32_t n_alpha);
int mfx_get_output_data_alpha(mfx_handle *h, int32_t alpha_index, float *data_out, int32_t frames);
/* ParamBase::get_input_buffer_size / estimated_window_count (parambase.h:23-24, parambase.cpp:12-19) */
int mfx_get_input_buffer_size(const mfx_handle *h);
int mfx_estimated_window_count(const mfx_handle *h, int32_t samples);
/* True upper bound on the frames one set_input()/flush() can return.  The reference sizes its
 * output buffer from estimated_window_count(get_input_buffer_size()) (ASR_OCL.cpp:157-161), which
 * a steady-state block can exceed; size output buffers with this instead. */
int mfx_max_frames_out(const mfx_handle *h);
/* FFT length in use (mfcccpu.cpp:94) */
int mfx_fft_size(const mfx_handle *h);

/* ---- batch interface: many independent utterances per call (the reference processes its file
 *      list one utterance at a time through the loop at ASR_OCL.cpp:163-321; this runs the same
 *      per-utterance computation -- whole-utterance semantics, i.e. what a multi-block streaming
 *      run delivers -- for all of them in one launch sequence) ---- */

/* Frames of one utterance of `samples` samples per channel (= estimated_window_count, but with
 * integer arithmetic so it stays exact above 2^24 samples; parambase.cpp:16-19). */
int64_t mfx_batch_frames(const mfx_handle *h, int64_t samples);

/* Describe a batch: utterance u occupies samples [offsets[u], offsets[u]+lengths[u]) of the PCM
 * array (per channel; for stereo the array holds 2*that many interleaved int16).  Feature rows of
 * utterance u start at row out_rows[u] of the output (computed here: prefix sum of frame counts).
 * Arrays are host pointers, copied.  Returns total rows in *total_rows. */
int mfx_batch_plan(mfx_handle *h, int32_t n_utt, const int64_t *offsets, const int64_t *lengths,
                   int64_t *out_rows, int64_t *total_rows);

/* Run the planned batch on DEVICE pointers: d_pcm (int16, HBM) -> d_out (float [total_rows][width],
 * HBM).  Asynchronous on the handle's stream; nothing is copied to or from the host.  This is the
 * entry the roofline numbers are measured on.  d_pcm must be 4-byte aligned; when the number of int16
 * elements is odd the kernels read the 32-bit word that holds the last sample whole (2 bytes past the
 * last element, inside any device allocation; that half-word only meets a zero window tap).
 * With normalisation on, an utterance's statistics are the reference's for a file consumed as one
 * block (mfx_config.batch_norm_stats).
 * d_out may have any 4-byte alignment and may lie anywhere in a device allocation (row k of a larger matrix, say): the rows are
 * the same bits wherever it lies, and nothing outside [d_out, d_out + total_rows * width) is written (width =
 * mfx_batch_output_width; pinned by tests/test_placement_gpu.py). */
int mfx_batch_run_device(mfx_handle *h, const int16_t *d_pcm, int64_t pcm_samples_total, float *d_out);

/* Per-utterance VTLN: one warp factor per utterance of the planned batch, in the plan's utterance order -- the alpha loop
 * of ASR_OCL.cpp:236-243 applied across files: sweep, pick a factor per speaker, then extract every utterance with its own
 * factor in ONE run instead of one plan and run per distinct factor.  Valid after mfx_batch_plan; n_utt must be the planned
 * count and every factor > 0 (MFX_ERR_ARG otherwise).  The list is reduced to its distinct float values, compared bit for
 * bit (nothing is quantised for the caller); more than 4096 distinct values is MFX_ERR_ARG (the cap of mfx_apply_alphas).
 * alphas == NULL with n_utt == 0 clears the list, and so does a later mfx_batch_plan (the list is tied to the plan's
 * utterance order): the handle is back on mfx_set_alpha's factor and the kernels it ran before.
 * All tables and lists are built, allocated and uploaded HERE (the call waits for the handle's streams);
 * mfx_batch_run_device still allocates nothing.  mfx_set_alpha and the handle's own tables are untouched: streaming calls
 * on the same handle are unaffected.  Accepted for MFCC, log mel energies (ceps_len = 0), PLP and TRAPS.
 * While a list is in force the batch runs spectrum -> HBM slab -> k_melcep_runs / k_plp_runs (every table on its own rows,
 * one launch per slab and stage) whatever front end the shape would otherwise take: rows of utterance u are bit-identical
 * to those of an MFX_ENGINE_STREAM_KERNELS handle at mfx_set_alpha(alphas[u]); mfx_dominant_kernel_name names the
 * spectrum kernel that runs and mfx_profile_read times it.  MFX_ENGINE_FUSE_DELTA and mfx_batch_overlap have NO effect on
 * such a run: neither the fused delta plan nor the statics scratch (and with it the second stream) is taken. */
int mfx_batch_set_alphas(mfx_handle *h, const float *alphas, int32_t n_utt);

/* Splice + affine transform as the last stage of a batch run ("Splice + affine transform"): LDA / HLDA / MLLT
 * over spliced frames, PCA or a linear merger over TRAPS columns, a per-speaker fMLLR matrix.  No reference analogue.
 * For utterance u with T frames, let y[t] (t = 0 .. T-1) be the rows the handle delivers today, of width
 * Wd = mfx_get_output_data_width(h), layout [static | d | dd], normalised if normalisation is on.  With left, right >= 0,
 * C = left + right + 1 and in_dim = C * Wd:
 *   1. Splice.  z[t] = [ y[clamp(t-left, 0, T-1)] | ... | y[clamp(t+right, 0, T-1)] ]: the first and last frame of the
 *      UTTERANCE are replicated, the rule the delta stage and TRAPS use.
 *   2. Affine map with transform x = utt_xf[u] (0 when no list is given); A_x row-major [out_dim][in_dim], b_x [out_dim]:
 *      acc = b_x[r]; for i = 0 .. in_dim-1 ascending: acc = fmaf(A_x[r][i], z[t][i], acc); out[t][r] = acc.
 *      A float32 chain with one FMA per tap, in this order: a row's bits do not depend on the tiling, on the other
 *      utterances of the batch, or on whether the matrix-pipe or the vector form (MFX_ENGINE_XFORM_VALU) computed it.
 *   3. Output.  d_out is then [total_rows][out_dim] in the plan's row order (out_rows[u] unchanged).  The rows y are not
 *      delivered.
 * Valid after mfx_batch_plan (MFX_ERR_STATE before one).  A == NULL with n_xf == 0 clears the transform, and so does a
 * later mfx_batch_plan (the list and the scratch are tied to the plan): the handle is back on its previous kernels and
 * bits.  MFX_ERR_ARG: left or right outside 0 .. 32, out_dim outside 1 .. 256, n_xf outside 1 .. 1024, in_dim > 8192,
 * utt_xf given with n_utt != the planned count or with an entry outside [0, n_xf).  The matrix values are not inspected.
 * The matrices (in the layout the kernel streams, mfx_host_xform_operands), the biases, the per-utterance index and a
 * handle-owned scratch [total_rows][Wd] for the rows y are allocated and uploaded HERE (the call waits for the handle's
 * streams); mfx_batch_run_device still allocates nothing.  While a transform is in force a batch run does exactly what it
 * does today with that scratch in the place of d_out -- whatever the front end, MFX_ENGINE_* bits, per-utterance alpha
 * list or mfx_batch_overlap mode, so the rows the transform reads are bit-identical to those of a handle without one --
 * and k_splice_affine then turns scratch rows into d_out as the last launch, on the stream the tail runs on.
 * mfx_batch_run_host sizes and copies its output by mfx_batch_output_width.  The streaming entries, mfx_set_alpha,
 * mfx_debug_read, mfx_dominant_kernel_name and mfx_profile_read (which still name and time the front end) do not change. */
int mfx_batch_set_transform(mfx_handle *h, int32_t left, int32_t right, int32_t out_dim, int32_t n_xf,
                            const float *A,        /* [n_xf][out_dim][in_dim]            */
                            const float *b,        /* [n_xf][out_dim], NULL = zeros      */
                            const int32_t *utt_xf, /* [n_utt] transform of each utterance, NULL = all 0 */
                            int32_t n_utt);
/* out_dim while a transform is in force, else mfx_get_output_data_width */
int mfx_batch_output_width(const mfx_handle *h);

/* Per-speaker CMN / CVN / MINMAX ("Per-speaker normalisation"): the statistics of the normaliser pooled over all
 * utterances of a speaker -- compute-cmvn-stats --spk2utt, then apply-cmvn --utt2spk, of a Kaldi-style recipe -- between the
 * per-utterance warp factor (mfx_batch_set_alphas) and the per-speaker transform (mfx_batch_set_transform).  No reference
 * analogue: its NormalizerCPU keeps one block's statistics (normalizercpu.cpp:22-27).
 * utt_spk[u] in [0, n_spk) is the speaker of utterance u of the planned batch.  Wn is the number of normalised columns:
 * mfx_get_output_data_width when norm_after_dyn, else the static column count.
 *   Scope.  Valid after mfx_batch_plan / mfx_batch_plan_rates (MFX_ERR_STATE before one); MFX_ERR_CONFIG on a handle with
 *     norm == MFX_NORM_NONE, MFX_ERR_DEVICE on a planning handle.  utt_spk == NULL with n_utt == 0 clears the list, and so
 *     does a later plan: the handle is back on today's kernels and bits.  MFX_ERR_ARG: n_utt is not the planned count, an id
 *     outside [0, n_spk), n_spk outside 1 .. 2^20, only one of the two prior arrays, a negative prior_count, a mode other
 *     than the two below, MFX_SPK_PRIOR_ONLY without a prior or with a speaker of count 0 that owns an utterance with frames.
 *     The lists, the prior, the per-chunk partial totals, the accumulators and the statistics are allocated and uploaded
 *     HERE (the call waits for the handle's streams); mfx_batch_run_device still allocates nothing.
 *   Statistics.  Every utterance contributes all T of its rows (mfx_config.batch_norm_stats is ignored).  Per utterance and
 *     column the totals -- S and S2 in double, S2 from the float32 product v * v, min and max -- are formed exactly as
 *     k_norm_stats forms them for a segment of those rows: the same thread per (row class, column), the same order of double
 *     additions, the same tree, chunks of 4096 rows combined in ascending order.  Per speaker the accumulator starts from
 *     the prior if one is given (a prior of count 0 counts as none), else from the totals of the speaker's first
 *     contributing utterance as they are; the remaining utterances are added in ascending utterance index, min / max
 *     likewise.  With n = prior count + pooled rows: mean = (float)(S / n); CVN multiplier (float)sqrt((n - 1) / (S2 - S (S /
 *     n))); MINMAX 1 / max(|min - mean|, |max - mean|) in float32; CMN 1 -- the per-utterance normaliser's formulas on those
 *     doubles.  MFX_SPK_PRIOR_ONLY: the statistics come from the prior alone, the batch's rows are not accumulated.  A
 *     speaker's bits therefore do not depend on the other speakers, on how the ids are numbered, or on unrelated utterances
 *     of the batch.  A speaker without rows and without a prior has n = 0 and non-finite statistics, which no row reads.
 *   Apply.  Every row of utterance u becomes (v - mean[spk]) * mult[spk] (v - mean[spk] for CMN), the float32 expression of
 *     the per-utterance normaliser, in its place in the run: before the deltas or after them as configured, on the stream
 *     the tail runs on.  Everything else in the run is unchanged -- front end, MFX_ENGINE_* bits, alpha list, rates plan,
 *     mfx_batch_overlap, the transform (which reads the normalised rows).  While a list is in force mfx_batch_run_host takes
 *     its unsliced path (a speaker may span slices) and mfx_debug_read kind 6 returns 0 elements.
 *   Read-back.  mfx_batch_speaker_stats synchronises and returns what the last run used: count [n_spk], acc [n_spk][4][Wn]
 *     (S, S2, min, max; prior plus batch, in MFX_SPK_PRIOR_ONLY the prior) and stats [n_spk][2][Wn] (mean, multiplier).  Any
 *     output may be NULL.  MFX_ERR_STATE without a list in force or before a run.  Feeding a run's count and acc as the next
 *     batch's prior gives the same bits as one batch holding both, provided each speaker's utterances keep their order;
 *     summing the accumulators of several devices on the host (sharding.merge_speaker_acc) and running MFX_SPK_PRIOR_ONLY
 *     is the multi-GPU flow.
 * The session entries and the streaming interface are untouched and ignore the list.  While the online normaliser
 * (mfx_batch_set_online_norm, below) is in force the setter answers MFX_ERR_STATE. */
enum { MFX_SPK_POOL = 0, MFX_SPK_PRIOR_ONLY = 1 };
int mfx_batch_set_speakers(mfx_handle *h, const int32_t *utt_spk, int32_t n_utt, int32_t n_spk,
                           const int64_t *prior_count, /* [n_spk] or NULL */
                           const double *prior_acc,    /* [n_spk][4][Wn]: S, S2, min, max; or NULL */
                           int32_t mode);
int mfx_batch_speaker_stats(mfx_handle *h, int64_t *count, double *acc, float *stats /* [n_spk][2][Wn] mean, multiplier */);

/* Online CMN / CVN: a causal sliding-window (or cumulative) normaliser, per stream, for the batch entries and the session
 * entries ("Online normalisation") -- apply-cmvn-online of a Kaldi-style recipe: training features made to match
 * what a live recogniser's normaliser delivers, and that normaliser itself on the session entries.  No reference analogue:
 * its NormalizerCPU keeps one block's statistics (normalizercpu.cpp:22-27).  It needs no look-ahead, so the sessions' E does
 * not change.  A stream is one utterance of a batch or one session.
 *   Inputs.  Rows v[t][j], t = 0, 1, ..., j < Wn; Wn as for the speaker list (mfx_get_output_data_width when norm_after_dyn,
 *     else the static column count), Wn <= 256 (MFX_ERR_CONFIG beyond).  The rows are what the handle's norm = NONE twin
 *     delivers at the normaliser's place in the run: before or after the deltas, as norm_after_dyn says.
 *     q[t][j] = (double)(v * v), the product rounded to float32 first (k_norm_stats' rule).
 *   Parameters.  window N: 0 (cumulative: statistics from the start of the stream) or a multiple of 32 in 32 .. 4096 (the
 *     last N rows, row t included).  prior_frames F in 0 .. 2^20.  prior_count p >= 0.  prior_acc [2][Wn] doubles (sum, sum
 *     of squares), NULL exactly when p = 0.  The kind is mfx_config.norm: MFX_NORM_CMN or MFX_NORM_CVN; MFX_NORM_MINMAX and
 *     MFX_NORM_NONE are refused with MFX_ERR_CONFIG.  Anything else outside these limits: MFX_ERR_ARG.
 *   Prefix sums, per column, in chunks of 32 rows counted from the stream's first row (the same chains run on q):
 *     inside chunk c, I = 0, then for each row ascending I = I + (double)v[r]; I[t] is the value after row t; Tot[c] is I at
 *     the chunk's last row; across chunks O[0] = 0, O[c + 1] = O[c] + Tot[c]; P[t] = O[t div 32] + I[t].
 *   Window.  n = t + 1 and Sw = P[t] when N = 0 or t < N; else n = N and Sw = P[t] - P[t - N] (N is a multiple of 32: the
 *     trailing row sits at the same place in its chunk as row t).  Qw likewise from the q chains.
 *   Prior (Kaldi's global-stats smoothing).  k = min(p, F - n) when p > 0 and F > n, else 0.  If k > 0: r = (double)k /
 *     (double)p, Sw = Sw + PS[j] * r, Qw = Qw + PQ[j] * r (product and sum rounded separately).  nn = (double)(n + k).
 *   Statistics and apply.  m = Sw / nn, mean = (float)m.  CVN: d = Qw - Sw * m; mult = (float)sqrt((nn - 1) / d) when nn >= 2
 *     and d > 0, else 1.0f.  y = v - mean (CMN), y = (v - mean) * mult (CVN), in float32.  Every double operation above is
 *     rounded on its own (no fused multiply-add), so the rows are an exact function of v and the parameters: they do not
 *     depend on the other streams, on buffer placement, on the run, or -- for a session -- on how the stream is cut.
 *   Batch.  mfx_batch_set_online_norm is valid after mfx_batch_plan / mfx_batch_plan_rates (MFX_ERR_STATE before one); a
 *     later plan drops it with the other attachments; mfx_batch_clear_online_norm puts the handle back on the per-utterance
 *     normaliser's kernels and bits.  MFX_ERR_STATE while a speaker list is in force, and mfx_batch_set_speakers answers
 *     MFX_ERR_STATE while this attachment is.  MFX_ERR_DEVICE on a planning handle.  mfx_config.batch_norm_stats is ignored
 *     and mfx_debug_read kind 6 returns 0 elements.  Everything is allocated HERE (the call waits for the handle's streams):
 *     16 bytes per 32-row chunk and column of totals / offsets, and a handle-owned scratch [total_rows][width] (grown, never
 *     shrunk) that everything ahead of the normaliser's place writes instead of the run's rows -- the normaliser does not
 *     run in place, its trailing edge reads raw rows; mfx_batch_run_device still allocates nothing.  Everything else in a
 *     run is unchanged: front end, MFX_ENGINE_* bits, alpha list, rates plan, mfx_batch_overlap, the transform and the VAD
 *     (which read the normalised rows).  Utterances are independent: mfx_batch_run_host keeps its sliced path.
 *   Sessions.  mfx_sessions_set_online_norm stores the parameters and allocates nothing; it and
 *     mfx_sessions_clear_online_norm are valid only while no sessions exist (before mfx_sessions_create, or after
 *     mfx_sessions_create(h, 0, 0)), else MFX_ERR_STATE.  mfx_sessions_create on a CMN / CVN handle succeeds only with the
 *     parameters set, and then sizes the state: 8 doubles per session and column (lead and trail O and I of v and q), and
 *     when N > 0 a ring of the last N raw rows, n_sessions * N * Wn * 4 bytes (MFX_ERR_DEVICE when that cannot be
 *     allocated).  Every push then runs ONE more launch, k_onorm_sess: behind the deltas on the rows [E_old, E_new) it
 *     delivers, or ahead of them on the new frames' static rows in the slot (carried static rows are already normalised).
 *     A push may deliver more rows than N.  A final push or mfx_sessions_reset leaves the session fresh.  The rows of a
 *     push are THE SAME BITS that mfx_batch_run_device writes for the whole utterance on a handle of the same
 *     configuration with mfx_batch_set_online_norm of the same parameters.
 * One prior serves all streams.  NOT served: MINMAX, TRAPS handles on the session entries, the streaming interface
 * (mfx_set_input / mfx_apply), which is untouched. */
int mfx_batch_set_online_norm(mfx_handle *h, int32_t window, int32_t prior_frames, int64_t prior_count,
                              const double *prior_acc /* [2][Wn] or NULL */);
int mfx_batch_clear_online_norm(mfx_handle *h);
int mfx_sessions_set_online_norm(mfx_handle *h, int32_t window, int32_t prior_frames, int64_t prior_count,
                                 const double *prior_acc /* [2][Wn] or NULL */);
int mfx_sessions_clear_online_norm(mfx_handle *h);

/* Sliding-window CMN / CVN of the batch entries ("Sliding-window normalisation"): apply-cmvn-sliding of a
 * Kaldi-style recipe -- a mean (optionally a variance) over a window of a few hundred frames around every row, centred or
 * trailing -- the normaliser of the speaker-recognition recipes (compute-mfcc-feats, compute-vad-energy, apply-cmvn-sliding
 * --center=true --cmn-window=300, select-voiced-frames).  The definition below is restated from Kaldi's SlidingWindowCmn
 * (feature-functions.cc); AGREEMENT WITH A KALDI BINARY HAS NOT BEEN MEASURED (none is available to the build).  No
 * reference analogue.  The online normaliser above cannot stand in for it: it is causal, its window is a multiple of 32 and
 * it divides the variance by n - 1.
 *   Rows.  For utterance u with T frames, y[t] is the row the transform and the VAD read today: width Wy =
 *     mfx_batch_output_width WITHOUT a transform, pasted pitch columns included when a paste is in force.  Wy <= 256
 *     (MFX_ERR_CONFIG beyond).  All Wy columns are normalised.  v = y[t][j]; q = (double)(float)(v * v), the product rounded
 *     to float32 first (k_norm_stats' rule).
 *   Window of row t (Kaldi's rule), N = window.  With center: ws = t - N div 2, we = ws + N.  Without it: ws = t - N,
 *     we = t + 1 -- THE STEADY WINDOW THEN HOLDS N + 1 ROWS, as in Kaldi.  If ws < 0: we -= ws, ws = 0.  Without center:
 *     we = max(t + 1, min_window); min_window is ignored with center, as in Kaldi.  If we > T: ws -= we - T, we = T,
 *     ws = max(ws, 0).  n = we - ws; always 0 <= ws <= t < we <= T.
 *   Sums.  P is the prefix chain the online normaliser defines above -- chunks of 32 rows from the utterance's first row, I,
 *     Tot, O -- built on v and on q.  Sw = P[we - 1] - P[ws - 1] with P[-1] = 0 (the subtraction is done then too); Qw
 *     likewise.  Every double operation is rounded on its own (no fused multiply-add).
 *   Statistics and apply.  m = Sw / n, mean = (float)m, c = v - mean in float32.  CMN (norm_vars = 0): y = c.  With
 *     norm_vars: if n == 1, y = +0.0f; else var = Qw / n - m * m (quotient, product and difference rounded separately), var
 *     = 1e-10 when var < 1e-10, mult = (float)(1.0 / sqrt(var)) (square root and quotient rounded separately), y = c * mult
 *     in float32.  This is Kaldi's population variance and its floor, not the online normaliser's n - 1.
 *     The rows are an exact function of the utterance's rows and the four parameters: they do not depend on the other
 *     utterances, the tiling, buffer placement, the run, or the device or host entry.
 *   Scope.  Valid after mfx_batch_plan / mfx_batch_plan_rates (MFX_ERR_STATE before one); a later plan drops it with the other
 *     attachments; mfx_batch_clear_sliding_norm puts the handle back on its previous kernels and bits.  MFX_ERR_CONFIG:
 *     mfx_config.norm != MFX_NORM_NONE (this normaliser replaces the others, it does not stack on them), an STFT log-mel
 *     handle, Wy > 256.  MFX_ERR_ARG: window outside 1 .. 4096, min_window outside 0 .. window, center or norm_vars other than
 *     0 / 1.  MFX_ERR_DEVICE on a planning handle.  Everything is allocated HERE (the call waits for the handle's streams):
 *     a handle-owned raw-row scratch [total_rows][Wy] (grown, never shrunk) and 16 bytes per 32-row chunk and column of
 *     totals / offsets; mfx_batch_run_device still allocates nothing.  While it is in force a call that would change Wy
 *     (mfx_batch_set_pitch_feats, mfx_batch_clear_pitch, mfx_batch_clear_pitch_feats) answers MFX_ERR_STATE, as under a
 *     transform or a VAD.
 *   Place in a run.  One more link, between the rows y and the transform: everything up to and including the pitch paste
 *     writes the raw rows into the scratch; k_onorm_totals, k_onorm_offsets and k_slide_apply read them and write the
 *     normalised rows where the rows y went before; the transform and the tensor output read the normalised rows.  The VAD's
 *     decision reads the raw rows (see there).  The front end, MFX_ENGINE_* bits, alpha list, rates plan and
 *     mfx_batch_overlap are unchanged; the launches go on the stream the tail runs on.  Utterances are independent:
 *     mfx_batch_run_host keeps its sliced path.
 * NOT served: the session entries and the streaming interface, which ignore it (a centred window needs N / 2 rows of
 * look-ahead); stacking on another normaliser; windows beyond 4096. */
int mfx_batch_set_sliding_norm(mfx_handle *h, int32_t window, int32_t min_window, int32_t center, int32_t norm_vars);
int mfx_batch_clear_sliding_norm(mfx_handle *h);

/* Energy voice-activity decision and voiced-frame selection as the last stage of a batch run ("Voice activity and
 * frame selection"): compute-vad-energy followed by select-voiced-frames of a Kaldi-style recipe, on the device, behind
 * everything else a run does.  No reference analogue: the reference hands every frame to its consumer.
 *   Input.  For utterance u with T frames, y[t] is the row the handle delivers today WITHOUT a transform: width Wd =
 *     mfx_get_output_data_width, normalised if normalisation is on (per utterance or per speaker).  e[t] = y[t][column];
 *     column = -1 means the last static column (c0 when want_c0).  A transform in force does not change what is read.
 *     Nor does the sliding-window normaliser (mfx_batch_set_sliding_norm; norm = NONE handles only): it sits between the
 *     rows y and the transform, so the decision reads the raw c0 or energy -- threshold and flags are what they are
 *     without that attachment -- and SELECT / PACK move the finished, normalised rows.  That is the recipe's order
 *     (compute-vad-energy on the raw features, apply-cmvn-sliding, select-voiced-frames).
 *   Threshold.  thr_u = (float)((double)energy_threshold + (double)energy_mean_scale * (S / T)), S = the sum of e[t] over
 *     all T rows in double: rows i, i + 256, ... of every 4096-row chunk by one owner in ascending order, a halving tree over
 *     the 256 owners, the chunks in ascending order.  No atomics: thr_u does not depend on the other utterances of the batch,
 *     on buffer placement, or on the run.  T = 0 gives thr_u = energy_threshold.
 *   Decision (Kaldi's rule; the window is CUT at the utterance ends, not replicated).  For frame t, den = the number of t2 in
 *     [t - frames_context, t + frames_context] with 0 <= t2 < T, num = the number of those with e[t2] > thr_u (a float32
 *     comparison: a NaN on either side is "not greater"), flag[t] = ((float)num >= (float)den * proportion_threshold) in
 *     float32.  Given the rows and thr_u the flags are an exact function.
 *   Modes.  Wo = mfx_batch_output_width, which the VAD does not change; out_rows[u] are the plan's and do not move.
 *     MFX_VAD_FLAGS   d_out is exactly what it is without the VAD; only flags and counts are produced.
 *     MFX_VAD_SELECT  the voiced rows of u, in ascending t, go to rows out_rows[u] .. out_rows[u] + voiced[u] - 1 -- the
 *                     rows the handle would deliver without the VAD (the transform's output if one is in force), bit for
 *                     bit; rows [out_rows[u] + voiced[u], out_rows[u] + T) are written as +0.0f.
 *     MFX_VAD_PACK    the voiced rows of the whole batch lie back to back: utterance u starts at row packed_row0[u], the
 *                     exclusive prefix sum of voiced; packed_row0[n_utt] = total_voiced; rows [total_voiced, total_rows) are
 *                     written as +0.0f.
 *     In every mode nothing outside [d_out, d_out + total_rows * Wo) is written, and mfx_batch_run_device's placement rule
 *     holds: any 4-byte alignment, the same bits.
 *   Scope.  Valid after mfx_batch_plan / mfx_batch_plan_rates (MFX_ERR_STATE before one); a later plan drops the VAD with
 *     the other attachments, and mfx_batch_clear_vad puts the handle back on today's kernels and bits.  MFX_ERR_ARG: column
 *     outside [-1, Wd), frames_context outside 0 .. 64, proportion_threshold not in (0, 1], a non-finite energy_threshold or
 *     energy_mean_scale, an unknown mode.  MFX_ERR_DEVICE on a planning handle.  The flags [total_rows], the counts,
 *     thresholds and packed_row0, the per-chunk sums and per-tile masks and, for SELECT / PACK, a handle-owned scratch
 *     [total_rows][Wo] (grown, never shrunk; re-sized by a later mfx_batch_set_transform) are allocated HERE (the call waits
 *     for the handle's streams); mfx_batch_run_device still allocates nothing.
 *   Composition.  Everything else in a run is unchanged -- front end, MFX_ENGINE_* bits, alpha list, rates plan, speaker
 *     list, mfx_batch_overlap, the transform.  In SELECT / PACK the run's last stage writes to the scratch instead of the
 *     caller's array; the VAD's launches follow on the stream the tail runs on.  mfx_batch_run_host works in every mode; its
 *     sliced path stays on in FLAGS and SELECT (utterances are independent), PACK takes the unsliced path as a speaker list
 *     does.
 *   Read-back.  mfx_batch_vad_read synchronises and returns what the last run produced: flags [total_rows] (0 / 1),
 *     voiced [n_utt], threshold [n_utt], *total_voiced.  Any output may be NULL.  MFX_ERR_STATE without a VAD in force or
 *     before a run.  mfx_batch_vad_device returns the handle-owned device arrays (d_packed_row0 has n_utt + 1 entries): valid
 *     until the next plan or clear, and ordered after the run on the stream its tail ran on (the handle's stream, or
 *     mfx_synchronize with mfx_batch_overlap on).
 * NOT served: the session entries (mfx_sessions_*) and the streaming interface are untouched and ignore the VAD. */
enum { MFX_VAD_FLAGS = 0, MFX_VAD_SELECT = 1, MFX_VAD_PACK = 2 };
int mfx_batch_set_vad(mfx_handle *h, int32_t column, float energy_threshold, float energy_mean_scale, int32_t frames_context,
                      float proportion_threshold, int32_t mode);
int mfx_batch_clear_vad(mfx_handle *h);
int mfx_batch_vad_read(mfx_handle *h, uint8_t *flags /* [total_rows] */, int32_t *voiced /* [n_utt] */,
                       float *threshold /* [n_utt] */, int64_t *total_voiced);
int mfx_batch_vad_device(const mfx_handle *h, const uint8_t **d_flags, const int32_t **d_voiced,
                         const int64_t **d_packed_row0 /* [n_utt + 1] */);

/* Pitch track beside the feature rows of a batch run ("Pitch track"): what compute-kaldi-pitch-feats gives a
 * Kaldi-style recipe -- a normalised cross-correlation (NCCF) of the PCM over a range of lags and a Viterbi path through it --
 * on the device, from the PCM the batch already has there.  No reference analogue.  d_out, mfx_batch_output_width and every
 * existing row stay bit for bit what they are: the track goes to handle-owned arrays indexed by the plan's rows.
 *   Scope.  Valid after mfx_batch_plan / mfx_batch_plan_rates (MFX_ERR_STATE before one); a later plan drops the track with the
 *     other attachments, and mfx_batch_clear_pitch puts the handle back on today's launches.  MFX_ERR_DEVICE on a planning
 *     handle, before any argument is looked at.  MFX_ERR_CONFIG on an STFT log-mel handle (its frames are centred); MFCC,
 *     fbank, PLP and TRAPS handles are served, they share one frame rule.  MFX_ERR_ARG: window outside 32 .. 1024 (0 means the
 *     handle's window_size, which must then lie in that range); lag_min < 2, lag_max > 1024, or K = lag_max - lag_min + 1
 *     outside 1 .. 512; ballast, lag_cost or penalty not finite or negative, or lag_cost > 1; max_jump outside 0 .. 511 (0
 *     means J = K - 1, or 1 when K = 1; larger values are clamped to J = max(K - 1, 1)).
 *   Samples.  Utterance u has n samples per channel and T = mfx_batch_frames(h, n) frames at shift S; its rows are the
 *     plan's out_rows[u].  p[i] is the int16 sample, for channels = 2 the front ends' (L + R) >> 1; p[i] = 0 for i outside
 *     [0, n) of THAT utterance: a neighbour's samples are never read.  Under a rates plan the samples are the converted
 *     scratch's, which is what the front end reads.  x[i] = (float)p[i] * 2^-15.
 *   Frame t, span Ls = window + lag_max samples from i0 = t S:
 *     Mean.  sI = the sum of p[i0 .. i0 + Ls) as an exact integer; m = (float)sI * c1, c1 = (float)(1.0 / (32768.0 * Ls));
 *       z[j] = x[i0 + j] - m for all j < Ls, the zero-filled samples included.
 *     Energies.  q[j] = (double)(z[j] * z[j]), the product rounded to float32 first; P[0] = 0, P[j + 1] = P[j] + q[j]
 *       ascending, in double; e(l) = (float)(P[l + window] - P[l]).
 *     Correlation, for l_k = lag_min + k: c = 0, then for j = 0 .. window - 1 ascending c = fmaf(z[j], z[j + l_k], c): one
 *       float32 FMA chain per value, in that order, whatever the tiling and the batch.
 *     NCCF.  s = e(0) * e(l_k) + ballast, the product and the sum rounded separately; rho[k] = c / sqrtf(s) when s > 0, else
 *       0; the division and the square root correctly rounded.
 *   Track, per utterance.  Host tables, built in double and rounded once: wt[k] = (float)(1 - lag_cost * l_k / lag_max),
 *     lg[k] = (float)ln(l_k).  Every float32 operation below is rounded on its own.
 *     Local cost.  loc_t[k] = 1.0f - rho_t[k] * wt[k].
 *     Start.  a_0 = loc_0.  For every t: m_t = min_k a_t[k] and fwd_t[k] = a_t[k] - m_t.
 *     Step, for t >= 1 and each k, over k' from max(0, k - J) to min(K - 1, k + J) ascending: d = lg[k] - lg[k'],
 *       tr = (penalty * d) * d, cand = fwd_{t-1}[k'] + tr; a strictly smaller cand replaces the best, so ties keep the
 *       smallest k'.  a_t[k] = loc_t[k] + best, and bp_t[k] is that k'.
 *     Backtrace.  The end state is the smallest k that minimises fwd_{T-1}; bp is followed backwards from it.
 *     Outputs per row.  index = k_t; rho = rho_t[k_t]; lag = (float)l_{k_t} + delta, the parabolic refinement: if
 *       0 < k_t < K - 1, with a, b, c = rho_t[k_t - 1], rho_t[k_t], rho_t[k_t + 1] and den = (a - b) + (c - b): if den < 0,
 *       delta = clamp((0.5f * (a - c)) / den, -0.5f, 0.5f); in every other case delta = 0.  f0 is sample_rate / lag.
 *     All values are finite (|x| <= 1), and the outputs are an exact function of the utterance's samples and the parameters.
 *   Run.  While in force, mfx_batch_run_device / _host queue k_pitch_nccf and k_pitch_track on the handle's OWN stream,
 *     directly behind the front end's launches -- never on the tail's: with mfx_batch_overlap the caller may reuse the PCM
 *     once the handle's stream has passed it.  The run still allocates nothing.  The sliced host path stays on (utterances
 *     are independent: a slice runs its utterance range).
 *   Memory.  The setter allocates, after waiting for the handle's streams: the NCCF rows [total_rows][K] floats, the
 *     back-pointers [total_rows][K] uint16, pitch, index, the two tables and the tile descriptors -- about 1.7 GB for
 *     1000 x 10 s at K = 281.  MFX_ERR_DEVICE when it does not fit (nothing of it stays allocated then).
 *   Composition.  d_out, mfx_batch_output_width and every other attachment, in any combination, are unchanged.  The pitch
 *     arrays are indexed by the plan's rows, also under MFX_VAD_SELECT / MFX_VAD_PACK.
 *   Read-back.  mfx_batch_pitch_read synchronises and copies pitch [total_rows][2] = (lag, rho), index [total_rows] and the
 *     NCCF rows [total_rows][K]; any output may be NULL.  MFX_ERR_STATE without the attachment or before a run; a batch
 *     without rows counts as run.  mfx_batch_pitch_device returns the device arrays: valid until the next plan or clear,
 *     ordered on the handle's stream.
 * NOT served: the session entries (mfx_sessions_*) and the streaming interface are untouched and ignore the pitch track. */
int mfx_batch_set_pitch(mfx_handle *h, int32_t window, int32_t lag_min, int32_t lag_max, float ballast, float lag_cost,
                        float penalty, int32_t max_jump);
int mfx_batch_clear_pitch(mfx_handle *h);
int mfx_batch_pitch_read(mfx_handle *h, float *pitch /* [total_rows][2]: lag, rho */, int32_t *index /* [total_rows] */,
                         float *nccf /* [total_rows][K] */);
int mfx_batch_pitch_device(const mfx_handle *h, const float **d_pitch, const int32_t **d_index);

/* Kaldi's pitch features from the pitch track, and their paste into the rows of a batch run ("Pitch features"):
 * what process-kaldi-pitch-feats and paste-feats give a Kaldi-style recipe -- a probability-of-voicing feature, the log-pitch
 * with a POV-weighted sliding mean removed, a delta of the log-pitch, optionally the raw log-pitch -- on the device, from the
 * (lag, rho) rows k_pitch_track leaves there.  No reference analogue.
 *   Scope.  Valid while a pitch track is in force (mfx_batch_set_pitch): MFX_ERR_STATE otherwise, and before a plan.
 *     MFX_ERR_DEVICE on a planning handle, before any argument is looked at.  A later plan drops the attachment with the
 *     others; mfx_batch_clear_pitch drops it with the track; mfx_batch_clear_pitch_feats drops it alone.
 *   Arguments.  columns: MFX_PF_* bits, 0 means POV | NORM_LOG_PITCH | DELTA (Kaldi's default); F is the number of bits set,
 *     the columns are delivered in the order of the enum (Kaldi's).  left, right: 0 .. 1024 rows of the normalisation window
 *     (Kaldi: 75, 75, its normalization-left-context / -right-context).  delta_window D: 1 .. 16 (Kaldi: 2).  The four
 *     scales must be finite (Kaldi: pov_scale 2, pov_offset 0, pitch_scale 2, delta_scale 10).  paste: 0 or 1.  Anything else
 *     is MFX_ERR_ARG, and nothing changes.
 *   Per utterance of T rows (lag_t, rho_t).  Every operation is in double and rounded on its own (no contraction); an
 *     output is (float) of the double.
 *       n = min(1, max(-1, (double)rho_t)), a = |n|
 *       r = -5.2 + 5.4 exp(7.5 (a - 1)) + 4.8 a - 2 exp(-10 a) + 4.2 exp(20 (a - 1)), summed left to right;
 *       w_t = 1 / (1 + exp(-r))   (Kaldi's NccfToPov; in (0, 1): no window is empty of weight)
 *       p_t = ln((double)sample_rate / (double)lag_t)
 *     POV             pov_scale * (pow(1.0001 - n, 0.15) - 1) + pov_offset
 *     NORM_LOG_PITCH  lo = max(0, t - left), hi = min(T - 1, t + right); over i = lo .. hi ascending sw += w_i and
 *                     sp += w_i * p_i -- direct sums per row, not running sums: a row does not depend on any tiling --
 *                     and the value is pitch_scale * (p_t - sp / sw)
 *     DELTA           the library's own regression: num = sum over l = 1 .. D ascending of
 *                     l * (p[min(T - 1, t + l)] - p[max(0, t - l)]), edges replicated as in the delta stage; the value is
 *                     (delta_scale * num) / (2 sum of l^2)
 *     RAW_LOG_PITCH   p_t
 *     A row is a function of its own utterance's track and the parameters only.  exp, ln and pow are the platform's: the
 *     device and mfx_host_pitch_feats agree to within the functions' errors, not bit for bit (tests/pitchfeat_ref.py bounds
 *     it).
 *   NOT served: Kaldi's random delta-pitch-noise-stddev (the DELTA column has no noise added), and its online mode, whose
 *     normalisation window is not symmetric and grows with the stream (normalization-left-context frames behind a lookahead).
 *   Run.  k_pitch_feats runs on the handle's own stream directly behind k_pitch_track; it fills feats [total_rows][F], a
 *     handle-owned array indexed by the plan's rows in every mode, as the pitch arrays are.
 *   Paste.  With paste = 1 the rows y of a run -- behind the deltas and every normaliser, ahead of the transform and the VAD --
 *     become [ y (Wd columns) | feats (F columns) ], of width Wy = Wd + F; k_pitch_paste writes them on the stream the tail
 *     runs on, as the last launch ahead of the transform.  mfx_batch_output_width becomes Wy (out_dim under a transform);
 *     mfx_batch_set_transform takes in_dim = (left + right + 1) * Wy and splices the wide rows; the VAD reads its column among
 *     the first Wd columns and, in SELECT / PACK, moves the wide rows; mfx_batch_run_host sizes by the new width.  The first
 *     Wd columns are bit for bit what the handle delivers without the paste, and every placement guarantee of
 *     mfx_batch_run_device holds for the wide rows.  A call that would change Wy -- setting or clearing with paste, changing F
 *     under paste, mfx_batch_clear_pitch under paste -- answers MFX_ERR_STATE while a transform or a VAD is in force: clear
 *     them, set the paste, set them again.  With paste = 0 nothing outside the feats array changes.
 *   Memory.  The setter allocates, after waiting for the handle's streams: the feats array, its tile descriptors and, under
 *     paste, a scratch [total_rows][Wd] for the narrow rows.  The run still allocates nothing.
 *   Read-back.  mfx_batch_pitch_feats_read synchronises and copies feats [total_rows][F].  MFX_ERR_STATE without the
 *     attachment or before a run; a batch without rows counts as run.  mfx_batch_pitch_feats_device returns the device array
 *     and F: valid until the next plan, set or clear, ordered on the handle's stream.
 * NOT served: the session entries (mfx_sessions_*) and the streaming interface ignore the attachment. */
enum { MFX_PF_POV = 1, MFX_PF_NORM_LOG_PITCH = 2, MFX_PF_DELTA = 4, MFX_PF_RAW_LOG_PITCH = 8 };
int mfx_batch_set_pitch_feats(mfx_handle *h, int32_t columns, int32_t left, int32_t right, int32_t delta_window,
                              float pov_scale, float pov_offset, float pitch_scale, float delta_scale, int32_t paste);
int mfx_batch_clear_pitch_feats(mfx_handle *h);
int mfx_batch_pitch_feats_read(mfx_handle *h, float *feats /* [total_rows][F] */);
int mfx_batch_pitch_feats_device(const mfx_handle *h, const float **d_feats, int32_t *F);

/* Dense padded tensor output of a batch run ("Tensor output"): what pad_sequence, a transpose and a cast to half
 * or bfloat16 make of the ragged rows, written by one launch as the last stage of the run.  No reference analogue: a neural
 * model's input.
 *   Definition.  B = the planned utterance count; Wo = mfx_batch_output_width (out_dim under a transform, the wide rows under
 *     a pitch paste); y_u[t][c] = what the run delivers today at row out_rows[u] + t, behind everything, the transform and the
 *     VAD included.  L_u = T_u, the plan's frame count; under MFX_VAD_SELECT, voiced[u] of this run.  Tp = t_pad when t_pad > 0,
 *     else the largest T_u of the whole plan: fixed when the setter is called; it may be 0.  len_u = min(L_u, Tp): a longer
 *     utterance is cut to its first Tp rows.  Element (u, t, c) = cvt(y_u[t][c]) for t < len_u, else cvt(pad_value), at index
 *       MFX_TENSOR_TIME_MAJOR     (u * Tp + t) * Wo + c      the tensor is [B][Tp][Wo]
 *       MFX_TENSOR_CHANNEL_MAJOR  (u * Wo + c) * Tp + t      the tensor is [B][Wo][Tp]
 *     in 64-bit arithmetic.
 *   Conversion.  MFX_DTYPE_F32 delivers the bits as they are.  MFX_DTYPE_F16 (IEEE binary16) and MFX_DTYPE_BF16 round to
 *     nearest, ties to even (IEEE 754 roundTiesToEven): overflow gives +-inf, results in the subnormal range are produced, not
 *     flushed, the sign of zero is kept, a NaN becomes a NaN (its payload is not pinned).
 *   Write guarantee.  Every element of the tensor is written on every run: the caller never has to clear it.  Nothing outside
 *     [d_out, d_out + mfx_batch_output_bytes) is written.  d_out needs only the alignment of the element (4, 2 or 2 bytes); the
 *     bits are the same wherever it lies and on a second run.
 *   Whisper.  A Whisper encoder wants [80][3000] from audio zero-padded to 30 s.  A constant pad value does not reproduce that
 *     (MFX_LOGMEL_WHISPER's clamp follows the utterance's maximum, and the last frames reflect the audio's right end): callers
 *     who need exactly that pad the AUDIO.  Everyone else -- conformer / wav2vec-style front ends, vocoders, taggers -- pads the
 *     features.
 *   Scope.  Valid after mfx_batch_plan / mfx_batch_plan_rates (MFX_ERR_STATE before one); a later plan drops the tensor with the
 *     other attachments, and mfx_batch_clear_tensor puts the handle back on today's launches and bits.  MFX_ERR_DEVICE on a
 *     planning handle, before any argument is looked at (all entries below).  MFX_ERR_ARG: an unknown layout or dtype, t_pad
 *     outside 0 .. 2^24 (or, with t_pad = 0, a T_u beyond it).  pad_value is not inspected.  MFX_ERR_CONFIG: CHANNEL_MAJOR at an
 *     output width whose tile does not fit the LDS (never at Wo <= 256): there is never a failed launch.
 *     The tensor is set LAST: while it is in force mfx_batch_set_transform, mfx_batch_set_vad, mfx_batch_clear_vad and the
 *     pitch-feats calls that would change the row width answer MFX_ERR_STATE ("clear the tensor first").  The setter itself
 *     answers MFX_ERR_STATE under MFX_VAD_PACK: packed rows have no per-utterance place.  A float32 scratch [total_rows][Wo]
 *     that the run's last stage writes in the place of d_out (grown, never shrunk), len [B] and the utterance table k_tensor_pack
 *     reads are allocated HERE (the call waits for the handle's streams); mfx_batch_run_device still allocates nothing.
 *   Composition.  Everything else in a run is unchanged -- front end, MFX_ENGINE_* bits, alpha list, rates plan, speakers,
 *     online normaliser, pitch, mfx_batch_overlap.  The one launch of k_tensor_pack goes on the stream the tail runs on, as the
 *     transform and the VAD do.  mfx_batch_run_device's d_out is then the tensor (the float pointer is a formality), and so is
 *     mfx_batch_run_host's out: mfx_batch_output_bytes of it.  The host entry keeps its sliced path: an utterance's block of the
 *     tensor is contiguous in both layouts.
 *   Read-back.  mfx_batch_output_bytes: what a run writes at d_out -- the tensor's bytes, else total_rows * Wo * 4.
 *     mfx_batch_tensor_shape: dims = {B, Tp, Wo} or {B, Wo, Tp} and the element's bytes (MFX_ERR_STATE without a tensor).
 *     mfx_batch_tensor_lengths synchronises and returns len [B] and / or the handle-owned device array (valid until the next plan,
 *     set or clear; written by the run, ordered as mfx_batch_vad_device's arrays are): MFX_ERR_STATE without a tensor, or before
 *     a run when a selecting VAD decides the lengths.
 *   A second format.  mfx_batch_tensor_from_rows queues the one launch alone, on the handle's stream, over the caller's device
 *     rows [total_rows][Wo] in the plan's row order (4-byte aligned), with L_u = T_u: a second layout or type from rows the
 *     caller already has.  MFX_ERR_STATE without a tensor or while a VAD is in force.
 * NOT served: the session entries (mfx_sessions_*) and the streaming interface ignore the attachment. */
enum { MFX_TENSOR_TIME_MAJOR = 0 /* [B][Tp][Wo] */, MFX_TENSOR_CHANNEL_MAJOR = 1 /* [B][Wo][Tp] */ };
enum { MFX_DTYPE_F32 = 0, MFX_DTYPE_F16 = 1, MFX_DTYPE_BF16 = 2 };
int mfx_batch_set_tensor(mfx_handle *h, int32_t layout, int32_t dtype, int32_t t_pad, float pad_value);
int mfx_batch_clear_tensor(mfx_handle *h);
int64_t mfx_batch_output_bytes(const mfx_handle *h);      /* what a run writes at d_out: tensor bytes, else total_rows * Wo * 4 */
int mfx_batch_tensor_shape(const mfx_handle *h, int64_t dims[3], int32_t *elem_bytes);
int mfx_batch_tensor_lengths(mfx_handle *h, int32_t *len /* [B] or NULL */, const int32_t **d_len /* or NULL */);
int mfx_batch_tensor_from_rows(mfx_handle *h, const float *d_rows, void *d_out);

/* ---- sample-rate conversion in front of a batch ("Sample-rate conversion").  No reference analogue: the
 *      reference refuses a file whose rate differs from the first file's (ASR_OCL.cpp:191). ----
 *
 * Utterance u arrives at r_in = rates_hz[u] Hz (an integer); the rate the features are extracted at is r_out =
 * mfx_config.sample_rate, which must be an integral value.  g = gcd(r_in, r_out), L = r_out / g, M = r_in / g.
 *   Pass-through.  An utterance with r_in == r_out is copied, sample for sample.
 *   Length.  N_in samples per channel give N_out = ceil(N_in L / M) (int64 arithmetic; 0 gives 0).
 *   Filter.  A Hann-windowed sinc, evaluated in double on the host and rounded once to float32: rolloff in (0, 1] (0 means
 *     0.99), zeros in 1 .. 64 (0 means 6); c = rolloff min(1, L / M), Wh = ceil(zeros / c), P = 2 Wh taps per phase.  For
 *     phase phi in [0, L) and tap k in [0, P): t = (k - Wh + 1) - phi / L,
 *     h[phi][k] = c sinc(c t) (1 + cos(pi t / Wh)) / 2 for |t| < Wh, else 0; sinc(x) = sin(pi x) / (pi x), sinc(0) = 1.
 *     No per-phase renormalisation (the phase sums are 1 to within the window's ripple).  Table layout [L][P].
 *   Output sample j of an utterance, 0 <= j < N_out: n = (j M) div L, phi = (j M) mod L (int64);
 *     acc = 0; for k = 0 .. P - 1 ascending: acc = fmaf(h[phi][k], (float)x[n - Wh + 1 + k], acc);
 *     y[j] = clamp(rintf(acc), -32768, 32767) as int16.  x outside [0, N_in) of THAT utterance and channel is 0, never a
 *     neighbour's samples.  One float32 FMA chain in a fixed order: the bits of y do not depend on the tiling, on the other
 *     utterances of the batch, or on the alignment of the source.
 *   Stereo (channels = 2): each channel is converted on its own and the result is stored interleaved; the (L+R)>>1 downmix
 *     stays in the front ends.
 *   Limits (MFX_ERR_ARG with a message on the handle): rates in 1000 .. 768000 Hz, L <= 4096, P <= 4096, L P <= 2^20
 *     floats, at most 16 distinct input rates per plan.
 *
 * mfx_batch_plan_rates is mfx_batch_plan with offsets and lengths in INPUT-RATE samples per channel and one input rate per
 * utterance; out_rows / total_rows follow from the converted lengths, T_u = mfx_batch_frames(h, N_out_u).  It builds and
 * uploads the tap tables and tile descriptors and allocates a handle-owned int16 scratch for the converted PCM: every
 * utterance starts at an even sample offset, in ascending utterance order, and the scratch is padded at its end (the front
 * ends' "32-bit word that holds the last sample" rule holds); mfx_batch_run_device still allocates nothing.  A later
 * mfx_batch_plan or mfx_batch_plan_rates replaces the plan and drops the converter.  mfx_batch_set_alphas,
 * mfx_batch_set_transform and mfx_batch_overlap work after it exactly as after mfx_batch_plan.  MFX_ERR_DEVICE on a planning
 * handle; MFX_ERR_CONFIG when sample_rate is not integral; like mfx_batch_plan it does not need the window yet (the run
 * returns MFX_ERR_STATE before mfx_set_window).
 * While a rates plan is in force, mfx_batch_run_device / mfx_batch_run_host take pcm_samples_total and check their bounds
 * against the INPUT array (4-byte aligned as always; utterances may start at odd input offsets), convert d_pcm -> scratch
 * with ONE launch of k_resample over the utterance range being run, and then do exactly what they do today with the scratch
 * and its layout in the place of the caller's array.  The sliced host path cuts the input array by utterance, in input-rate
 * samples.
 * mfx_batch_resample_layout: the scratch layout in output-rate samples per channel (what a second handle needs to be planned
 * on the converted PCM, which mfx_debug_read kind 8 returns); MFX_ERR_STATE without a rates plan.
 * NOT served: the session entries (mfx_sessions_*) and the streaming interface are untouched and ignore a rates plan.  The
 * session entries have rates of their own: mfx_sessions_set_rates / mfx_sessions_select_rate below. */
int mfx_batch_plan_rates(mfx_handle *h, int32_t n_utt, const int64_t *offsets, const int64_t *lengths, const int32_t *rates_hz,
                         int32_t zeros, float rolloff, int64_t *out_rows, int64_t *total_rows);
int mfx_batch_resample_layout(const mfx_handle *h, int64_t *offsets, int64_t *lengths, int64_t *total);

/* Opt-in pipelining of consecutive batches: with enable=1 the delta / normalisation tail of a batch runs
 * on a second internal stream, so it overlaps the front end of the NEXT mfx_batch_run_device call.
 * Results of a batch are then complete only after mfx_synchronize() (or a device-wide synchronise),
 * not in order on the handle's stream.  Off by default (strict stream order). */
int mfx_batch_overlap(mfx_handle *h, int enable);

/* Convenience: same, from/to HOST buffers (pinned staging + H2D, run, D2H, synchronises). */
int mfx_batch_run_host(mfx_handle *h, const int16_t *pcm, int64_t pcm_samples_total, float *out);

/* ---- session entries: many OPEN streams, each advanced by one piece of samples per push, all in one launch sequence
 *      ("Session entries").  No reference analogue: its thread loop is sequential (ASR_OCL.cpp:365-366). ----
 *
 * A handle owns up to n_sessions sessions, numbered 0 .. n_sessions-1; a session is one open stream.  Let n be the samples
 * (per channel) a session has received since it was opened, T(n) = mfx_batch_frames(h, n) and D = delta_l1 + delta_l2 (0
 * with dyn = NONE).  After every push the session has delivered rows [0, E) of its utterance:
 *   E = max(0, T(n) - D) while the stream is open;
 *   E = T(n)             once a push is marked final (it may carry zero new samples: the flush).
 * The E_new - E_old rows a push delivers are THE SAME BITS that mfx_batch_run_device writes for that utterance as a whole
 * (planned at an even offset) on a handle of the same configuration and mfx_set_alpha, however the stream was cut into
 * pushes: shorter than a hop, completing no frame, empty, one sample, at odd offsets of the caller's array.  First- and
 * last-frame replication happens at the true start and end of the stream only (mfcccpu.cpp:243-254).  After a final push
 * the session is fresh and its id may be reused at once.  Every frame's static row is computed ONCE: a session carries
 * static rows (at most 2 D) and fewer than window + shift samples, never PCM context to re-transform.
 *
 * mfx_sessions_create sizes everything (two slot arrays, descriptor buffers, pinned descriptor staging) for n_sessions
 * sessions and pieces of at most max_push_samples samples per channel; called again it re-sizes after a synchronise and
 * drops all state; (0, 0) releases everything.  mfx_sessions_reset drops the carried state of one session (-1: of all) and
 * any pending plan.  mfx_sessions_plan describes one push as mfx_batch_plan describes a batch: session ids[i] receives
 * samples [offsets[i], offsets[i] + lengths[i]) of the caller's ONE PCM array (per channel; interleaved for channels = 2),
 * final_flags[i] != 0 ends its stream (NULL: none final); out_counts[i] rows will be delivered to rows out_rows[i] ..
 * (prefix sum) of d_out [total_rows][mfx_get_output_data_width].  A plan changes no session state; a second plan replaces
 * the first.  mfx_sessions_run_device queues gather -> front end -> delta on the handle's stream, asynchronously, allocates
 * nothing, and commits the sessions' state once its launches are queued; without a pending plan, or twice for one plan, it
 * returns MFX_ERR_STATE.  mfx_sessions_run_host is the same from / to host buffers (it synchronises, and may grow its
 * device copies).  mfx_sessions_delivered: E so far (0 for a fresh session).
 * As for mfx_batch_run_device, d_out may have any 4-byte alignment and may lie anywhere in a device allocation: the rows are
 * the same bits wherever it lies, and nothing outside [d_out, d_out + total_rows * width) is written.
 * Errors: MFX_ERR_ARG an id outside the range or twice in one push, a negative length or offset, a piece past
 * pcm_samples_total, a misaligned d_pcm (the 4-byte rule of mfx_batch_run_device); MFX_ERR_BUFFER_TOO_SMALL lengths[i] >
 * max_push_samples; MFX_ERR_STATE no mfx_set_window yet, no mfx_sessions_create yet, a TRAPS handle, a handle with norm !=
 * MFX_NORM_NONE without mfx_sessions_set_online_norm (the one normaliser the session entries serve is the online CMN / CVN
 * above; MINMAX never); MFX_ERR_DEVICE a planning handle.
 * The handle's mfx_set_alpha factor applies to all sessions.  NOT applied to session runs: mfx_batch_set_alphas,
 * mfx_batch_overlap, MFX_ENGINE_FUSE_DELTA.  The transform of mfx_batch_set_transform belongs to the batch plan and is not
 * applied either; the same stage is served through mfx_sessions_set_transform below.  A push leaves the batch plan (with its
 * alpha list and transform) and the streaming state of the same handle untouched, and they leave the sessions untouched. */
int mfx_sessions_create(mfx_handle *h, int32_t n_sessions, int32_t max_push_samples);
int mfx_sessions_reset(mfx_handle *h, int32_t session);
int mfx_sessions_plan(mfx_handle *h, int32_t n, const int32_t *ids, const int64_t *offsets, const int64_t *lengths,
                      const int32_t *final_flags, int64_t *out_rows, int32_t *out_counts, int64_t *total_rows);
int mfx_sessions_run_device(mfx_handle *h, const int16_t *d_pcm, int64_t pcm_samples_total, float *d_out);
int mfx_sessions_run_host(mfx_handle *h, const int16_t *pcm, int64_t pcm_samples_total, float *out);
int64_t mfx_sessions_delivered(const mfx_handle *h, int32_t session);

/* ---- session transform: splice + affine transform as the last stage of a push ("Session transform") ----
 *
 * The semantics are exactly those of mfx_batch_set_transform: with y[t] the rows a session delivers without it (width Wd =
 * mfx_get_output_data_width, after the deltas and after the online normaliser if one is set), C = left + right + 1 and in_dim
 * = C * Wd,
 *   z[t]      = [ y[clamp(t - left, 0, T - 1)] | ... | y[clamp(t + right, 0, T - 1)] ]     (T: the rows of the whole STREAM)
 *   out[t][r] = b_x[r], then for i = 0 .. in_dim - 1 ascending: fmaf(A_x[r][i], z[t][i], .)      (float32, one FMA per tap)
 * with x the session's transform (mfx_sessions_select_transform; default 0).  A is [n_xf][out_dim][in_dim] row-major, b
 * [n_xf][out_dim] or NULL (zeros).
 * Delivery rule.  right > 0 needs look-ahead.  Let Ey be the E of the session entries above (max(0, T(n) - D) while the
 * stream is open, T(n) once final).  A session with a transform has delivered rows [0, Ex):
 *   Ex = max(0, Ey - right) while the stream is open;
 *   Ex = Ey = T(n)          once a push is final.
 * mfx_sessions_delivered returns Ex, out_counts[i] = Ex_new - Ex_old, and d_out is [total_rows][out_dim]
 * (mfx_sessions_output_width).  The right clamp happens only on a final push, the left clamp only at the true start of the
 * stream.  A push may deliver 0 rows; a flush delivers up to right + D rows with no new samples.
 * Contract.  The rows a session delivers are THE SAME BITS that mfx_batch_run_device writes for the whole utterance on a
 * handle of the same configuration with mfx_batch_set_transform(left, right, out_dim, ..., utt_xf[u] = the session's x):
 * however the stream is cut, in the matrix and the vector form (MFX_ENGINE_XFORM_VALU applies here too), with or without
 * MFX_ENGINE_SESS_XFORM_PLAIN, wherever d_out lies (any 4-byte alignment); nothing outside [d_out, d_out + total_rows *
 * out_dim) is written.
 * State.  mfx_sessions_set_transform / mfx_sessions_clear_transform are valid only while no sessions exist (before
 * mfx_sessions_create, or after mfx_sessions_create(h, 0, 0)), else MFX_ERR_STATE.  The setter stores the matrices as the
 * kernels read them and allocates nothing on the device; mfx_sessions_create sizes and uploads everything (two more slot
 * arrays of left + right + frames_max + D rows of Wd floats per session, n_xf * out_dim * in_dim operand floats rounded up to
 * the kernels' tiles), mfx_sessions_run_device still allocates nothing and queues ONE launch more, and
 * mfx_sessions_create(h, 0, 0) releases the device parts.  A session carries at most left + right finished rows y from push
 * to push; mfx_sessions_reset drops them with the rest.  Without a session transform every session entry does exactly what it
 * did before.  The batch plan's transform and the streaming state of the same handle are untouched and leave the session
 * transform untouched.
 * mfx_sessions_select_transform(h, session, x): the session's transform.  The choice stays with the id across final pushes
 * and mfx_sessions_reset; mfx_sessions_create puts all back to 0.  It drops a pending plan.  MFX_ERR_STATE without a transform
 * or without sessions, or when the session is not fresh (it has received samples since its last final push or reset);
 * MFX_ERR_ARG for an id or x out of range.
 * Errors of the setter: MFX_ERR_ARG left / right outside 0 .. 32, out_dim outside 1 .. 256, n_xf outside 1 .. 1024, in_dim >
 * 8192, A == NULL; MFX_ERR_CONFIG no block tiling fits the LDS (the launchers' own rule; cannot happen inside the limits
 * above); MFX_ERR_DEVICE a planning handle, before any argument is looked at (all four entries). */
int mfx_sessions_set_transform(mfx_handle *h, int32_t left, int32_t right, int32_t out_dim, int32_t n_xf, const float *A,
                               const float *b);
int mfx_sessions_clear_transform(mfx_handle *h);
int mfx_sessions_select_transform(mfx_handle *h, int32_t session, int32_t xf);
/* out_dim while a session transform is set, else mfx_get_output_data_width */
int mfx_sessions_output_width(const mfx_handle *h);

/* ---- session rates: per-session sample-rate conversion in front of a push ("Session sample-rate conversion") ----
 *
 * A session arrives at r_in = rates_hz[its rate index] Hz (mfx_sessions_select_rate; default index 0); r_out =
 * mfx_config.sample_rate, g, L, M, the filter h[phi][k], Wh, P, zeros and rolloff are those of mfx_batch_plan_rates above.
 *   Converted sample.  Output sample j of a STREAM is the batch definition, unchanged: n = (j M) div L, phi = (j M) mod L;
 *     acc = 0; for k = 0 .. P - 1 ascending: acc = fmaf(h[phi][k], (float)x[n - Wh + 1 + k], acc);
 *     y[j] = clamp(rintf(acc), -32768, 32767).  x outside [0, N_in) of the stream is 0; the right zero fill happens only once
 *     the stream is final.
 *   Delivery rule.  After a session has received N input samples (per channel) it has converted samples [0, J):
 *     J = max(0, ceil((N - Wh) L / M)) while the stream is open: the outputs whose last tap n + Wh has arrived;
 *     J = ceil(N L / M)                once a push is final.
 *     A pass-through session (r_in == r_out) has J = N throughout: its samples are taken as they are.
 *   Everything behind the converter is the session contract above with n = J: T(J) = mfx_batch_frames(h, J), E, Ex, the online
 *     normaliser and the session transform are unchanged.  A flush (final push, no new samples) also converts the stream's last
 *     ceil(N L / M) - J samples before it delivers the tail rows.
 *   Contract.  The converted samples and the rows of a stream are THE SAME BITS that mfx_batch_run_device produces for the whole
 *     utterance on a handle of the same configuration under mfx_batch_plan_rates(..., rates_hz[u] = r_in, zeros, rolloff): the
 *     converted samples are that handle's mfx_debug_read kind 8, the rows its rows (with the same online normaliser and
 *     transform), however the stream is cut: pushes of 0 or 1 samples, pushes shorter than Wh, pieces at odd offsets of the
 *     caller's array, mono or stereo (each channel converted on its own, interleaved; the (L+R)>>1 downmix stays in the
 *     front ends).
 *   Units.  While rates are set, max_push_samples of mfx_sessions_create, offsets and lengths of mfx_sessions_plan and
 *     pcm_samples_total of the run entries are in INPUT-rate samples per channel of the caller's one array (4-byte aligned as
 *     always; pieces may sit at odd offsets).  MFX_ERR_BUFFER_TOO_SMALL: lengths[i] > max_push_samples; MFX_ERR_ARG: a piece past
 *     pcm_samples_total.
 * State.  mfx_sessions_set_rates / mfx_sessions_clear_rates are valid only while no sessions exist, else MFX_ERR_STATE.  The
 * setter builds the tap tables on the host (the code of mfx_batch_plan_rates) and allocates nothing on the device;
 * mfx_sessions_create sizes and uploads everything -- the tables, two carry slot arrays of max over rates (2 Wh + M div L + 2)
 * samples per channel and session (rounded up to 8), an int16 scratch of one converted piece per session, and every slot of the
 * session entries for the largest converted piece, max over rates ceil((max_push_samples + Wh) L / M) + 1 (MFX_ERR_ARG when that
 * exceeds 2^24) -- mfx_sessions_run_device still allocates nothing and queues ONE launch more (k_sess_resample, ahead of the
 * gather), and mfx_sessions_create(h, 0, 0) releases the device parts.  A session carries at most 2 Wh - 1 input samples per
 * channel from push to push; a final push and mfx_sessions_reset leave it fresh.  A push whose pieces are all pass-through (or
 * bring nothing) queues no conversion launch and reads the caller's array directly.  Without mfx_sessions_set_rates every
 * session entry does exactly what it did before.  The batch rates plan and the session rates are strangers: neither reads or
 * changes the other.
 * mfx_sessions_select_rate(h, session, i): the session's rate.  The choice stays with the id across final pushes and
 * mfx_sessions_reset; mfx_sessions_create puts all back to 0.  It drops a pending plan.  MFX_ERR_STATE without rates or without
 * sessions, or when the session is not fresh; MFX_ERR_ARG for an id or index out of range.
 * Errors of the setter: MFX_ERR_ARG n_rates outside 1 .. 16, rates_hz == NULL, and the limits of mfx_batch_plan_rates (rates in
 * 1000 .. 768000 Hz, L <= 4096, P <= 4096, L P <= 2^20, zeros in 0 .. 64, rolloff in [0, 1]); MFX_ERR_CONFIG a sample_rate that
 * is not integral; MFX_ERR_DEVICE a planning handle, before any argument is looked at (all entries).
 * mfx_sessions_converted_read (test / inspection aid; it synchronises): the converted samples of the last push that ran, piece
 * by piece in the plan's order, back to back in dst (interleaved for channels = 2); offsets[i] / lengths[i] (either may be NULL)
 * are piece i's place in dst in samples per channel.  Returns the int16 elements written (dst == NULL: needed);
 * MFX_ERR_BUFFER_TOO_SMALL when cap_elems is less; MFX_ERR_STATE without rates or sessions, or when the last push queued no
 * conversion launch (its samples are the caller's own). */
int mfx_sessions_set_rates(mfx_handle *h, int32_t n_rates, const int32_t *rates_hz, int32_t zeros, float rolloff);
int mfx_sessions_clear_rates(mfx_handle *h);
int mfx_sessions_select_rate(mfx_handle *h, int32_t session, int32_t rate_index);
int64_t mfx_sessions_converted_read(mfx_handle *h, int16_t *dst, int64_t cap_elems, int64_t *offsets, int64_t *lengths);

/* Page-locked host memory for the caller's PCM / feature buffers (mfx_batch_run_host and the streaming entries DMA
 * straight from / to such buffers; pageable ones go through the handle's staging).  NULL on failure. */
void *mfx_alloc_pinned(size_t bytes);
void mfx_free_pinned(void *p);

/* ---- stream / timing plumbing ---- */
/* Use an existing hipStream_t (e.g. torch's current stream) instead of the handle's own. */
int mfx_set_stream(mfx_handle *h, void *hip_stream);
int mfx_synchronize(mfx_handle *h);
/* HIP-event timing of the dominant kernel over the launches since the last reset: number of
 * launches and their summed device time in milliseconds (events recorded on the handle's stream
 * around that kernel only).  enable=1 turns recording on; it is off by default. */
int mfx_profile_enable(mfx_handle *h, int enable);
int mfx_profile_read(mfx_handle *h, int32_t *launches, double *kernel_ms, int reset);
/* name of the dominant (front-end) kernel of the batch entries as it appears in rocprofv3's kernel trace: what the ONE
 * dispatch rule of the library (choose_front, mfx_api.cpp) picks for this handle */
const char *mfx_dominant_kernel_name(const mfx_handle *h);
/* The fused delta stage of the 512-point batch path (k_front512's FUSE builds; unstable, like the MFX_ENGINE_* bits that steer
 * it).  Without MFX_ENGINE_FUSE_DELTA it runs on planned batches of *min_frames .. *max_frames frames with nothing attached and no
 * overlap in force (measured: it wins on a batch of a million frames and loses on one of twelve); with it, on every batch that qualifies; with MFX_ENGINE_NO_FUSE_DELTA never.  *planned: 1 when the current
 * plan carries the fused form's block lists; *runs: fused launches since the handle was created (a run that took the separate
 * delta kernel does not count); *share: what such a launch does with the block's tiles -- 0 the delta wave alone, 1 shared
 * with front-end waves that have run out of frames, 2 those waves take every tile.  Any pointer may be null. */
int mfx_batch_fuse_info(const mfx_handle *h, int32_t *planned, int32_t *share, int64_t *runs, int64_t *min_frames,
                        int64_t *max_frames);
/* Host restatements of what the kernel and the planner share (mfx_kernels.h).  LDS floats of a delta tile staged `rows` rows
 * at a time; *shares: 1 when a 16-row sub-tile at these orders fits a wave's frame slots (else tiles are not shared). */
int32_t mfx_host_delta_tile_lds_floats(int32_t rows, int32_t l1, int32_t l2, int32_t *shares);
/* The claim word of a block's tile list.  word < 0: the initial word of a list of *tile tiles.  Else one claim from the head
 * (from_head != 0) or the tail: the word after it, *tile = the tile claimed, or -1 with the word unchanged once the list is
 * exhausted. */
int64_t mfx_host_fuse_claim(int64_t word, int32_t from_head, int32_t *tile);
/* A PLANNING handle: mfx_create's own configuration checks, host-built tables and LDS sums with every device call left
 * out -- it answers mfx_dominant_kernel_name and the geometry accessors (mfx_get_output_data_width,
 * mfx_get_input_buffer_size, mfx_estimated_window_count, mfx_max_frames_out, mfx_fft_size) without a GPU and computes
 * nothing; every other entry fails on it with MFX_ERR_DEVICE.  The shape -> kernel table of DESIGN.md is pinned through it
 * (tests/test_host.py).  The reference has no analogue: it chooses its back end by a CLI switch (ASR_OCL.cpp:132-146).
 * mfx_plan_set_aligned: whether the batch's frames lie on aligned sample pairs (mfx_batch_plan derives that from the
 * caller's offsets on a real handle; default 1). */
int mfx_plan_create(const mfx_config *cfg, mfx_handle **out);
int mfx_plan_set_aligned(mfx_handle *h, int aligned);

/* ---- host-side table builders (no device needed; the same code fills the tables the kernels
 *      read, exposed so that CPU-only tests can compare them with the oracle bit for bit) ---- */
/* mel table of MfccCpu::refresh_filters (mfcccpu.cpp:24-60): weights [2][fft_size], beg [num_banks+2] */
int mfx_host_mel_table(int32_t num_banks, int32_t fft_size, float sample_rate, float low_freq, float high_freq,
                       float alpha, float *weights, int32_t *beg);
/* DCT-II + lifter matrix (mfcccpu.cpp:118-136): [num_banks][ceps_len + (want_c0 ? 1 : 0)] */
int mfx_host_dct_matrix(int32_t num_banks, int32_t ceps_len, int32_t want_c0, float lift_coef, float *matrix);
/* Lane plan of the mel walk of the fused kernels (lanes = 16: 512-point kernel, and with fft_size = 1024 the short-window
 * 1024-point kernel, whose starts are multiples of 4 bins; lanes = 64: long-transform kernel): filters dealt to the lanes
 * in rounds, longest first; returns the number of rounds.  Test / inspection aid. */
int mfx_host_mel_lane_plan(int32_t lanes, int32_t num_banks, int32_t fft_size, const float *weights, const int32_t *beg,
                           int32_t max_read_bin, int32_t *L, int32_t *row_stride, int32_t *start, int32_t *fid, float *w,
                           int64_t w_cap);
/* Operands of the DCT on the matrix pipe, [tile][K step][lane]; returns their count.  Test / inspection aid. */
int64_t mfx_host_dct_mfma_operands(int32_t num_banks, int32_t dct_len, const float *matrix, float *out, int64_t out_cap,
                                   int32_t *tiles, int32_t *ksteps);
/* One push of one session under a session transform, exactly as the planner derives it (mfx_host_session_step's companion).
 * state = {Ey, Ex}: finished rows y, transformed rows delivered; n_y: the rows y this push completes (mfx_host_session_step's
 * result).  Returns the rows delivered and advances the state ({0, 0} after a final push).  carry_rows: rows y carried in from
 * the previous slot (<= left + right); the push's slot holds carry_rows + n_y rows.  win = {src_row0, lo, hi}: output row r
 * reads slot rows src_row0 + clamp(r - left + c, lo, hi), c <= left + right (k_splice_affine's convention: src_row0 is the
 * slot row of y[Ex_old], lo is negative by the carried rows in front of it).  MFX_ERR_ARG on a bad argument. */
int32_t mfx_host_session_xform_step(int32_t left, int32_t right, int64_t state[2], int32_t n_y, int32_t final_flag,
                                    int32_t *carry_rows, int32_t win[3]);
/* UNSTABLE test / inspection aid: the work list of k_sess_xform for pieces that deliver n_out[i] rows with transform xf[i], at
 * G = 4, 2 or 1 row groups per block.  groups [.][3] = (piece, first row, rows <= 16), sorted by transform; blocks [.][3] =
 * (first group, groups <= G, transform).  Returns the number of groups, *n_blocks the number of blocks; either array may be
 * NULL (count only), MFX_ERR_ARG when one is too small. */
int32_t mfx_host_sess_xform_groups(int32_t n, const int32_t *n_out, const int32_t *xf, int32_t G, int32_t *groups,
                                   int32_t groups_cap, int32_t *blocks, int32_t blocks_cap, int32_t *n_blocks);
/* PLP tables as uploaded (PLP): equal-loudness weights eql [num_banks] at the (warped) filter centres, and the
 * cosine basis of the autocorrelation idft [lpc_order + 1][num_banks + 2] (r_i = sum_m idft[i][m] A_m).  Neither depends on
 * fft_size; it is taken for symmetry with mfx_host_mel_table */
int mfx_host_plp_tables(int32_t num_banks, int32_t fft_size, float sample_rate, float low_freq, float high_freq, float alpha,
                        int32_t lpc_order, float *eql, float *idft);
/* TRAPS basis as uploaded (TRAPS): basis [traps_dct_len][traps_len], Hamming window times the DCT-II in the
 * reference's DCT convention, evaluated in double and rounded once.  Lengths as given (no 0 = default here). */
int mfx_host_traps_basis(int32_t traps_len, int32_t traps_dct_len, float *basis);
/* Run lists of mfx_batch_set_alphas as uploaded ("Per-utterance warp factors"): utterance u holds frames[u]
 * consecutive rows.  tables [<= n_utt]: the distinct factors (bit patterns) in order of first appearance; off
 * [tables + 1]; runs [<= n_utt][2] = (first row, rows): table a owns runs off[a] .. off[a + 1] - 1, ascending, equal
 * neighbours merged, frameless utterances left out.  win_rows >= 0: every run clipped to rows [win_row0, win_row0 +
 * win_rows) as the kernels clip it to a slab (empty ones dropped).  Returns the number of tables.  Any output may be NULL.
 * Test / inspection aid. */
int64_t mfx_host_alpha_runs(int32_t n_utt, const float *alphas, const int64_t *frames, int64_t win_row0, int64_t win_rows,
                            float *tables, int32_t *off, int64_t *runs);
/* Speaker lists of mfx_batch_set_speakers as uploaded: speaker s owns list[off[s] .. off[s + 1]), its utterances in ascending
 * utterance index, frameless utterances (frames[u] <= 0) left out.  off [n_spk + 1], list [<= n_utt]; either may be NULL.
 * Returns the list's length, or MFX_ERR_ARG (an id outside [0, n_spk)).  Test / inspection aid. */
int64_t mfx_host_speaker_lists(int32_t n_utt, const int32_t *utt_spk, const int64_t *frames, int32_t n_spk,
                               int32_t *off /* [n_spk+1] */, int32_t *list /* [<= n_utt] */);
/* One transform of mfx_batch_set_transform as k_splice_affine streams it: for every step of 4 taps and every tile of 16
 * outputs the 64 lanes' operands of v_mfma_f32_16x16x4_f32, out[(s * tiles + tile) * 64 + lane] =
 * A[16 tile + (lane & 15)][4 s + (lane >> 4)], zero beyond the matrix; tiles = ceil(out_dim / 16), steps = ceil(in_dim / 4).
 * Returns steps * tiles * 64 (out may be NULL to query).  Test / inspection aid. */
int64_t mfx_host_xform_operands(int32_t out_dim, int32_t in_dim, const float *A, float *out, int64_t out_cap, int32_t *tiles,
                                int32_t *steps);
/* One push of one session of the session entries as the planner derives it: state = {n, E} in / out (both 0 after a final
 * push: the session is fresh); returns the rows delivered.  Also reports the carried PCM samples (per channel) and carried
 * static rows going in, the frames the push computes, and the delta Segment fields seg = {n_out, shift, lo, hi,
 * static_off}, rows relative to the first carried frame max(0, E_old - D).  Any output may be NULL.  Test / inspection aid. */
int32_t mfx_host_session_step(int32_t window, int32_t shift, int32_t D, int64_t state[2], int64_t length, int32_t final_flag,
                              int64_t *carry_samples, int32_t *carry_rows, int32_t *new_frames, int32_t seg[5]);
/* One push of one session under a session rate, exactly as the planner derives it (mfx_sessions_set_rates' delivery rule).  state
 * = {N_in, J} in / out: input samples received, converted samples held (both 0 after a final push); returns J_new - J_old.
 * carry_in / carry_out: the input samples per channel the previous carry slot hands in and the current one keeps, [max(0, (J M)
 * div L - Wh + 1), N) on either side (0 out of a final push, 0 for in_hz == out_hz); either may be NULL.  MFX_ERR_ARG on a pair
 * outside the limits of mfx_batch_plan_rates, a negative length or state, or J beyond ceil(N L / M); nothing is written then.
 * Test / inspection aid. */
int64_t mfx_host_session_resample_step(int32_t in_hz, int32_t out_hz, int32_t zeros, float rolloff, int64_t state[2] /* {N_in, J} */,
                                       int64_t length, int32_t final_flag, int32_t *carry_in, int32_t *carry_out);
/* Sample-rate conversion (mfx_batch_plan_rates).  mfx_host_resample_taps: the table as uploaded, [L][P]; returns L * P or a
 * negative status (MFX_ERR_ARG: outside the limits, or cap too small); taps may be NULL to query.
 * mfx_host_resampled_length: ceil(samples L / M).  mfx_host_resample_layout: the scratch layout (offsets, out_lengths; either
 * may be NULL) of utterances of the given input lengths and rates; returns the total, in output-rate samples per channel.
 * mfx_host_resample_tile: output samples per tile of k_resample for the pair.  UNSTABLE, a test / inspection aid only (utterance
 * lengths at a tile edge): the tiling is the kernel's private matter and may change in any release without an ABI version
 * change; nothing but tests may depend on its value. */
int64_t mfx_host_resample_taps(int32_t in_hz, int32_t out_hz, int32_t zeros, float rolloff, float *taps, int64_t cap, int32_t *L,
                               int32_t *M, int32_t *P);
int64_t mfx_host_resampled_length(int64_t samples, int32_t in_hz, int32_t out_hz);
int64_t mfx_host_resample_layout(int32_t n_utt, const int64_t *lengths, const int32_t *rates_hz, int32_t out_hz, int64_t *offsets,
                                 int64_t *out_lengths);
int32_t mfx_host_resample_tile(int32_t in_hz, int32_t out_hz, int32_t zeros, float rolloff, int32_t channels);
/* The online normaliser (mfx_batch_set_online_norm) on host memory, exactly as defined there: rows [T][pitch], columns
 * [0, Wn) -> out [T][Wn].  kind: MFX_NORM_CMN or MFX_NORM_CVN.  MFX_ERR_ARG on anything outside the limits (nothing is
 * written then).  Test / inspection aid. */
int mfx_host_online_norm(const float *rows, int64_t T, int32_t pitch, int32_t Wn, int32_t kind, int32_t window,
                         int32_t prior_frames, int64_t prior_count, const double *prior_acc, float *out);
/* The sliding-window normaliser (mfx_batch_set_sliding_norm) on host memory, exactly as defined there (no device needed).
 * mfx_host_sliding_window: the window [*ws, *we) of row t of an utterance of T rows.  mfx_host_sliding_norm: rows [T][pitch],
 * columns [0, W) -> out [T][out_pitch], 1 <= W <= 256.  MFX_ERR_ARG on anything outside the limits stated there, t outside
 * [0, T) or a pitch below W (nothing is written then).  Test / inspection aid. */
int mfx_host_sliding_window(int64_t T, int32_t window, int32_t min_window, int32_t center, int64_t t, int64_t *ws, int64_t *we);
int mfx_host_sliding_norm(const float *rows, int64_t T, int32_t W, int32_t pitch, int32_t window, int32_t min_window,
                          int32_t center, int32_t norm_vars, float *out, int32_t out_pitch);
/* The pitch track (mfx_batch_set_pitch) on host memory, exactly as defined there, for ONE utterance: pcm holds its n samples
 * per channel (interleaved for channels = 2), T = its frames (mfx_batch_frames of n on the handle in question) at `shift`;
 * window as resolved (32 .. 1024, never 0).  Writes pitch [T][2], index [T], nccf [T][K]; any of them may be NULL.
 * MFX_ERR_ARG on anything outside the limits (nothing is written then).  Test / inspection aid. */
int mfx_host_pitch(const int16_t *pcm, int64_t n, int32_t channels, int64_t T, int32_t shift, int32_t window, int32_t lag_min,
                   int32_t lag_max, float ballast, float lag_cost, float penalty, int32_t max_jump, float *pitch, int32_t *index,
                   float *nccf);
/* The pitch features (mfx_batch_set_pitch_feats) on host memory, as defined there, for ONE utterance of T rows:
 * pitch [T][2] = (lag, rho) as mfx_batch_pitch_read / mfx_host_pitch deliver them; writes feats [T][F].  MFX_ERR_ARG on
 * anything outside the limits, a sample_rate that is not finite and positive included (nothing is written then).  Test /
 * inspection aid. */
int mfx_host_pitch_feats(const float *pitch /* [T][2]: lag, rho */, int64_t T, float sample_rate, int32_t columns, int32_t left,
                         int32_t right, int32_t delta_window, float pov_scale, float pov_offset, float pitch_scale,
                         float delta_scale, float *feats /* [T][F] */);
/* The tensor output (mfx_batch_set_tensor) on host memory, exactly as defined there, with both conversions in integer
 * arithmetic: rows [.][Wo], utterance u's from row out_rows[u] on, lengths[u] = L_u (cut at Tp) -> out, mfx_host_tensor_bytes
 * of it, every element written.  mfx_host_tensor_bytes: B * Tp * Wo elements of dtype in bytes.  Both: MFX_ERR_ARG on a
 * negative size, Wo < 1 (pack), Tp > 2^24, an unknown layout or dtype, a product beyond int64 (nothing is written then).
 * mfx_host_tensor_lds_bytes: the LDS bytes a block of k_tensor_pack asks for in CHANNEL_MAJOR at this width and the rows t a
 * block owns (*tile_rows); UNSTABLE, a test / inspection aid only, as mfx_host_stft_lds_bytes. */
int mfx_host_tensor_pack(const float *rows, const int64_t *out_rows /* [B] */, const int32_t *lengths /* [B] */, int64_t B,
                         int32_t Wo, int64_t Tp, int32_t layout, int32_t dtype, float pad, void *out);
int64_t mfx_host_tensor_bytes(int64_t B, int32_t Wo, int64_t Tp, int32_t dtype);
int64_t mfx_host_tensor_lds_bytes(int32_t Wo, int32_t *tile_rows);
/* frame count, integer arithmetic (parambase.cpp:16-19 without the float32 division) */
int64_t mfx_host_frame_count(int64_t samples, int32_t window_size, int32_t shift);
/* STFT log-mel (MFX_METHOD_STFT_LOGMEL) tables as uploaded, and its frame rule.  mfx_host_slaney_mel_table: weights
 * [num_banks][dft_size / 2 + 1], beg / len [num_banks] the non-zero span of every row (len 0: none).  mfx_host_stft_basis:
 * cos_sin [2][dft_size / 2 + 1][dft_size], the windowed cosine rows, then the negated windowed sine rows.  MFX_ERR_ARG outside
 * the limits of the method (dft_size even in 32 .. 512, or 1024 / 2048; num_banks 1 .. 128, shift 1 .. dft_size, the frequency
 * rule).  mfx_host_stft_basis describes the matrix form and refuses 1024 / 2048, as mfx_host_stft_lds_bytes,
 * mfx_host_session_stft_step and mfx_host_sess_stft_lds_bytes do. */
int mfx_host_slaney_mel_table(int32_t num_banks, int32_t dft_size, float sample_rate, float low_freq, float high_freq,
                              float *weights, int32_t *beg, int32_t *len);
int mfx_host_stft_basis(int32_t dft_size, const float *window, float *cos_sin);
int64_t mfx_host_stft_frame_count(int64_t samples, int32_t dft_size, int32_t shift);
/* Frames per block (*tile_rows: 64, 32 or 16) that k_stft_mel takes for a shape, and ALL the LDS bytes such a block asks for (the
 * kernel has no static LDS beside them): what mfx_create holds against the 160 KB of a gfx950 block.  MFX_ERR_ARG outside the
 * method's limits, MFX_ERR_CONFIG if no tile fitted.  UNSTABLE, a test / inspection aid only: the tiling is the kernel's private
 * matter. */
int64_t mfx_host_stft_lds_bytes(int32_t dft_size, int32_t shift, int32_t num_banks, int32_t *tile_rows);
/* FFT form (dft_size 1024 or 2048, M = dft_size / 2).  mfx_host_stft_fft_tables: the tables as uploaded, twid [M] complex
 * (re, im): W_M^k = e^(-2 pi i k / M); split [M + 1] complex: -i W_N^k.  mfx_host_stft_fft_lds_bytes: frames per block
 * (*tile_rows: 16, 8 or 4) that k_stft_fft_mel takes for a shape, and ALL the LDS bytes such a block asks for; UNSTABLE, a test /
 * inspection aid only, as mfx_host_stft_lds_bytes.  MFX_ERR_ARG outside the FFT form's limits. */
int mfx_host_stft_fft_tables(int32_t dft_size, float *twid, float *split);
int64_t mfx_host_stft_fft_lds_bytes(int32_t dft_size, int32_t shift, int32_t num_banks, int32_t *tile_rows);
/* One push of one session of an STFT log-mel handle, exactly as the planner derives it (the delivery rule of the method's
 * comment).  state = {n, E} in / out: samples received, rows delivered (both 0 after a final push); returns E_new - E_old.
 * carry_in / carry_out: the samples the previous slot hands in and the current one keeps, [max(0, E S - N / 2), n) on either
 * side (0 out of a final push); either may be NULL.  MFX_ERR_ARG outside the method's limits, on a negative length or state, a
 * length above 2^24, or an E that no open stream of n samples has (beyond mfx_host_stft_frame_count(n), or so far below it
 * that N + S samples or more would be carried); nothing is written then.  Test / inspection aid. */
int32_t mfx_host_session_stft_step(int32_t dft_size, int32_t shift, int64_t state[2], int64_t length, int32_t final_flag,
                                   int32_t *carry_in, int32_t *carry_out);
/* ALL the LDS bytes a block of k_sess_stft_mel asks for with *groups 16-frame groups per block.  *groups = 0 (or groups NULL)
 * on entry: the packing mfx_sessions_create takes -- the largest of 4, 2, 1 that fits the 160 KB of a gfx950 block -- written
 * back; 1, 2 or 4: that packing.  MFX_ERR_ARG outside the method's limits or for another *groups.  UNSTABLE, a test /
 * inspection aid only, as mfx_host_stft_lds_bytes. */
int64_t mfx_host_sess_stft_lds_bytes(int32_t dft_size, int32_t shift, int32_t num_banks, int32_t *groups);
/* Kaldi front end (MFX_METHOD_KALDI) tables as uploaded.  mfx_host_kaldi_mel_table: weights [num_banks][fft_size / 2] (the Nyquist
 * bin has none), beg / len [num_banks] the non-zero span of every band (len 0: none); fft_size 128, 256 or 512, high_freq by the
 * method's rule.  mfx_host_kaldi_dct: matrix [ceps_len][num_banks] = G, row 0 is c0's.  MFX_ERR_ARG outside the method's limits.
 * mfx_host_kaldi_lds_bytes: ALL the LDS bytes a block of k_kaldi_front asks for (the kernel has no static LDS beside them): what
 * mfx_create holds against the 160 KB of a gfx950 block; UNSTABLE, a test / inspection aid only. */
int mfx_host_kaldi_mel_table(int32_t num_banks, int32_t fft_size, float sample_rate, float low_freq, float high_freq,
                             float *weights, int32_t *beg, int32_t *len);
int mfx_host_kaldi_dct(int32_t num_banks, int32_t ceps_len, float lifter, float *matrix);
int64_t mfx_host_kaldi_lds_bytes(int32_t window_size, int32_t shift, int32_t num_banks, int32_t ceps_len);
/* The same under kaldi_flags (fbank with the energy column assembles rows of num_banks + 1 floats): what mfx_create
 * holds against the cap on a handle with flags; at flags 0 it is mfx_host_kaldi_lds_bytes.  MFX_ERR_ARG for flags the method
 * refuses.  UNSTABLE likewise. */
int64_t mfx_host_kaldi_lds_bytes_flags(int32_t window_size, int32_t shift, int32_t num_banks, int32_t ceps_len, int32_t flags);
/* Host restatements of the Kaldi frame rule (no device needed).  mfx_host_kaldi_frame_count: T of an utterance of `samples`
 * samples under `flags` (only MFX_KALDI_NO_SNIP_EDGES matters); MFX_ERR_ARG for samples < 0 or a window / shift outside the
 * method's limits.  mfx_host_kaldi_frame_samples: idx [window_size] = the utterance sample index of every tap of frame t, by
 * the closed form the kernel uses (every index lies in [0, samples)); MFX_ERR_ARG also for t outside [0, T). */
int64_t mfx_host_kaldi_frame_count(int64_t samples, int32_t window_size, int32_t shift, int32_t flags);
int mfx_host_kaldi_frame_samples(int64_t samples, int32_t window_size, int32_t shift, int32_t flags, int64_t t, int64_t *idx);

/* ---- test taps (device -> host copies of intermediate tables; used by the parity tests) ---- */
/* kind: 0 = mel table [2][fft_size] floats, 1 = filter_beg [num_banks+2] int32,
 *       2 = DCT matrix [num_banks][dct_len] floats, 3 = magnitude spectrum of the current block
 *       [frames_with_context][fft_size/2+1] floats, 5 / 6 = normaliser statistics of the last streaming apply / batch run,
 *       7 = PLP autocorrelations r_0 .. r_p of the last plain streaming apply [frames_with_context][lpc_order + 1] floats
 *       (MFCC handles: 0 elements), 8 = converted PCM of the last batch run under a rates plan, int16 in the scratch layout
 *       of mfx_batch_resample_layout (0 elements without one).  Returns element count or <0. */
int64_t mfx_debug_read(mfx_handle *h, int kind, void *dst, int64_t dst_bytes);

#ifdef __cplusplus
}
#endif
#endif /* MFX_H */
