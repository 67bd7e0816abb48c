// afet_hip.cpp -- command-line driver over MfccHip: the reference's per-file loop
// (process_files_worker, ASR_OCL.cpp:109-338) with its own minimal RIFF/PCM16 reader in place of
// libsndfile and the option names of the reference's (commented-out) option table
// (ASR_OCL.cpp:569-669).  Output is the reference's text format (ASR_OCL.cpp:252-260):
//     | <frame time> | v0 | v1 | ... |
//
//   afet_hip [options] in1.wav out1.txt [in2.wav out2.txt ...]
// Inputs: RIFF/WAVE or NIST SPHERE (the reference's sample1.wav), 16-bit PCM.  --htk writes HTK
// parameter files instead of text (the reference's binary branch is a stub).
//
// Files that the reference's loop would consume as ONE block (no longer than --sample-limit; one alpha) are not pushed
// through set_input / apply / get_output_data one by one: a worker drains the queue into batches of up to --batch-mb of
// PCM, packs them into one pinned buffer and runs ONE mfx_batch_plan + mfx_batch_run_host per batch (a 7 s file is ~1 us
// of kernel work against ~130 us of per-call overhead), while helper threads read the next batch's files and format /
// write the previous batch's rows.  The extractor is created with MFX_ENGINE_STREAM_KERNELS, so the rows are the same
// bits the per-file loop delivers, and the reference's single-block flush behaviour (B1, --bug-compat) is applied to them:
// the outputs are byte-identical to the per-file loop's (--batch-mb 0 selects that loop; tests compare the two).
// --resample-to HZ extracts at HZ instead of the first file's rate: window and shift in samples follow HZ, and a file at
// another rate is converted on the device -- inside its batch through mfx_batch_plan_rates, or as a batch of one where the
// per-file loop would otherwise run (--batch-mb 0).  The reference has no rows for such a file (it refuses it), so its
// single-block flush behaviour (B1) is not applied to converted files.  Without the option nothing changes.
// --alpha-file gives every input file its own warp factor: the files of a batch then run with mfx_batch_set_alphas (one
// launch sequence for all factors), files on the per-file loop with set_alpha of their own factor.
// --spk-file gives every input file a speaker label: the normaliser's statistics are pooled over each speaker's files
// (mfx_batch_set_speakers) in two passes over the list -- pass 1 runs the batches and carries their accumulators from batch
// to batch, pass 2 runs them again with the final accumulators and writes the files.  Batches only, one device.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <atomic>
#include <charconv>
#include <future>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "afet_param.h"
#include "../../include/mfx.h"

namespace {

struct Options {
    float window_ms = 25.f, shift_ms = 10.f;
    int banks = 15, ceps = 12, norm = 2, dyn = 0, l1 = 3, l2 = 3;   // reference main() defaults (ASR_OCL.cpp:560)
    float low = 64.f, high = 0.f, lift = 22.f;
    bool low_given = false;                        // (--method LOGMEL starts at 0 Hz unless --low-freq says otherwise)
    bool c0 = true, norm_after_dyn = true;
    float alpha_min = 1.f, alpha_max = 1.f, alpha_step = 1.f;
    std::string alpha_file;        // --alpha-file: one warp factor per line, in the order of the input list
    std::vector<float> file_alpha; // its factors: file i of the list is extracted with file_alpha[i]
    int online_window = -1;        // --online-window: online (causal) CMN / CVN of the batches, window in frames (0: cumulative)
    int online_prior_frames = 0;   // --online-prior-frames
    int cmn_window = 0;            // --cmn-window: sliding-window CMN / CVN of the batches (apply-cmvn-sliding), window in frames (0: off)
    int cmn_center = 0;            // --cmn-center 0|1
    int cmn_min_window = -1;       // --cmn-min-window (-1: apply-cmvn-sliding's 100, or the window if that is shorter)
    bool cmn_norm_vars = false;    // --cmn-norm-vars
    bool cmn_options = false;      // one of the three was given
    std::string spk_file;          // --spk-file: one speaker label per line, in the order of the input list
    std::vector<int> file_spk;     // its labels as ids, numbered by first appearance: file i belongs to speaker file_spk[i]
    int n_spk = 0;
    int sample_limit = 10000000, device = 0;
    bool bug_compat = true;
    int method = MFX_METHOD_MFCC, model_order = 8; // --method MFCC|PLP|TRAPS, --model-order (ASR_OCL.cpp:54-56: default 8)
    int traps_len = 31, traps_dct = 10;            // --traps-length, --traps-dct (ASR_OCL.cpp:604-606: defaults 31 and 10)
    int logmel_post = MFX_LOGMEL_WHISPER;          // --logmel-post whisper|log10|ln (--method LOGMEL)
    int logmel_nfft = 0;                           // --logmel-nfft 1024|2048 (--method LOGMEL): the DFT length; the Hann window of
                                                   // the --window-size length is centred in it.  0: the window's own length
    // --method KALDI: the three frame options (Kaldi's defaults); the window is the Povey window, --ceps 0 is fbank
    float kaldi_preemph = 0.97f;   // --preemph X
    bool kaldi_dc = true;          // --no-dc-removal
    bool kaldi_power = true;       // --magnitude
    int kaldi_flags = 0;           // --snip-edges 0, --use-energy, --raw-energy 0, --htk-compat: MFX_KALDI_* (creation-time)
    bool kaldi_raw_energy = true;  // --raw-energy 0|1 (needs --use-energy when 0)
    float kaldi_energy_floor = 0.f; // --energy-floor X
    bool htk = false; // binary output in HTK parameter-file format instead of the reference's text rows
    int format_threads = 4; // threads that format the text rows of a block (per worker)
    int batch_mb = 16;      // PCM per batch of files (0: the per-file loop only); small enough that a few thousand files pipeline
    int io_threads = 12;    // helper threads of a worker that read files and format / write rows of a batch
    std::vector<int> devices; // --devs a,b,...: one worker (own MfccHip, own thread) per entry
    int resample_to = 0;    // --resample-to HZ: extract at HZ whatever the first file's rate; files at other rates are converted
                            // on the device (mfx_batch_plan_rates).  0: the reference's rule -- every file at the first file's rate
    int resample_zeros = 0; // --resample-zeros N: zero crossings of the conversion filter per side (0 = the library's 6)
    // --vad: energy VAD + select-voiced-frames on the device (mfx_batch_set_vad, SELECT): every output file holds its voiced
    // rows only.  The defaults are compute-vad-energy's; the column is the last static one (c0 with --c0 1)
    bool vad = false;
    float vad_energy_threshold = 5.f, vad_energy_mean_scale = 0.5f, vad_proportion_threshold = 0.6f;
    int vad_frames_context = 0, vad_column = -1;
    // --pitch: pitch track + Kaldi's three default pitch features (mfx_batch_set_pitch, mfx_batch_set_pitch_feats) pasted
    // behind every row; --pitch-range LO:HI in Hz bounds the lags searched
    bool pitch = false;
    float pitch_lo = 50.f, pitch_hi = 400.f;
};

struct Wav {
    int sample_rate = 0, channels = 0;
    std::vector<int16_t> pcm; // interleaved
};

uint32_t rd32(const unsigned char *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
uint16_t rd16(const unsigned char *p) { return (uint16_t)(p[0] | (p[1] << 8)); }

// NIST SPHERE (the reference ships one: sample1.wav): "NIST_1A\n   <header bytes>\n" followed by
// "key -type value" lines up to "end_head"; 16-bit PCM, sample_byte_format 01 = little endian, 10 = big.
Wav read_sphere(const std::vector<unsigned char> &b, const std::string &path)
{
    // "NIST_1A\n" then the header length as text on a line of its own: parse a bounded, terminated copy
    const std::string len_field(reinterpret_cast<const char *>(b.data()) + 8, std::min<size_t>(b.size() - 8, 8));
    const size_t hdr = (size_t)std::max(0L, std::atol(len_field.c_str()));
    if (hdr < 16 || hdr > b.size()) throw std::runtime_error("bad SPHERE header in \"" + path + "\"");
    const std::string text(reinterpret_cast<const char *>(b.data()), hdr);
    auto field = [&](const char *key, const std::string &dflt) -> std::string {
        size_t p = text.find(std::string("\n") + key + " ");
        if (p == std::string::npos) return dflt;
        p = text.find(' ', p + 1 + std::strlen(key) + 1); // skip "-i" / "-sN"
        if (p == std::string::npos) return dflt;
        const size_t e = text.find('\n', p);
        return text.substr(p + 1, e - p - 1);
    };
    Wav w;
    w.channels = std::atoi(field("channel_count", "1").c_str());
    w.sample_rate = std::atoi(field("sample_rate", "0").c_str());
    const long count = std::atol(field("sample_count", "0").c_str());
    if (std::atoi(field("sample_n_bytes", "2").c_str()) != 2 || field("sample_coding", "pcm").find("pcm") != 0)
        throw std::runtime_error("only 16-bit PCM SPHERE files are supported");
    const bool big = field("sample_byte_format", "01") == "10";
    size_t n = std::min<size_t>((b.size() - hdr) / 2, (size_t)std::max<long>(count, 0) * std::max(w.channels, 1));
    w.pcm.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const unsigned char *q = &b[hdr + 2 * i];
        w.pcm[i] = (int16_t)(big ? ((q[0] << 8) | q[1]) : (q[0] | (q[1] << 8)));
    }
    if (w.channels < 1 || w.sample_rate <= 0 || w.pcm.empty()) throw std::runtime_error("Error while loading \"" + path + "\"");
    return w;
}

Wav read_wav(const std::string &path)
{
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("Can't open \"" + path + "\"");
    std::vector<unsigned char> b;
    std::fseek(f, 0, SEEK_END);
    const long fsz = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (fsz > 0) { // one read of the whole file
        b.resize((size_t)fsz);
        b.resize(std::fread(b.data(), 1, (size_t)fsz, f));
    } else { // (not seekable)
        unsigned char buf[65536];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
    }
    std::fclose(f);
    if (b.size() >= 16 && std::memcmp(b.data(), "NIST_1A", 7) == 0) return read_sphere(b, path);
    if (b.size() < 12 || std::memcmp(b.data(), "RIFF", 4) != 0 || std::memcmp(b.data() + 8, "WAVE", 4) != 0)
        throw std::runtime_error("\"" + path + "\" is not a RIFF/WAVE or NIST SPHERE file");
    Wav w;
    size_t pos = 12;
    bool have_fmt = false;
    while (pos + 8 <= b.size()) {
        const uint32_t sz = rd32(&b[pos + 4]);
        const unsigned char *body = b.data() + pos + 8;
        if (std::memcmp(&b[pos], "fmt ", 4) == 0 && sz >= 16) {
            if (pos + 8 + 16 > b.size()) throw std::runtime_error("truncated fmt chunk in \"" + path + "\"");
            if (rd16(body) != 1 || rd16(body + 14) != 16) throw std::runtime_error("only 16-bit PCM is supported");
            w.channels = rd16(body + 2);
            w.sample_rate = (int)rd32(body + 4);
            have_fmt = true;
        } else if (std::memcmp(&b[pos], "data", 4) == 0) {
            const size_t avail = std::min<size_t>(sz, b.size() - pos - 8);
            w.pcm.resize(avail / 2);
            if (!w.pcm.empty()) std::memcpy(w.pcm.data(), body, w.pcm.size() * 2);
        }
        pos += (size_t)8 + sz + (sz & 1);
    }
    // (a fmt chunk that announces 0 channels or a rate of 0 is refused like an unreadable file: the downmix divides by the
    // channel count -- found reading the parser beside tools/fuzz_all.py's finds, round 4)
    if (!have_fmt || w.channels < 1 || w.sample_rate <= 0 || w.pcm.empty()) throw std::runtime_error("Error while loading \"" + path + "\"");
    return w;
}

// HTK parameter file: big-endian header {int32 nSamples, int32 sampPeriod [100 ns], int16 sampSize, int16 parmKind}
// then nSamples vectors of big-endian float32 (the reference's own binary branch is an empty stub,
// ASR_OCL.cpp:212,315-319).
void put_be32(FILE *f, uint32_t v)
{
    unsigned char b[4] = {(unsigned char)(v >> 24), (unsigned char)(v >> 16), (unsigned char)(v >> 8), (unsigned char)v};
    std::fwrite(b, 1, 4, f);
}
void put_be16(FILE *f, uint16_t v)
{
    unsigned char b[2] = {(unsigned char)(v >> 8), (unsigned char)v};
    std::fwrite(b, 1, 2, f);
}
void write_htk_header(FILE *f, uint32_t n_frames, const Options &o, int width)
{
    const bool traps = o.method == MFX_METHOD_TRAPS;
    uint16_t kind = traps ? 9 /* USER */ : o.method == MFX_METHOD_PLP ? 11 /* PLP */ : o.ceps > 0 ? 6 /* MFCC */ : 7 /* FBANK */;
    if (!traps && o.ceps > 0 && o.c0) kind |= 0x2000;  // _0 (a Kaldi handle's c0 is column 0, not the last: no qualifier)
    if (o.dyn >= 1) kind |= 0x0100;          // _D
    if (o.dyn >= 2) kind |= 0x0200;          // _A
    if (o.norm == 1) kind |= 0x0800;         // _Z (zero mean)
    put_be32(f, n_frames);
    put_be32(f, (uint32_t)std::llround(o.shift_ms * 1e4));
    put_be16(f, (uint16_t)(4 * width));
    put_be16(f, kind);
}
void write_rows_htk(FILE *out, const float *rows, int n, int width, std::vector<char> &buf)
{
    const size_t count = (size_t)n * width;
    buf.resize(count * 4);
    for (size_t i = 0; i < count; ++i) { // big endian, one write for the block
        uint32_t u;
        std::memcpy(&u, &rows[i], 4);
        buf[4 * i] = (char)(u >> 24);
        buf[4 * i + 1] = (char)(u >> 16);
        buf[4 * i + 2] = (char)(u >> 8);
        buf[4 * i + 3] = (char)u;
    }
    std::fwrite(buf.data(), 1, buf.size(), out);
}

// "%f" of a double into p (std::to_chars with fixed notation and precision 6 is specified to produce what printf("%f")
// prints in the C locale, i.e. the reference's text, ASR_OCL.cpp:254-257 -- only without a format parse per value)
inline char *put_f(char *p, char *end, double v)
{
    if (!(v == v) || v - v != 0.0) return p + std::snprintf(p, (size_t)(end - p), "%f", v); // nan / inf as printf spells them
    return std::to_chars(p, end, v, std::chars_format::fixed, 6).ptr;
}

// "%f" of a FLOAT, exactly as printf prints it, without going through a general double formatter: the value is
// m * 2^e with a 24-bit m, so round(value * 10^6) is one 64-bit product, one shift and a round-half-to-even on the exact
// remainder (ties do occur: 1/128 = 0.0078125).  Values of 2^40 and more, NaN and infinities take the general path.
inline char *put_f32(char *p, char *end, float vf)
{
    uint32_t u;
    std::memcpy(&u, &vf, 4);
    const uint32_t ex = (u >> 23) & 0xffu;
    if (ex >= 127 + 40) return put_f(p, end, (double)vf);
    uint64_t m = u & 0x7fffffu;
    int e;
    if (ex == 0) {
        e = -149; // denormal (or zero)
    } else {
        m |= 0x800000u;
        e = (int)ex - 150;
    }
    uint64_t q;
    const uint64_t P = m * 1000000ull; // < 2^44
    if (e >= 0) {
        q = P << e; // e <= 16 here: < 2^60
    } else {
        const int sh = -e;
        if (sh >= 64) {
            q = 0;
        } else {
            q = P >> sh;
            const uint64_t rem = P & ((1ull << sh) - 1), half = 1ull << (sh - 1);
            if (rem > half || (rem == half && (q & 1))) ++q;
        }
    }
    if (u >> 31) *p++ = '-';
    const uint64_t ip = q / 1000000ull;
    uint32_t fp = (uint32_t)(q % 1000000ull);
    p = std::to_chars(p, end, ip).ptr;
    *p++ = '.';
    for (int i = 5; i >= 0; --i) {
        p[i] = (char)('0' + fp % 10);
        fp /= 10;
    }
    return p + 6;
}

// rows [r0, r1) formatted into p; returns the end
char *format_rows(char *p, char *end, const float *rows, int r0, int r1, int width, int first_frame, long double t0, long double dt)
{
    for (int f = r0; f < r1; ++f) {
        *p++ = '|';
        *p++ = ' ';
        p = put_f(p, end, (double)(t0 + (first_frame + f) * dt));
        *p++ = ' ';
        *p++ = '|';
        for (int i = 0; i < width; ++i) {
            *p++ = ' ';
            p = put_f32(p, end, rows[(size_t)width * f + i]);
            *p++ = ' ';
            *p++ = '|';
        }
        *p++ = '\n';
    }
    return p;
}

void write_rows(FILE *out, const float *rows, int n, int width, int first_frame, long double t0, long double dt,
                std::vector<char> &buf, int threads)
{
    // a value needs at most 1 + 39 + 1 + 6 characters plus " |"; the rows are formatted into one buffer (large blocks: by a
    // few threads, each into its own share of the buffer) and written in order
    const size_t per_row = ((size_t)width + 1) * 52 + 4;
    buf.resize((size_t)n * per_row + 16);
    const int T = (n >= 256 && threads > 1) ? std::min(threads, 4) : 1;
    if (T == 1) {
        char *p = format_rows(buf.data(), buf.data() + buf.size(), rows, 0, n, width, first_frame, t0, dt);
        std::fwrite(buf.data(), 1, (size_t)(p - buf.data()), out);
        return;
    }
    std::vector<std::thread> th;
    std::vector<size_t> used((size_t)T, 0);
    for (int t = 0; t < T; ++t) {
        const int r0 = (int)((int64_t)n * t / T), r1 = (int)((int64_t)n * (t + 1) / T);
        char *base = buf.data() + (size_t)r0 * per_row;
        th.emplace_back([=, &used] { used[t] = (size_t)(format_rows(base, base + (size_t)(r1 - r0) * per_row, rows, r0, r1, width, first_frame, t0, dt) - base); });
    }
    for (auto &x : th) x.join();
    for (int t = 0; t < T; ++t) std::fwrite(buf.data() + (size_t)((int64_t)n * t / T) * per_row, 1, used[t], out);
}

// --spk-file: speaker labels (one per line; blank lines skipped, surrounding white space dropped) -> ids by first appearance
int map_speaker_labels(const std::vector<std::string> &labels, std::vector<int> &ids)
{
    std::vector<std::string> seen;
    ids.clear();
    for (const std::string &l : labels) {
        size_t k = 0;
        while (k < seen.size() && seen[k] != l) ++k;
        if (k == seen.size()) seen.push_back(l);
        ids.push_back((int)k);
    }
    return (int)seen.size();
}

bool read_label_lines(FILE *f, std::vector<std::string> &labels)
{
    char line[1024];
    while (std::fgets(line, sizeof(line), f)) {
        std::string l(line);
        const size_t a = l.find_first_not_of(" \t\r\n");
        if (a == std::string::npos) continue; // (blank line)
        const size_t b = l.find_last_not_of(" \t\r\n");
        labels.push_back(l.substr(a, b - a + 1));
    }
    return true;
}

// --timing: wall time per phase, summed over the files of all workers (dev aid; printed at exit)
struct Timing {
    std::atomic<long long> wait_read{0}, prep{0}, device{0}, write{0}, files{0};
    std::atomic<long long> prep_wall{0}, write_wall{0}, wait_write{0}, batches{0}; // batched mode: wall time of the stages
    std::atomic<long long> t_main{0}, t_created{0}, t_loop_end{0}, t_destroyed{0};  // process milestones (last worker to pass)
    bool on = false;
} g_time;
inline long long now_ns()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (long long)ts.tv_sec * 1000000000ll + ts.tv_nsec;
}

// buffers a worker keeps from file to file (the row buffer alone is ~10 MB at the reference's default sample limit)
struct Scratch {
    std::vector<float> rows;
    std::vector<int16_t> mono;
    std::vector<char> text;
};

// --resample-to, a file at another rate where the per-file loop runs: a batch of one through mfx_batch_plan_rates (the
// streaming interface takes samples at the extractor's rate only).  One warp factor: the file's own or --alpha.
void process_file_resampled(MfccHip &param, const Options &o, const Wav &w, const std::string &in, const std::string &out_name,
                            float sample_rate, Scratch &sc, const float *own_alpha)
{
    if (!own_alpha && o.alpha_max - o.alpha_min >= o.alpha_step)
        throw std::runtime_error("File \"" + in + "\" needs sample-rate conversion, which takes one warp factor, not a sweep");
    std::vector<int16_t> &mono = sc.mono;
    mono.assign(w.pcm.size() / w.channels + 2, 0); // (+ 2: the word that holds the last sample is inside the buffer)
    const long long n = (long long)(w.pcm.size() / w.channels);
    for (long long i = 0; i < n; ++i)
        mono[i] = w.channels >= 2 ? (int16_t)(((int)w.pcm[i * w.channels] + (int)w.pcm[i * w.channels + 1]) >> 1)
                                  : w.pcm[i * w.channels];
    const int width = param.get_output_data_width();
    const long long off = 0;
    long long row0 = 0;
    const long long total = param.batch_plan_rates(1, &off, &n, &w.sample_rate, o.resample_zeros, &row0);
    param.set_warp(own_alpha ? *own_alpha : o.alpha_min); // (same-rate files of the loop set their own factor before apply)
    std::vector<float> &rows = sc.rows;
    if (rows.size() < (size_t)std::max<long long>(total, 1) * width) rows.resize((size_t)std::max<long long>(total, 1) * width);
    param.batch_run_host(mono.data(), n + 1, rows.data());
    const long double dt = o.bug_compat ? (long double)(o.shift_ms / sample_rate) : o.shift_ms / 1000.0L;
    const long double t0 = o.bug_compat ? (long double)(0.5f * o.window_ms / sample_rate) : 0.5L * o.window_ms / 1000.0L;
    FILE *fo = std::fopen(out_name.c_str(), o.htk ? "wb" : "w");
    if (!fo) throw std::runtime_error("Can't create output file: " + out_name);
    if (o.htk) {
        write_htk_header(fo, (uint32_t)total, o, width);
        write_rows_htk(fo, rows.data(), (int)total, width, sc.text);
    } else {
        write_rows(fo, rows.data(), (int)total, width, 0, t0, dt, sc.text, o.format_threads);
    }
    std::fclose(fo);
    if (g_time.on) ++g_time.files;
    static std::mutex print_lock;
    std::lock_guard<std::mutex> g(print_lock);
    std::printf("%s: %lld frames x %d\n", in.c_str(), total, width);
}

// own_alpha: the file's factor of --alpha-file (one output, no name suffix) instead of the --alpha options' loop
void process_file(MfccHip &param, const Options &o, const Wav &w, const std::string &in, const std::string &out_name,
                  float sample_rate, Scratch &sc, const float *own_alpha = nullptr)
{
    if ((float)w.sample_rate != sample_rate) {
        if (o.resample_to <= 0) throw std::runtime_error("File \"" + in + "\" has incorrect sample rate");
        process_file_resampled(param, o, w, in, out_name, sample_rate, sc, own_alpha);
        return;
    }
    // Multi-channel input: ONE policy across the product -- the downmix of the batch kernels (channels = 2 in the C
    // ABI: mono = (L + R) >> 1 in integer arithmetic), applied here on the host because the streaming
    // interface is mono like the reference's (which has no downmix at all: it reads `frames` shorts into a mono-sized
    // buffer, ASR_OCL.cpp:229-231).  More than two channels: the first two.
    const long long t_begin = g_time.on ? now_ns() : 0;
    long long t_dev = 0, t_wr = 0;
    std::vector<int16_t> &mono = sc.mono;
    mono.resize(w.pcm.size() / w.channels);
    for (size_t i = 0; i < mono.size(); ++i)
        mono[i] = w.channels >= 2 ? (int16_t)(((int)w.pcm[i * w.channels] + (int)w.pcm[i * w.channels + 1]) >> 1)
                                  : w.pcm[i * w.channels];

    const int limit = param.get_input_buffer_size();
    const int width = param.get_output_data_width();
    const int rows_cap = std::max(param.estimated_window_count(limit), 0) + 64;
    std::vector<float> &rows = sc.rows;
    if (rows.size() < (size_t)rows_cap * width) rows.resize((size_t)rows_cap * width);
    // Frame time column.  The reference divides its window / shift IN MILLISECONDS by the sample rate
    // (ASR_OCL.cpp:225-226: cfg.shift / cfg.sample_rate, 0.5f * cfg.window_size / cfg.sample_rate, float arithmetic):
    // 0.000625 s per frame at 10 ms / 16 kHz instead of 0.01 s.  --bug-compat 1 (default) prints
    // what the reference prints, --bug-compat 0 the times in seconds.
    const long double dt = o.bug_compat ? (long double)(o.shift_ms / sample_rate) : o.shift_ms / 1000.0L;
    const long double t0 = o.bug_compat ? (long double)(0.5f * o.window_ms / sample_rate) : 0.5L * o.window_ms / 1000.0L;

    std::vector<std::pair<float, FILE *>> outs;
    int idx = 0;
    const float a_min = own_alpha ? *own_alpha : o.alpha_min, a_max = own_alpha ? *own_alpha : o.alpha_max;
    for (float a = a_min; a <= a_max; a = a_min + (++idx) * o.alpha_step) {
        std::string name = out_name;
        if (a_max - a_min >= o.alpha_step) name += "." + std::to_string(a);
        FILE *fo = std::fopen(name.c_str(), o.htk ? "wb" : "w");
        if (!fo) throw std::runtime_error("Can't create output file: " + name);
        if (o.htk) write_htk_header(fo, 0, o, width); // frame count patched at the end
        outs.emplace_back(a, fo);
    }
    size_t pos = 0;
    int total = 0;
    std::vector<float> alphas;
    for (auto &oa : outs) alphas.push_back(oa.first);
    // One alpha: the reference's set_alpha + apply + get_output_data (ASR_OCL.cpp:236-243).  Several:
    // the whole sweep over the block's stored spectrum in one call (mfx_apply_alphas).
    auto emit = [&](int n) {
        if (n <= 0) return;
        long long t0e = g_time.on ? now_ns() : 0;
        if (alphas.size() > 1) param.apply_alphas(alphas.data(), (int)alphas.size());
        for (size_t i = 0; i < outs.size(); ++i) {
            if (alphas.size() > 1) {
                param.get_output_data_alpha((int)i, rows.data(), n);
            } else {
                param.set_alpha(alphas[i]);
                param.apply();
                param.get_output_data(rows.data(), n);
            }
            const long long t1e = g_time.on ? now_ns() : 0;
            t_dev += t1e - t0e;
            if (o.htk)
                write_rows_htk(outs[i].second, rows.data(), n, width, sc.text);
            else
                write_rows(outs[i].second, rows.data(), n, width, total, t0, dt, sc.text, o.format_threads);
            t0e = g_time.on ? now_ns() : 0;
            t_wr += t0e - t1e;
        }
    };
    while (pos < mono.size()) {
        const int n_in = (int)std::min<size_t>(mono.size() - pos, (size_t)limit);
        const long long ts0 = g_time.on ? now_ns() : 0;
        const int n = param.set_input(mono.data() + pos, n_in);
        if (g_time.on) t_dev += now_ns() - ts0;
        emit(n);
        total += n;
        pos += n_in;
    }
    const long long tf0 = g_time.on ? now_ns() : 0;
    const int n = param.flush();
    if (g_time.on) t_dev += now_ns() - tf0;
    if (n > 0) emit(n);
    total += n;
    for (auto &oa : outs) {
        if (o.htk) {
            std::fseek(oa.second, 0, SEEK_SET);
            write_htk_header(oa.second, (uint32_t)total, o, width);
        }
        std::fclose(oa.second);
    }
    if (g_time.on) {
        const long long t_end = now_ns();
        g_time.device += t_dev;
        g_time.write += t_wr;
        g_time.prep += (t_end - t_begin) - t_dev - t_wr; // downmix, opening and closing the outputs
        ++g_time.files;
    }
    static std::mutex print_lock;
    std::lock_guard<std::mutex> g(print_lock);
    std::printf("%s: %d frames x %d\n", in.c_str(), total, width);
}

// ---- batches of whole files -----------------------------------------------------------------------------------------
struct Pinned { // page-locked buffer (DMA straight from / to it), grown on demand
    void *p = nullptr;
    size_t bytes = 0;
    void *get(size_t need)
    {
        if (need > bytes) {
            mfx_free_pinned(p);
            bytes = need + need / 4;
            p = mfx_alloc_pinned(bytes);
            if (!p) throw std::runtime_error("can't allocate pinned host memory");
        }
        return p;
    }
    ~Pinned() { mfx_free_pinned(p); }
};

template <class F>
void parallel_for(size_t n, int threads, F fn)
{
    std::atomic<size_t> next{0};
    auto body = [&](int t) { // t = helper index: callers keep per-helper scratch
        for (size_t i; (i = next.fetch_add(1)) < n;) fn(i, t);
    };
    const int T = (int)std::min<size_t>((size_t)std::max(threads, 1), n);
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(body, t);
    body(0);
    for (auto &x : th) x.join();
}

struct BatchItem {
    size_t file = 0;            // index of the (input, output) pair
    std::vector<int16_t> mono;  // downmixed samples
    std::string error;          // reading / checking failed
    bool stream = false;        // not batchable: goes through the per-file loop
    Wav wav;                    // kept for the per-file loop
    long long off = 0, len = 0, row0 = 0, frames = 0;
    long long out_frames = 0;   // rows written to the file: frames, or the voiced ones with --vad
    int rate = 0;               // the file's own sample rate (--resample-to: may differ from the extractor's)
    long long conv_len = 0;     // samples after conversion (= len at the extractor's rate)
};

struct Batch {
    std::vector<BatchItem> items;
    Pinned pcm, rows;
    long long samples = 0, total_rows = 0;
    int width = 0;
};

// Claims files from the shared queue until the batch holds `cap_samples`, reads and downmixes them (io threads) and
// packs the batchable ones back to back (even offsets: aligned 32-bit loads) into the pinned PCM buffer.
bool prepare_batch(Batch &b, const Options &o, const std::vector<std::string> &files, std::atomic<size_t> &next, float sr,
                   long long cap_samples, int limit, int W, int S, int D)
{
    struct WallTimer {
        long long t0 = g_time.on ? now_ns() : 0;
        ~WallTimer()
        {
            if (g_time.on) g_time.prep_wall += now_ns() - t0;
        }
    } wall_timer;
    b.items.clear();
    b.samples = 0;
    // file sizes bound the sample counts before anything is read: claim while the batch has room
    long long claimed = 0;
    while (claimed < cap_samples && b.items.size() < 4096) {
        const size_t i = next.fetch_add(1);
        if (2 * i + 1 >= files.size()) break;
        BatchItem it;
        it.file = i;
        b.items.push_back(std::move(it));
        FILE *f = std::fopen(files[2 * i].c_str(), "rb");
        long sz = 0;
        if (f) {
            std::fseek(f, 0, SEEK_END);
            sz = std::ftell(f);
            std::fclose(f);
        }
        claimed += std::max(sz, 0L) / 2;
    }
    if (b.items.empty()) return false;
    const bool sweep = o.alpha_max - o.alpha_min >= o.alpha_step;
    parallel_for(b.items.size(), o.io_threads, [&](size_t k, int) {
        BatchItem &it = b.items[k];
        try {
            it.wav = read_wav(files[2 * it.file]);
            const bool other_rate = (float)it.wav.sample_rate != sr;
            if (other_rate && o.resample_to <= 0)
                throw std::runtime_error("File \"" + files[2 * it.file] + "\" has incorrect sample rate");
            const size_t n = it.wav.pcm.size() / it.wav.channels;
            it.rate = it.wav.sample_rate;
            // (--resample-to: frames, block limit and context are counted in samples AFTER conversion)
            const long long nc = other_rate ? (long long)mfx_host_resampled_length((int64_t)n, it.rate, o.resample_to) : (long long)n;
            if (nc < 0) throw std::runtime_error("File \"" + files[2 * it.file] + "\": sample rate outside 1000 .. 768000 Hz");
            it.conv_len = nc;
            const bool logmel = o.method == MFX_METHOD_STFT_LOGMEL; // (centred frames: its own frame rule)
            const long long T = logmel ? std::max<long long>(0, (long long)mfx_host_stft_frame_count(nc, W, S)) : nc >= W ? (nc - (W - S)) / S : 0;
            // the per-file loop keeps: files of more than one block, files too short for the deltas' context (the
            // reference refuses or mangles them: same messages from the same code), alpha sweeps
            // (TRAPS has no per-file loop: every file is one utterance of a batch, whatever its length)
            // (a file at another rate has no per-file loop either: it stays in the batch, and a sweep over it is refused)
            if (other_rate && sweep)
                throw std::runtime_error("File \"" + files[2 * it.file] + "\" needs sample-rate conversion, which takes one warp factor, not a sweep");
            it.stream = o.method != MFX_METHOD_TRAPS && o.method != MFX_METHOD_KALDI && !logmel && !other_rate && (sweep || n > (size_t)limit || T < 2 * D + 1);
            if (!it.stream) {
                it.mono.resize(n);
                const int ch = it.wav.channels;
                for (size_t s2 = 0; s2 < n; ++s2)
                    it.mono[s2] = ch >= 2 ? (int16_t)(((int)it.wav.pcm[s2 * ch] + (int)it.wav.pcm[s2 * ch + 1]) >> 1) : it.wav.pcm[s2 * ch];
                it.wav.pcm.clear();
                it.wav.pcm.shrink_to_fit();
                it.len = (long long)n;
                it.frames = T;
            }
        } catch (const std::exception &e) {
            it.error = e.what();
        }
    });
    long long pos = 0;
    for (BatchItem &it : b.items)
        if (it.error.empty() && !it.stream) {
            it.off = pos;
            pos += it.len + (it.len & 1);
        }
    b.samples = pos;
    if (pos > 0) {
        int16_t *dst = (int16_t *)b.pcm.get((size_t)(pos + 8) * sizeof(int16_t));
        parallel_for(b.items.size(), o.io_threads, [&](size_t k, int) {
            BatchItem &it = b.items[k];
            if (!it.error.empty() || it.stream) return;
            std::memcpy(dst + it.off, it.mono.data(), (size_t)it.len * sizeof(int16_t));
            if (it.len & 1) dst[it.off + it.len] = 0;
            std::vector<int16_t>().swap(it.mono);
        });
    }
    return true;
}

// One worker of the reference's file queue (process_files_worker over the shared std::list,
// ASR_OCL.cpp:109-338,340-368): its own extractor on its own device, files drawn from a shared index
// until the queue is empty.  The reference runs its workers one after another (:365-366); these run
// concurrently, one per GPU (utterances are independent: SURVEY 8e, no exchange between devices).
void worker(const Options &o, int device, float sr, const std::vector<std::string> &files,
            std::atomic<size_t> &next, std::atomic<int> &failures)
{
    try {
        // (--logmel-nfft: the frames are nfft samples long, the window of WL samples lies centred in them)
        const long WL = (long)(sr * o.window_ms * 1e-3), S = (long)(sr * o.shift_ms * 1e-3);
        const long W = o.logmel_nfft > 0 ? (long)o.logmel_nfft : WL;
        // (a header that announces a sample rate of a few Hz -- found by mutating the reference's own sample1.wav, round 4 --
        // makes the window or the shift shorter than one sample: refused here, before anything divides by the shift)
        if (WL < 1 || S < 1) throw std::runtime_error("window or shift shorter than one sample at this sample rate");
        // The extractor (HIP start-up, code object load, tables: 0.1-0.3 s of a fresh process) is created on a helper
        // thread while this one claims and reads the first batch of files: reading needs nothing from the device.
        auto make_param = [&]() -> std::unique_ptr<MfccHip> {
            const int engine = o.batch_mb > 0 ? MFX_ENGINE_STREAM_KERNELS : 0;
            if (o.method == MFX_METHOD_TRAPS) { // batch entries only: no engine switch, no reference flush quirk to reproduce
                std::unique_ptr<TrapsHip> t(new TrapsHip(o.sample_limit, (int)W, (int)S, o.banks, sr, o.low, o.high, o.traps_len,
                                                         o.traps_dct, (Normalizer::norm_t)o.norm, (ParamBase::dyn_t)o.dyn, o.l1, o.l2,
                                                         o.norm_after_dyn, device));
                std::vector<float> window((size_t)W);
                for (long i = 0; i < W; ++i) // ASR_OCL.cpp:149-151
                    window[i] = (float)(0.56f - 0.46f * std::cos((2.0f * M_PI * i) / W)) / 32768.f;
                t->set_window(window.data());
                t->set_warp(o.alpha_min);
                if (g_time.on) g_time.t_created = now_ns();
                return std::unique_ptr<MfccHip>(std::move(t));
            }
            if (o.method == MFX_METHOD_KALDI) { // batch entries only; the Povey window, samples in the int16 range
                std::unique_ptr<KaldiHip> t(new KaldiHip(o.sample_limit, (int)W, (int)S, o.banks, sr, o.low, o.high, o.ceps, o.lift,
                                                         (Normalizer::norm_t)o.norm, (ParamBase::dyn_t)o.dyn, o.l1, o.l2, o.norm_after_dyn,
                                                         device, o.kaldi_flags, o.kaldi_energy_floor));
                std::vector<float> window((size_t)W);
                KaldiHip::povey_window((int)W, window.data());
                t->set_window(window.data());
                t->set_options(o.kaldi_preemph, o.kaldi_dc, o.kaldi_power);
                if (g_time.on) g_time.t_created = now_ns();
                return std::unique_ptr<MfccHip>(std::move(t));
            }
            if (o.method == MFX_METHOD_STFT_LOGMEL) { // batch entries only; the window is the periodic Hann, samples are scaled in the kernel
                std::unique_ptr<MfccHip> t(new LogmelHip(o.sample_limit, (int)W, (int)S, o.banks, sr, o.low, o.high, o.logmel_post, device));
                std::vector<float> window((size_t)W, 0.f); // (torch.stft's placement: left pad (W - WL) / 2)
                for (long i = 0; i < WL; ++i) window[(W - WL) / 2 + i] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)i / (double)WL));
                t->set_window(window.data());
                if (g_time.on) g_time.t_created = now_ns();
                return t;
            }
            std::unique_ptr<MfccHip> p(
                o.method == MFX_METHOD_PLP
                    ? new PlpHip(o.sample_limit, (int)W, (int)S, o.banks, sr, o.low, o.high, o.ceps, o.c0, o.lift, o.model_order,
                                 (Normalizer::norm_t)o.norm, (ParamBase::dyn_t)o.dyn, o.l1, o.l2, o.norm_after_dyn, device,
                                 o.bug_compat, engine)
                    : new MfccHip(o.sample_limit, (int)W, (int)S, o.banks, sr, o.low, o.high, o.ceps, o.c0, o.lift,
                                  (Normalizer::norm_t)o.norm, (ParamBase::dyn_t)o.dyn, o.l1, o.l2, o.norm_after_dyn, device,
                                  o.bug_compat, engine));
            std::vector<float> window((size_t)W);
            for (long i = 0; i < W; ++i) // ASR_OCL.cpp:149-151
                window[i] = (float)(0.56f - 0.46f * std::cos((2.0f * M_PI * i) / W)) / 32768.f;
            p->set_window(window.data());
            p->set_warp(o.alpha_min); // (the batch entries have no apply() to carry it; the per-file loop sets its own)
            if (g_time.on) g_time.t_created = now_ns();
            return p;
        };
        Batch slots[2]; // (declared before the extractor: their pinned buffers outlive nothing of it, and the first fills early)
        std::future<bool> prep;
        const int D = o.dyn == 0 ? 0 : o.dyn == 1 ? o.l1 : o.l1 + o.l2;
        const long long cap = (long long)o.batch_mb * 1024 * 1024 / 2;
        std::unique_ptr<MfccHip> param_owner;
        if (o.batch_mb > 0) {
            // largest block one set_input takes (parambase.cpp:12-13,16-19; the extractor reports the same number)
            const int limit0 = (int)std::floor(float(o.sample_limit - (W - S)) / S) * (int)S + (int)(W - S);
            std::future<std::unique_ptr<MfccHip>> created = std::async(std::launch::async, make_param);
            if (o.file_spk.empty()) // (--spk-file walks the list twice, on its own: below)
                prep = std::async(std::launch::async, [&, limit0] {
                    return prepare_batch(slots[0], o, files, next, sr, cap, limit0, (int)W, (int)S, D);
                });
            auto prep_wait = [&] {
                if (prep.valid()) prep.wait();
            };
            try {
                param_owner = created.get();
            } catch (...) {
                prep_wait();
                throw;
            }
            if (param_owner->get_input_buffer_size() != limit0) {
                prep_wait();
                throw std::runtime_error("input block size mismatch");
            }
        } else {
            param_owner = make_param();
        }
        MfccHip &param = *param_owner;
        struct LoopEnd { // (runs before the extractor is destroyed: declared after it)
            ~LoopEnd()
            {
                if (g_time.on) g_time.t_loop_end = now_ns();
            }
        } loop_end;
        Scratch sc;
        if (o.batch_mb > 0) {
            // ---- batches of whole files: read batch k + 1 and write batch k - 1 (helper threads) beside the device calls
            // of batch k (this thread)
            // (--pitch: rows of `width` floats, the extractor's `wd` and the three pitch features behind them)
            const int limit = param.get_input_buffer_size(), wd = param.get_output_data_width(), width = wd + (o.pitch ? 3 : 0);
            const int cols = wd / (1 + o.dyn);
            auto set_pitch = [&] { // the track parameters of tools/pitch_bench.py; process-kaldi-pitch-feats' defaults, pasted
                param.batch_set_pitch(0, (int)std::floor(sr / o.pitch_hi), (int)std::ceil(sr / o.pitch_lo), 0.f, 0.1f, 1.f, 16);
                param.batch_set_pitch_feats(0, 75, 75, 2, 2.f, 0.f, 2.f, 10.f, true);
            };
            const long double dt = o.bug_compat ? (long double)(o.shift_ms / sr) : o.shift_ms / 1000.0L;
            const long double t0 = o.bug_compat ? (long double)(0.5f * o.window_ms / sr) : 0.5L * o.window_ms / 1000.0L;
            std::vector<std::vector<char>> text_bufs((size_t)std::max(o.io_threads, 1));
            auto write_batch = [&](Batch *b) {
                const long long tww = g_time.on ? now_ns() : 0;
                const float *rows = (const float *)b->rows.p;
                parallel_for(b->items.size(), o.io_threads, [&](size_t k, int t) {
                    const BatchItem &it = b->items[k];
                    if (!it.error.empty() || it.stream) return;
                    try {
                        const long long tw0 = g_time.on ? now_ns() : 0;
                        const std::string &name = files[2 * it.file + 1];
                        FILE *fo = std::fopen(name.c_str(), o.htk ? "wb" : "w");
                        if (!fo) throw std::runtime_error("Can't create output file: " + name);
                        std::vector<char> &text = text_bufs[(size_t)t]; // (grown once per helper, not per file)
                        const float *r = rows + (size_t)it.row0 * b->width;
                        if (o.htk) {
                            write_htk_header(fo, (uint32_t)it.out_frames, o, b->width);
                            write_rows_htk(fo, r, (int)it.out_frames, b->width, text);
                        } else {
                            write_rows(fo, r, (int)it.out_frames, b->width, 0, t0, dt, text, 1);
                        }
                        std::fclose(fo);
                        if (g_time.on) {
                            g_time.write += now_ns() - tw0;
                            ++g_time.files;
                        }
                    } catch (const std::exception &e) {
                        std::fprintf(stderr, "Exception caught %s\n", e.what());
                        ++failures;
                    }
                });
                std::string log;
                for (const BatchItem &it : b->items)
                    if (it.error.empty() && !it.stream)
                        log += files[2 * it.file] + ": " + std::to_string(it.frames) + " frames x " + std::to_string(b->width) + "\n";
                {
                    static std::mutex print_lock;
                    std::lock_guard<std::mutex> g(print_lock);
                    std::fputs(log.c_str(), stdout);
                }
                if (g_time.on) g_time.write_wall += now_ns() - tww;
            };
            if (!o.file_spk.empty()) {
                // ---- --spk-file: two passes over the same batches (prepare_batch cuts the list by file sizes: the same cut
                // both times).  Pass 1 pools: every batch starts from the accumulators of the batches before it and writes
                // nothing.  Pass 2 normalises every batch with the final accumulators and writes its files.  A speaker's
                // files keep their order, so the statistics are those of one batch holding the whole list.  The reference
                // has no such rows: its single-block flush behaviour (B1) is not applied to them.
                const int Wn = o.norm_after_dyn ? wd : cols;
                std::vector<long long> count((size_t)o.n_spk, 0);
                std::vector<double> acc((size_t)o.n_spk * 4 * Wn, 0.0);
                bool have_prior = false;
                Batch &b = slots[0];
                for (int pass = 1; pass <= 2; ++pass) {
                    std::atomic<size_t> at{0};
                    while (prepare_batch(b, o, files, at, sr, cap, limit, (int)W, (int)S, D)) {
                        std::vector<long long> off, len, row0;
                        std::vector<int> spk, rates;
                        std::vector<float> al;
                        std::vector<BatchItem *> in_batch;
                        for (BatchItem &it : b.items) {
                            if (!it.error.empty()) throw std::runtime_error(it.error);
                            if (it.stream)
                                throw std::runtime_error("--spk-file: \"" + files[2 * it.file] +
                                                         "\" would take the per-file loop (longer than one block, too short for the "
                                                         "deltas, or an alpha sweep): speakers are pooled over batches of whole files only");
                            off.push_back(it.off);
                            len.push_back(it.len);
                            spk.push_back(o.file_spk[it.file]);
                            rates.push_back(it.rate);
                            if (!o.file_alpha.empty()) al.push_back(o.file_alpha[it.file]);
                            in_batch.push_back(&it);
                        }
                        row0.resize(in_batch.size());
                        b.width = width;
                        b.total_rows = o.resample_to > 0 ? param.batch_plan_rates((int)in_batch.size(), off.data(), len.data(), rates.data(),
                                                                                  o.resample_zeros, row0.data())
                                                         : param.batch_plan((int)in_batch.size(), off.data(), len.data(), row0.data());
                        if (!al.empty()) param.batch_set_alphas(al.data(), (int)al.size());
                        param.batch_set_speakers(spk.data(), (int)spk.size(), o.n_spk, have_prior ? count.data() : nullptr,
                                                 have_prior ? acc.data() : nullptr, pass == 2);
                        if (o.pitch && pass == 2) set_pitch(); // (ahead of the VAD, which is sized for the wide rows)
                        if (o.vad && pass == 2) // (the rows that are written: selected from the normalised ones)
                            param.batch_set_vad(o.vad_column, o.vad_energy_threshold, o.vad_energy_mean_scale, o.vad_frames_context,
                                                o.vad_proportion_threshold, MFX_VAD_SELECT);
                        float *rows = (float *)b.rows.get((size_t)std::max<long long>(b.total_rows, 1) * width * sizeof(float));
                        param.batch_run_host((const short *)b.pcm.p, b.samples, rows);
                        if (pass == 1) {
                            if (b.total_rows > 0) {
                                param.batch_speaker_stats(count.data(), acc.data(), nullptr);
                                have_prior = true;
                            }
                            continue;
                        }
                        std::vector<int> voiced(in_batch.size());
                        if (o.vad) param.batch_vad_read(nullptr, voiced.data(), nullptr);
                        for (size_t k = 0; k < in_batch.size(); ++k) {
                            in_batch[k]->row0 = row0[k];
                            if (in_batch[k]->frames != param.batch_frames(in_batch[k]->conv_len)) throw std::runtime_error("frame count mismatch");
                            in_batch[k]->out_frames = o.vad ? voiced[k] : in_batch[k]->frames;
                        }
                        write_batch(&b);
                    }
                }
                return;
            }
            int cur = 0;
            std::future<void> writer;
            for (;;) {
                const long long tw0 = g_time.on ? now_ns() : 0;
                const bool have = prep.get();
                if (g_time.on) g_time.wait_read += now_ns() - tw0;
                if (!have) break;
                Batch &b = slots[cur];
                const int nxt = cur ^ 1;
                {
                    const long long t_ww = g_time.on ? now_ns() : 0;
                    if (writer.valid()) writer.get(); // the other slot's rows are on disk: it may be refilled
                    if (g_time.on) g_time.wait_write += now_ns() - t_ww, ++g_time.batches;
                }
                prep = std::async(std::launch::async, [&, nxt] {
                    return prepare_batch(slots[nxt], o, files, next, sr, cap, limit, (int)W, (int)S, D);
                });
                for (const BatchItem &it : b.items)
                    if (!it.error.empty()) { // a bad file does not stop the queue
                        std::fprintf(stderr, "Exception caught %s\n", it.error.c_str());
                        ++failures;
                    }
                // ---- device: one plan + one run for all batchable files
                std::vector<long long> off, len, row0;
                std::vector<BatchItem *> in_batch;
                for (BatchItem &it : b.items)
                    if (it.error.empty() && !it.stream) {
                        off.push_back(it.off);
                        len.push_back(it.len);
                        in_batch.push_back(&it);
                    }
                b.width = width;
                b.total_rows = 0;
                if (!in_batch.empty()) {
                    const long long td0 = g_time.on ? now_ns() : 0;
                    row0.resize(in_batch.size());
                    if (o.resample_to > 0) { // every file with its own rate: files at the extractor's rate are copied
                        std::vector<int> rates;
                        for (const BatchItem *it : in_batch) rates.push_back(it->rate);
                        b.total_rows = param.batch_plan_rates((int)in_batch.size(), off.data(), len.data(), rates.data(), o.resample_zeros,
                                                              row0.data());
                    } else {
                        b.total_rows = param.batch_plan((int)in_batch.size(), off.data(), len.data(), row0.data());
                    }
                    if (!o.file_alpha.empty()) { // --alpha-file: every file of the batch with its own factor, one run
                        std::vector<float> al;
                        for (const BatchItem *it : in_batch) al.push_back(o.file_alpha[it->file]);
                        param.batch_set_alphas(al.data(), (int)al.size());
                    }
                    if (o.online_window >= 0) // --online-window: every file normalised causally, as a live stream would be
                        param.batch_set_online_norm(o.online_window, o.online_prior_frames);
                    if (o.pitch) set_pitch(); // (ahead of the VAD, which is sized for the wide rows)
                    if (o.cmn_window > 0) // --cmn-window: behind the paste (all columns are normalised); the VAD decides on the raw rows
                        param.batch_set_sliding_norm(o.cmn_window, o.cmn_min_window, o.cmn_center, o.cmn_norm_vars ? 1 : 0);
                    if (o.vad)
                        param.batch_set_vad(o.vad_column, o.vad_energy_threshold, o.vad_energy_mean_scale, o.vad_frames_context,
                                            o.vad_proportion_threshold, MFX_VAD_SELECT);
                    float *rows = (float *)b.rows.get((size_t)std::max<long long>(b.total_rows, 1) * width * sizeof(float));
                    param.batch_run_host((const short *)b.pcm.p, b.samples, rows);
                    std::vector<int> voiced(in_batch.size());
                    if (o.vad) param.batch_vad_read(nullptr, voiced.data(), nullptr);
                    for (size_t k = 0; k < in_batch.size(); ++k) {
                        BatchItem &it = *in_batch[k];
                        it.row0 = row0[k];
                        if (it.frames != param.batch_frames(it.conv_len)) throw std::runtime_error("frame count mismatch");
                        it.out_frames = o.vad ? voiced[k] : it.frames;
                        if (o.vad) continue; // (selected rows have no reference analogue: nothing of B1 to reproduce on them)
                        if (o.online_window >= 0) continue; // (nor have causally normalised rows)
                        if (o.cmn_window > 0) continue;     // (nor rows normalised over a sliding window)
                        // The reference's flush after exactly one set_input reads its D static rows D rows early (B1,
                        // mfcccpu.cpp:439 + segmentercpu.cpp:97-106): rows T - D .. T - 1 repeat the statics of rows
                        // T - 2 D .. T - D - 1 (deltas unaffected).  The batch entries deliver the correct rows; the
                        // per-file loop this replaces reproduces the reference when --bug-compat is on, so do we.
                        // (not for a converted file: the reference has no rows for it, and it may be shorter than 2 D frames)
                        if (o.bug_compat && D > 0 && o.method != MFX_METHOD_TRAPS && o.method != MFX_METHOD_KALDI && (float)it.rate == sr)
                            for (int i = 0; i < D; ++i)
                                std::memcpy(rows + (size_t)(it.row0 + it.frames - D + i) * width,
                                            rows + (size_t)(it.row0 + it.frames - 2 * D + i) * width, (size_t)cols * sizeof(float));
                    }
                    if (g_time.on) g_time.device += now_ns() - td0;
                }
                // ---- files that need the per-file loop (longer than one block, too short, alpha sweeps)
                for (BatchItem &it : b.items)
                    if (it.error.empty() && it.stream) {
                        try {
                            if (o.online_window >= 0)
                                throw std::runtime_error("--online-window: \"" + files[2 * it.file] +
                                                         "\" would take the per-file loop (longer than one block, too short for the "
                                                         "deltas, or an alpha sweep): the online normaliser runs in batches of whole files only");
                            if (o.cmn_window > 0)
                                throw std::runtime_error("--cmn-window: \"" + files[2 * it.file] +
                                                         "\" would take the per-file loop (longer than one block, too short for the "
                                                         "deltas, or an alpha sweep): the sliding-window normaliser runs in batches of whole files only");
                            if (o.pitch)
                                throw std::runtime_error("--pitch: \"" + files[2 * it.file] +
                                                         "\" would take the per-file loop (longer than one block, too short for the "
                                                         "deltas, or an alpha sweep): the pitch features run in batches of whole files only");
                            if (o.vad)
                                throw std::runtime_error("--vad: \"" + files[2 * it.file] +
                                                         "\" would take the per-file loop (longer than one block, too short for the "
                                                         "deltas, or an alpha sweep): frames are selected in batches of whole files only");
                            process_file(param, o, it.wav, files[2 * it.file], files[2 * it.file + 1], sr, sc,
                                         o.file_alpha.empty() ? nullptr : &o.file_alpha[it.file]);
                        } catch (const std::exception &e) {
                            std::fprintf(stderr, "Exception caught %s\n", e.what());
                            ++failures;
                        }
                    }
                writer = std::async(std::launch::async, write_batch, &b);
                cur = nxt;
            }
            if (writer.valid()) writer.get();
            return;
        }
        // The worker's next file is claimed and read (its own thread) while the current one is on the GPU.
        // The worker's next file is claimed and read (its own thread) while the current one is on the GPU.
        struct Pending {
            size_t i;
            std::future<Wav> wav;
        };
        auto claim = [&](Pending &p) -> bool {
            p.i = next.fetch_add(1);
            if (2 * p.i + 1 >= files.size()) return false;
            p.wav = std::async(std::launch::async, read_wav, files[2 * p.i]);
            return true;
        };
        Pending cur, nxt;
        bool have = claim(cur);
        while (have) {
            const bool have_next = claim(nxt);
            try {
                const long long tw0 = g_time.on ? now_ns() : 0;
                const Wav w = cur.wav.get();
                if (g_time.on) g_time.wait_read += now_ns() - tw0;
                process_file(param, o, w, files[2 * cur.i], files[2 * cur.i + 1], sr, sc,
                             o.file_alpha.empty() ? nullptr : &o.file_alpha[cur.i]);
            } catch (const std::exception &e) { // a bad file does not stop the queue
                std::fprintf(stderr, "Exception caught %s\n", e.what());
                ++failures;
            }
            cur = std::move(nxt);
            have = have_next;
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "Exception caught %s\n", e.what());
        ++failures;
    }
}

} // namespace

int main(int argc, char **argv)
{
    g_time.t_main = now_ns();
    Options o;
    std::vector<std::string> files;
    bool alpha_options = false; // any of --alpha, --alpha-min, --alpha-max, --alpha-step
    bool kaldi_opts = false;    // any of --preemph, --no-dc-removal, --magnitude
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> const char * {
            if (i + 1 >= argc) {
                std::fprintf(stderr, "missing value for %s\n", a.c_str());
                std::exit(2);
            }
            return argv[++i];
        };
        if (a == "--alpha" || a == "--alpha-min" || a == "--alpha-max" || a == "--alpha-step") alpha_options = true;
        if (a == "--window-size") o.window_ms = (float)std::atof(val());
        else if (a == "--shift") o.shift_ms = (float)std::atof(val());
        else if (a == "--banks") o.banks = std::atoi(val());
        else if (a == "--ceps") o.ceps = std::atoi(val());
        else if (a == "--c0") o.c0 = std::atoi(val()) != 0;
        else if (a == "--norm") o.norm = std::atoi(val());
        else if (a == "--dyn") o.dyn = std::atoi(val());
        else if (a == "--l1") o.l1 = std::atoi(val());
        else if (a == "--l2") o.l2 = std::atoi(val());
        else if (a == "--low-freq") o.low = (float)std::atof(val()), o.low_given = true;
        else if (a == "--high-freq") o.high = (float)std::atof(val());
        else if (a == "--lift-coef") o.lift = (float)std::atof(val());
        else if (a == "--norm-after-dyn") o.norm_after_dyn = std::atoi(val()) != 0;
        else if (a == "--alpha") o.alpha_min = o.alpha_max = (float)std::atof(val());
        else if (a == "--alpha-min") o.alpha_min = (float)std::atof(val());
        else if (a == "--alpha-max") o.alpha_max = (float)std::atof(val());
        else if (a == "--alpha-step") o.alpha_step = (float)std::atof(val());
        else if (a == "--alpha-file") o.alpha_file = val();
        else if (a == "--spk-file") o.spk_file = val();
        else if (a == "--online-window") o.online_window = std::atoi(val());
        else if (a == "--online-prior-frames") o.online_prior_frames = std::atoi(val());
        else if (a == "--cmn-window") o.cmn_window = std::atoi(val()), o.cmn_options = true;
        else if (a == "--cmn-center") o.cmn_center = std::atoi(val()), o.cmn_options = true;
        else if (a == "--cmn-min-window") {
            const int m = std::atoi(val());
            o.cmn_min_window = m < 0 ? -2 : m; // (-1 is "not given": a negative value is refused below)
            o.cmn_options = true;
        }
        else if (a == "--cmn-norm-vars") o.cmn_norm_vars = o.cmn_options = true;
        else if (a == "--selftest-spk-labels") { // the label -> id mapping of --spk-file, on a file of labels: prints the ids
            FILE *fl = std::fopen(val(), "r");
            if (!fl) {
                std::fprintf(stderr, "can't read the label file\n");
                return 2;
            }
            std::vector<std::string> labels;
            read_label_lines(fl, labels);
            std::fclose(fl);
            std::vector<int> ids;
            const int n = map_speaker_labels(labels, ids);
            std::printf("%d speakers:", n);
            for (int id : ids) std::printf(" %d", id);
            std::printf("\n");
            return 0;
        }
        else if (a == "--sample-limit") o.sample_limit = std::atoi(val());
        else if (a == "--dev") o.device = std::atoi(val());
        else if (a == "--devs") { // comma separated device list; an id may repeat (two workers on one GPU)
            for (const char *q = val(); *q;) {
                o.devices.push_back((int)std::strtol(q, const_cast<char **>(&q), 10));
                if (*q == ',') ++q;
                else if (*q) { std::fprintf(stderr, "bad --devs list\n"); return 2; }
            }
        }
        else if (a == "--bug-compat") o.bug_compat = std::atoi(val()) != 0;
        else if (a == "--htk") o.htk = true;
        else if (a == "--method") { // the reference's names (ASR_OCL.cpp:54-56)
            const std::string m = val();
            if (m == "MFCC") o.method = MFX_METHOD_MFCC;
            else if (m == "PLP") o.method = MFX_METHOD_PLP;
            else if (m == "TRAPS") o.method = MFX_METHOD_TRAPS;
            else if (m == "LOGMEL") o.method = MFX_METHOD_STFT_LOGMEL;
            else if (m == "KALDI") o.method = MFX_METHOD_KALDI;
            else { std::fprintf(stderr, "--method: MFCC, PLP, TRAPS, LOGMEL or KALDI\n"); return 2; }
        }
        else if (a == "--preemph") {
            o.kaldi_preemph = (float)std::atof(val());
            if (!(o.kaldi_preemph >= 0.f && o.kaldi_preemph <= 1.f)) { std::fprintf(stderr, "--preemph: 0 .. 1\n"); return 2; }
            kaldi_opts = true;
        }
        else if (a == "--no-dc-removal") o.kaldi_dc = false, kaldi_opts = true;
        else if (a == "--magnitude") o.kaldi_power = false, kaldi_opts = true;
        else if (a == "--snip-edges") {
            const int v = std::atoi(val());
            if (v != 0 && v != 1) { std::fprintf(stderr, "--snip-edges: 0 or 1\n"); return 2; }
            o.kaldi_flags = v ? (o.kaldi_flags & ~MFX_KALDI_NO_SNIP_EDGES) : (o.kaldi_flags | MFX_KALDI_NO_SNIP_EDGES);
            kaldi_opts = true;
        }
        else if (a == "--use-energy") o.kaldi_flags |= MFX_KALDI_USE_ENERGY, kaldi_opts = true;
        else if (a == "--raw-energy") {
            const int v = std::atoi(val());
            if (v != 0 && v != 1) { std::fprintf(stderr, "--raw-energy: 0 or 1\n"); return 2; }
            o.kaldi_raw_energy = v != 0, kaldi_opts = true;
        }
        else if (a == "--energy-floor") {
            o.kaldi_energy_floor = (float)std::atof(val());
            if (!(o.kaldi_energy_floor >= 0.f) || !std::isfinite(o.kaldi_energy_floor)) { std::fprintf(stderr, "--energy-floor: >= 0\n"); return 2; }
            kaldi_opts = true;
        }
        else if (a == "--htk-compat") o.kaldi_flags |= MFX_KALDI_HTK_COMPAT, kaldi_opts = true;
        else if (a == "--traps-length") o.traps_len = std::atoi(val());
        else if (a == "--traps-dct") o.traps_dct = std::atoi(val());
        else if (a == "--logmel-nfft") {
            o.logmel_nfft = std::atoi(val());
            if (o.logmel_nfft != 1024 && o.logmel_nfft != 2048) { std::fprintf(stderr, "--logmel-nfft: 1024 or 2048\n"); return 2; }
        }
        else if (a == "--logmel-post") {
            const std::string m = val();
            if (m == "whisper") o.logmel_post = MFX_LOGMEL_WHISPER;
            else if (m == "log10") o.logmel_post = MFX_LOGMEL_LOG10;
            else if (m == "ln") o.logmel_post = MFX_LOGMEL_LN;
            else { std::fprintf(stderr, "--logmel-post: whisper, log10 or ln\n"); return 2; }
        }
        else if (a == "--model-order") o.model_order = std::atoi(val());
        else if (a == "--timing") g_time.on = true;
        else if (a == "--format-threads") o.format_threads = std::max(1, std::atoi(val()));
        else if (a == "--batch-mb") o.batch_mb = std::max(0, std::atoi(val()));
        else if (a == "--io-threads") o.io_threads = std::max(1, std::atoi(val()));
        else if (a == "--resample-to") o.resample_to = std::atoi(val());
        else if (a == "--resample-zeros") o.resample_zeros = std::atoi(val());
        else if (a == "--vad") o.vad = true;
        else if (a == "--pitch") o.pitch = true;
        else if (a == "--pitch-range") {
            if (std::sscanf(val(), "%f:%f", &o.pitch_lo, &o.pitch_hi) != 2 || !(o.pitch_lo > 0.f) || !(o.pitch_hi > o.pitch_lo) ||
                !std::isfinite(o.pitch_hi)) {
                std::fprintf(stderr, "--pitch-range: LO:HI in Hz, 0 < LO < HI\n");
                return 2;
            }
        }
        else if (a == "--vad-energy-threshold") o.vad_energy_threshold = (float)std::atof(val());
        else if (a == "--vad-energy-mean-scale") o.vad_energy_mean_scale = (float)std::atof(val());
        else if (a == "--vad-frames-context") o.vad_frames_context = std::atoi(val());
        else if (a == "--vad-proportion-threshold") o.vad_proportion_threshold = (float)std::atof(val());
        else if (a == "--vad-column") o.vad_column = std::atoi(val());
        else if (a == "--selftest-format") { // put_f32 against printf("%f") on n random bit patterns + the known hard cases
            const long n = std::atol(val());
            uint64_t st = 0x9E3779B97F4A7C15ull;
            long bad = 0;
            auto check = [&](float v) {
                char a1[128], a2[128];
                char *e1 = put_f32(a1, a1 + sizeof(a1), v);
                *e1 = 0;
                std::snprintf(a2, sizeof(a2), "%f", (double)v);
                if (std::strcmp(a1, a2) != 0 && ++bad < 10) std::fprintf(stderr, "put_f32 mismatch: %s vs %s\n", a1, a2);
            };
            const float hard[] = {0.f, -0.f, 1.f / 128, -1.f / 128, 0.5e-6f, 1.5e-6f, 2.5e-6f, 1e-10f, -1e-10f, 1e-45f, 123456.789f,
                                  -69.07755f, 0.9999995f, 0.99999994f, 9.9999995f, 16777216.f, 1e12f, 1.0995116e12f, 3.4e38f,
                                  -3.4e38f, 0.0078125f, 0.0234375f, 1.0000005f, 4194304.5f, 8388607.5f};
            for (float v : hard) check(v);
            check(std::nanf(""));
            check(INFINITY);
            check(-INFINITY);
            for (long i = 0; i < n; ++i) {
                st ^= st << 13, st ^= st >> 7, st ^= st << 17; // xorshift64
                uint32_t b = (uint32_t)(st >> 16);
                float v;
                std::memcpy(&v, &b, 4);
                check(v);
                // and values in the range features actually take
                check((float)((double)(int32_t)(st >> 33) * 1e-7));
            }
            std::printf("put_f32 selftest: %ld mismatches\n", bad);
            return bad ? 1 : 0;
        }
        else if (a == "--help") {
            std::printf("afet_hip [--window-size ms] [--shift ms] [--banks n] [--ceps n] [--c0 0|1] [--norm 0..3]\n"
                        "         [--dyn 0..2] [--l1 n] [--l2 n] [--low-freq hz] [--high-freq hz] [--lift-coef x]\n"
                        "         [--norm-after-dyn 0|1] [--alpha a | --alpha-min a --alpha-max b --alpha-step s | --alpha-file f]\n"
                        "         [--sample-limit n] [--dev n | --devs a,b,...] [--bug-compat 0|1] [--htk]  in.wav out.txt [...]\n"
                        "         [--method MFCC|PLP|TRAPS|LOGMEL|KALDI] [--model-order n (PLP model order, default 8)]\n"
                        "         [--preemph x] [--no-dc-removal] [--magnitude] (KALDI: Kaldi-compatible fbank (--ceps 0) / MFCC with c0 first,\n"
                        "          Povey window, --high-freq <= 0 an offset from Nyquist, --lift-coef the cepstral lifter; defaults 0.97, DC removal, power)\n"
                        "         [--snip-edges 0|1] [--use-energy] [--raw-energy 0|1] [--energy-floor x] [--htk-compat] (KALDI: Kaldi's options of\n"
                        "          those names; --use-energy puts the frame's log-energy in column 0 -- fbank rows are one column wider --,\n"
                        "          --htk-compat moves it, or c0 times sqrt 2, behind the others; defaults 1, off, 1, 0, off)\n"
                        "         [--logmel-post whisper|log10|ln (LOGMEL: what follows the log; default whisper)]\n"
                        "         [--logmel-nfft 1024|2048 (LOGMEL: the DFT length; the Hann window of --window-size lies centred in it)]\n"
                        "         [--traps-length n (TRAPS frames per trajectory, odd, default 31)] [--traps-dct n (default 10)]\n"
                        "         [--batch-mb n (PCM per batch of whole files; 0 = per-file loop)] [--io-threads n]\n"
                        "  --alpha-file: one warp factor per line, in the order of the input files; files of a batch run with\n"
                        "                their own factors in one launch sequence\n"
                        "  --spk-file: one speaker label per line, in the order of the input files (needs --norm 1..3, batches, one\n"
                        "                device): CMN / CVN / MINMAX statistics pooled over each speaker's files, in two passes\n"
                        "         [--online-window n [--online-prior-frames f]]\n"
                        "  --online-window: online (causal) CMN / CVN (needs --norm 1|2, batches; excludes --spk-file): every row is\n"
                        "                normalised with the last n rows of its file, itself included (0: all rows so far; else a\n"
                        "                multiple of 32 up to 4096).  --online-prior-frames is handed on for a prior, of which the\n"
                        "                driver has none to give: it changes nothing yet\n"
                        "         [--cmn-window n [--cmn-center 0|1] [--cmn-min-window m] [--cmn-norm-vars]]\n"
                        "  --cmn-window: sliding-window CMN, with --cmn-norm-vars CVN (apply-cmvn-sliding; needs --norm 0, batches;\n"
                        "                excludes --spk-file and --online-window): every row is normalised with the statistics of n\n"
                        "                rows of its file (1 .. 4096) around it (--cmn-center 1) or behind it (default; at least\n"
                        "                --cmn-min-window of them at a file's start, default 100).  All columns, pasted pitch features\n"
                        "                included; --vad decides on the rows as they were before.  Restated from Kaldi's\n"
                        "                SlidingWindowCmn; agreement with a Kaldi binary has not been measured\n"
                        "         [--resample-to hz [--resample-zeros n]]\n"
                        "  --resample-to: extract at hz instead of the first file's rate; files at other rates are converted on the\n"
                        "                device (Hann-windowed sinc, n zero crossings per side, default 6)\n"
                        "         [--vad [--vad-energy-threshold x] [--vad-energy-mean-scale x] [--vad-frames-context n]\n"
                        "          [--vad-proportion-threshold x] [--vad-column n]]\n"
                        "  --vad: energy voice-activity decision on the device (needs batches); every output file holds its voiced\n"
                        "                rows only.  Defaults 5, 0.5, 0, 0.6 (compute-vad-energy's); column -1 = the last static one\n"
                        "         [--pitch [--pitch-range LO:HI]]\n"
                        "  --pitch: pitch track on the device and Kaldi's three pitch features from it (probability of voicing,\n"
                        "                normalised log-pitch, delta log-pitch; process-kaldi-pitch-feats' defaults) as three more\n"
                        "                columns of every row (needs batches; not with --method LOGMEL).  Lags of LO .. HI Hz are\n"
                        "                searched, default 50:400\n"
                        "  --devs: one worker per listed GPU, files dealt from a shared queue\n"
                        "  inputs: RIFF/WAVE or NIST SPHERE, 16-bit PCM; output: the reference's text rows, or HTK binary\n");
            return 0;
        } else files.push_back(a);
    }
    if (files.empty() || files.size() % 2) {
        std::fprintf(stderr, "usage: afet_hip [options] in.wav out.txt [in2.wav out2.txt ...]  (--help)\n");
        return 2;
    }
    if (!o.alpha_file.empty()) {
        if (alpha_options) {
            std::fprintf(stderr, "--alpha-file excludes --alpha and --alpha-min / --alpha-max / --alpha-step\n");
            return 2;
        }
        FILE *fa = std::fopen(o.alpha_file.c_str(), "r");
        if (!fa) {
            std::fprintf(stderr, "can't read --alpha-file %s\n", o.alpha_file.c_str());
            return 2;
        }
        char line[256];
        while (std::fgets(line, sizeof(line), fa)) {
            char *end = nullptr;
            const float v = std::strtof(line, &end);
            if (end == line) continue; // (blank line)
            if (!(v > 0.f)) {
                std::fprintf(stderr, "--alpha-file: warp factors must be positive\n");
                std::fclose(fa);
                return 2;
            }
            o.file_alpha.push_back(v);
        }
        std::fclose(fa);
        if (o.file_alpha.size() != files.size() / 2) {
            std::fprintf(stderr, "--alpha-file holds %zu warp factors for %zu input files\n", o.file_alpha.size(), files.size() / 2);
            return 2;
        }
    }
    if (o.pitch && o.batch_mb <= 0) {
        std::fprintf(stderr, "--pitch tracks whole files in batches: --batch-mb must be positive\n");
        return 2;
    }
    if (o.pitch && o.method == MFX_METHOD_STFT_LOGMEL) {
        std::fprintf(stderr, "--pitch is not served with --method LOGMEL: its frames are centred, the pitch track's are not\n");
        return 2;
    }
    if (o.vad && o.batch_mb <= 0) {
        std::fprintf(stderr, "--vad selects frames in batches of whole files: --batch-mb must be positive\n");
        return 2;
    }
    if (o.online_window != -1 || o.online_prior_frames != 0) {
        if (o.online_window < 0 || o.online_window > 4096 || o.online_window % 32 != 0) {
            std::fprintf(stderr, "--online-window must be 0 or a multiple of 32 up to 4096 (--online-prior-frames needs it)\n");
            return 2;
        }
        if (o.online_prior_frames < 0 || o.online_prior_frames > (1 << 20)) {
            std::fprintf(stderr, "--online-prior-frames must be 0 .. 1048576\n");
            return 2;
        }
        if (o.norm != 1 && o.norm != 2) {
            std::fprintf(stderr, "--online-window is an online CMN / CVN: it needs --norm 1 or 2\n");
            return 2;
        }
        if (o.batch_mb <= 0) {
            std::fprintf(stderr, "--online-window runs in batches of whole files: --batch-mb must be positive\n");
            return 2;
        }
        if (!o.spk_file.empty()) {
            std::fprintf(stderr, "--online-window and --spk-file exclude each other: one normaliser per run\n");
            return 2;
        }
    }
    if (o.cmn_options) {
        if (o.cmn_window < 1 || o.cmn_window > 4096) {
            std::fprintf(stderr, "--cmn-window must be 1 .. 4096 (--cmn-center, --cmn-min-window and --cmn-norm-vars need it)\n");
            return 2;
        }
        if (o.cmn_center != 0 && o.cmn_center != 1) {
            std::fprintf(stderr, "--cmn-center must be 0 or 1\n");
            return 2;
        }
        if (o.cmn_min_window == -1) o.cmn_min_window = std::min(100, o.cmn_window);
        if (o.cmn_min_window < 0 || o.cmn_min_window > o.cmn_window) {
            std::fprintf(stderr, "--cmn-min-window must be 0 .. --cmn-window\n");
            return 2;
        }
        if (o.norm != 0) {
            std::fprintf(stderr, "--cmn-window replaces the other normalisers, it does not stack on them: it needs --norm 0\n");
            return 2;
        }
        if (o.method == MFX_METHOD_STFT_LOGMEL) {
            std::fprintf(stderr, "--cmn-window is not served with --method LOGMEL\n");
            return 2;
        }
        if (o.batch_mb <= 0) {
            std::fprintf(stderr, "--cmn-window runs in batches of whole files: --batch-mb must be positive\n");
            return 2;
        }
        if (!o.spk_file.empty() || o.online_window != -1) {
            std::fprintf(stderr, "--cmn-window excludes --spk-file and --online-window: one normaliser per run\n");
            return 2;
        }
    }
    if (!o.spk_file.empty()) {
        if (o.norm < 1 || o.norm > 3) {
            std::fprintf(stderr, "--spk-file pools the normaliser's statistics: it needs --norm 1, 2 or 3\n");
            return 2;
        }
        if (o.batch_mb <= 0) {
            std::fprintf(stderr, "--spk-file pools speakers over batches of whole files: --batch-mb must be positive\n");
            return 2;
        }
        if (o.devices.size() > 1) {
            std::fprintf(stderr, "--spk-file runs on one device: --devs names more than one\n");
            return 2;
        }
        FILE *fs = std::fopen(o.spk_file.c_str(), "r");
        if (!fs) {
            std::fprintf(stderr, "can't read --spk-file %s\n", o.spk_file.c_str());
            return 2;
        }
        std::vector<std::string> labels;
        read_label_lines(fs, labels);
        std::fclose(fs);
        if (labels.size() != files.size() / 2) {
            std::fprintf(stderr, "--spk-file holds %zu labels for %zu input files\n", labels.size(), files.size() / 2);
            return 2;
        }
        o.n_spk = map_speaker_labels(labels, o.file_spk);
    }
    if (o.method == MFX_METHOD_TRAPS) { // whole files through the batch entries: no per-file loop, no alpha loop, no DCT options
        if (o.batch_mb <= 0) {
            std::fprintf(stderr, "--method TRAPS runs whole files through the batch entries: --batch-mb must be positive\n");
            return 2;
        }
        if (o.alpha_max - o.alpha_min >= o.alpha_step) {
            std::fprintf(stderr, "--method TRAPS takes one warp factor (--alpha), not a sweep\n");
            return 2;
        }
    }
    if (o.method == MFX_METHOD_STFT_LOGMEL) { // whole files through the batch entries; log mel bands, nothing behind them
        if (o.batch_mb <= 0) {
            std::fprintf(stderr, "--method LOGMEL runs whole files through the batch entries: --batch-mb must be positive\n");
            return 2;
        }
        if (o.alpha_max - o.alpha_min >= o.alpha_step) {
            std::fprintf(stderr, "--method LOGMEL has no warp factor to sweep\n");
            return 2;
        }
        // (the reference CLI's defaults -- 64 Hz, cepstra with c0, deltas, CVN -- belong to the cepstral methods)
        o.ceps = 0, o.c0 = false, o.dyn = 0, o.norm = 0;
        if (!o.low_given) o.low = 0.f;
    } else if (o.logmel_nfft > 0) {
        std::fprintf(stderr, "--logmel-nfft goes with --method LOGMEL\n");
        return 2;
    }
    if (o.method == MFX_METHOD_KALDI) { // whole files through the batch entries; c0 is column 0 of the cepstra, there is no warp
        if (o.batch_mb <= 0) {
            std::fprintf(stderr, "--method KALDI runs whole files through the batch entries: --batch-mb must be positive\n");
            return 2;
        }
        if (o.alpha_max - o.alpha_min >= o.alpha_step || !o.alpha_file.empty()) {
            std::fprintf(stderr, "--method KALDI has no warp factor\n");
            return 2;
        }
        o.c0 = false, o.bug_compat = false;
        if (!o.low_given) o.low = 20.f; // (Kaldi's default)
        if (!o.kaldi_raw_energy) {
            if (!(o.kaldi_flags & MFX_KALDI_USE_ENERGY)) {
                std::fprintf(stderr, "--raw-energy 0 goes with --use-energy\n");
                return 2;
            }
            o.kaldi_flags |= MFX_KALDI_ENERGY_WINDOWED;
        }
        if (o.kaldi_flags != 0 && (o.kaldi_flags & ~mfx_kaldi_flags_supported()) != 0) {
            std::fprintf(stderr, "this libmfcchip.so does not serve these Kaldi options\n");
            return 2;
        }
    } else if (kaldi_opts) {
        std::fprintf(stderr, "--preemph, --no-dc-removal, --magnitude, --snip-edges, --use-energy, --raw-energy, --energy-floor and --htk-compat go with --method KALDI\n");
        return 2;
    }
    if (o.resample_to != 0 && (o.resample_to < 1000 || o.resample_to > 768000)) {
        std::fprintf(stderr, "--resample-to takes a rate of 1000 .. 768000 Hz\n");
        return 2;
    }
    if (o.resample_zeros < 0 || o.resample_zeros > 64) {
        std::fprintf(stderr, "--resample-zeros takes 1 .. 64\n");
        return 2;
    }
    try {
        // sample rate from the first file (ASR_OCL.cpp:342-358), unless --resample-to names it
        const float sr = o.resample_to > 0 ? (float)o.resample_to : (float)read_wav(files[0]).sample_rate;
        if (o.high <= 0 && o.method != MFX_METHOD_KALDI) o.high = sr / 2; // (KALDI: <= 0 is the library's offset from Nyquist)
        if (o.logmel_nfft > 0 && (long)(sr * o.window_ms * 1e-3) > (long)o.logmel_nfft) {
            std::fprintf(stderr, "--window-size is %ld samples at %g Hz: longer than --logmel-nfft %d\n", (long)(sr * o.window_ms * 1e-3), (double)sr,
                         o.logmel_nfft);
            return 2;
        }
        if (o.devices.empty()) o.devices.push_back(o.device);
        std::atomic<size_t> next{0};
        std::atomic<int> failures{0};
        if (o.devices.size() == 1) {
            worker(o, o.devices[0], sr, files, next, failures);
        } else {
            std::vector<std::thread> pool;
            for (int d : o.devices) pool.emplace_back(worker, std::cref(o), d, sr, std::cref(files), std::ref(next), std::ref(failures));
            for (auto &t : pool) t.join();
        }
        if (g_time.on) g_time.t_destroyed = now_ns();
        if (g_time.on && g_time.files > 0) {
            const double n = (double)g_time.files.load();
            std::fprintf(stderr, "process milestones (ms): start -> extractor created %.1f, file loop %.1f (%.0f files/s inside the loop), "
                                 "extractor destroyed %.1f\n", (g_time.t_created - g_time.t_main) / 1e6,
                         (g_time.t_loop_end - g_time.t_created) / 1e6, n / ((g_time.t_loop_end - g_time.t_created) / 1e9),
                         (g_time.t_destroyed - g_time.t_loop_end) / 1e6);
            std::fprintf(stderr, "timing per file (us): waiting for the reader %.0f, host preparation %.0f, device calls %.0f, "
                                 "formatting + writing %.0f", g_time.wait_read / n / 1e3, g_time.prep / n / 1e3,
                         g_time.device / n / 1e3, g_time.write / n / 1e3);
            if (g_time.batches > 0)
                std::fprintf(stderr, "; %lld batches, stage wall time per file: read + pack %.0f, write %.0f, waiting for the writer %.0f",
                             g_time.batches.load(), g_time.prep_wall / n / 1e3, g_time.write_wall / n / 1e3, g_time.wait_write / n / 1e3);
            std::fprintf(stderr, "\n");
        }
        return failures.load() ? 1 : 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "Exception caught %s\n", e.what());
        return 1;
    }
}
