// mfx_tables.cpp -- see mfx_tables.h.  Compiled with -ffp-contract=off so that the float32
// expression order below is what actually executes.
#include "mfx_tables.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <unordered_map>
#include <vector>

namespace mfx {

static const float kPiF = (float)3.14159265358979323846264338;

uint32_t ceil_pow2(uint32_t v)
{
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

int64_t frame_count(int64_t samples, int window_size, int shift)
{
    int64_t num = samples - (int64_t)(window_size - shift);
    // floor division (num may be negative for very short inputs)
    int64_t q = num / shift;
    if ((num % shift != 0) && ((num < 0) != (shift < 0))) --q;
    return q;
}

int32_t session_step(int window_size, int shift, int D, int64_t &n, int64_t &E, int64_t length, bool final_push, SessionStep &st)
{
    const int64_t T_old = std::max<int64_t>(frame_count(n, window_size, shift), 0);
    const int64_t f0 = std::max<int64_t>(E - D, 0);
    const int64_t n_new = n + length;
    const int64_t T_new = std::max<int64_t>(frame_count(n_new, window_size, shift), 0);
    const int64_t E_new = final_push ? T_new : std::max<int64_t>(T_new - D, 0);
    st.carry_samples = n - T_old * shift;
    st.carry_rows = (int32_t)(T_old - f0);
    st.new_frames = (int32_t)(T_new - T_old);
    st.n_out = (int32_t)(E_new - E);
    st.static_off = (int32_t)(E - f0);
    st.shift = st.static_off - D; // (row static_off - shift = D of the padded series is output row 0: k_delta's convention)
    st.lo = 0;
    st.hi = (int32_t)(T_new - 1 - f0); // (reached only by a final push: E_new + D <= T_new otherwise)
    n = final_push ? 0 : n_new;
    E = final_push ? 0 : E_new;
    return st.n_out;
}

int32_t session_xform_step(int left, int right, int64_t &Ey, int64_t &Ex, int32_t n_y, bool final_push, SessionXformStep &st)
{
    const int64_t c0 = std::max<int64_t>(Ex - left, 0);
    const int64_t Ey_new = Ey + n_y;
    const int64_t Ex_new = final_push ? Ey_new : std::max<int64_t>(Ey_new - right, 0);
    st.n_out = (int32_t)(Ex_new - Ex);
    st.carry_rows = (int32_t)(Ey - c0);
    st.src_row0 = (int32_t)(Ex - c0);
    st.lo = -st.src_row0;
    st.hi = (int32_t)(Ey_new - 1 - Ex);
    Ey = final_push ? 0 : Ey_new;
    Ex = final_push ? 0 : Ex_new;
    return st.n_out;
}

void pack_sess_xform_groups(const int32_t *n_out, const int32_t *xf, int n, int G, std::vector<SessXfCut> &groups, std::vector<SessXfPack> &blocks)
{
    groups.clear(), blocks.clear();
    for (int32_t i = 0; i < n; ++i)
        for (int32_t r0 = 0; r0 < n_out[i]; r0 += 16) groups.push_back(SessXfCut{i, r0, std::min(16, n_out[i] - r0)});
    std::stable_sort(groups.begin(), groups.end(), [&](const SessXfCut &a, const SessXfCut &b) { return xf[a.piece] < xf[b.piece]; });
    for (int32_t g = 0; g < (int32_t)groups.size(); ++g) {
        const int32_t x = xf[groups[g].piece];
        if (blocks.empty() || blocks.back().xf != x || blocks.back().ng == G) blocks.push_back(SessXfPack{g, 0, x});
        ++blocks.back().ng;
    }
}

int estimated_window_count_f32(int samples, int window_size, int shift)
{
    return (int)std::floor((float)(samples - (window_size - shift)) / (float)shift);
}

namespace {
inline float mel_of_hz(float f) { return 1127 * std::log(f / 700 + 1); }  // float overloads
inline float hz_of_mel(float m) { return 700 * (std::exp(m / 1127) - 1); }
inline int round_bin(float centre_hz, int fft_size, float sample_rate)
{
    // reference: floor(c * W2 / sr + 0.5) with the sum taken in double (mfcccpu.cpp:40,47-49)
    return (int)std::floor((double)(centre_hz * fft_size / sample_rate) + 0.5);
}
} // namespace

void build_mel_table(int num_banks, int fft_size, float sample_rate, float low_freq, float high_freq,
                     float alpha, MelTable &out)
{
    const int npts = num_banks + 2;
    std::vector<float> centre(npts);
    out.weights.assign((size_t)2 * fft_size, 0.0f);
    out.beg.assign(npts, 0);

    const float mel_lo = mel_of_hz(low_freq), mel_hi = mel_of_hz(high_freq);
    const float one_minus_alpha = 1 - alpha;
    for (int i = 0; i < npts; ++i) {
        float hz = hz_of_mel(i / float(num_banks + 1) * (mel_hi - mel_lo) + mel_lo);
        float omega = 2 * kPiF * hz / sample_rate;
        // VTLN bilinear warp; identity for alpha == 1 (mfcccpu.cpp:36-38)
        omega = omega + 2 * std::atan((one_minus_alpha * std::sin(omega)) / (1 - one_minus_alpha * std::cos(omega)));
        centre[i] = sample_rate * omega / (2 * kPiF);
        out.beg[i] = round_bin(centre[i], fft_size, sample_rate);
    }
    for (int m = 0; m < num_banks; ++m) {
        const float left = centre[m], mid = centre[m + 1], right = centre[m + 2];
        const int first = round_bin(left, fft_size, sample_rate);
        const int last = round_bin(right, fft_size, sample_rate);
        float *row = out.weights.data() + (size_t)(m & 1) * fft_size;
        for (int bin = first; bin < last; ++bin) {
            if (bin < 0 || bin >= fft_size) continue;
            float hz = bin * sample_rate / (fft_size);
            float rising = (hz - left) / (mid - left);
            float falling = (hz - right) / (mid - right);
            row[bin] = std::max(0.0f, std::min(rising, falling));
        }
    }
}

void build_plp_tables(int num_banks, float sample_rate, float low_freq, float high_freq, float alpha, int lpc_order,
                      std::vector<float> &eql, std::vector<float> &idft)
{
    // centres in double, as the float64 restatement states them (np_restatement.mel_tables); the filterbank itself keeps
    // the float32 centres of build_mel_table
    const double pi = 3.14159265358979323846264338;
    const double sr = sample_rate, a1 = 1.0 - (double)alpha;
    const double mlo = 1127.0 * std::log((double)low_freq / 700.0 + 1.0), mhi = 1127.0 * std::log((double)high_freq / 700.0 + 1.0);
    eql.assign((size_t)num_banks, 0.f);
    for (int m = 0; m < num_banks; ++m) {
        const double f = 700.0 * (std::exp(((m + 1) / (double)(num_banks + 1) * (mhi - mlo) + mlo) / 1127.0) - 1.0);
        double o = 2 * pi * f / sr;
        o = o + 2 * std::atan((a1 * std::sin(o)) / (1 - a1 * std::cos(o)));
        const double fc = sr * o / (2 * pi), q = fc * fc;
        const double t = q / (q + 1.6e5);
        eql[m] = (float)(t * t * (q + 1.44e6) / (q + 9.61e6));
    }
    const int N = num_banks + 2;
    idft.assign((size_t)(lpc_order + 1) * N, 0.f);
    for (int i = 0; i <= lpc_order; ++i)
        for (int m = 0; m < N; ++m) {
            const double w = (m == 0 || m == N - 1) ? 1.0 : 2.0;
            idft[(size_t)i * N + m] = (float)(w * std::cos(pi * i * m / (N - 1)) / (2.0 * (N - 1)));
        }
}

void build_traps_basis(int traps_len, int traps_dct_len, std::vector<float> &out)
{
    const double pi = 3.14159265358979323846264338;
    const int L = traps_len, K = traps_dct_len;
    out.assign((size_t)K * L, 0.f);
    const double norm = std::sqrt(2.0 / L);
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < L; ++j) {
            const double w = 0.54 - 0.46 * std::cos(2 * pi * j / (L - 1));
            out[(size_t)k * L + j] = (float)(w * norm * std::cos(pi * k * (j + 0.5) / L));
        }
}

void build_traps_mfma_operands(const std::vector<float> &basis, int traps_len, int traps_dct_len, int &tiles, int &steps,
                               std::vector<float> &out)
{
    const int L = traps_len, K = traps_dct_len;
    tiles = (K + 15) / 16;
    steps = (L + 3) / 4;
    out.assign((size_t)tiles * steps * 64, 0.f);
    for (int t = 0; t < tiles; ++t)
        for (int s = 0; s < steps; ++s)
            for (int lane = 0; lane < 64; ++lane) {
                const int k = 16 * t + (lane & 15), j = 4 * s + (lane >> 4);
                if (k < K && j < L) out[((size_t)t * steps + s) * 64 + lane] = basis[(size_t)k * L + j];
            }
}

void build_traps_valu_operands(const std::vector<float> &basis, int traps_len, int traps_dct_len, int &kp, std::vector<float> &out)
{
    const int L = traps_len, K = traps_dct_len;
    kp = K <= 4 ? 4 : K <= 16 ? 16 : 32;
    out.assign((size_t)L * kp, 0.f);
    for (int j = 0; j < L; ++j)
        for (int k = 0; k < K; ++k) out[(size_t)j * kp + k] = basis[(size_t)k * L + j];
}

void build_xform_operands(const float *A, int out_dim, int in_dim, int &tiles, int &steps, float *out)
{
    tiles = (out_dim + 15) / 16;
    steps = (in_dim + 3) / 4;
    for (int s = 0; s < steps; ++s)
        for (int t = 0; t < tiles; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                const int r = 16 * t + (lane & 15), i = 4 * s + (lane >> 4);
                out[((size_t)s * tiles + t) * 64 + lane] = (r < out_dim && i < in_dim) ? A[(size_t)r * in_dim + i] : 0.f;
            }
}

void build_plp_lifter(int ceps_len, float lift_coef, std::vector<float> &out)
{
    out.assign((size_t)ceps_len, 0.f);
    for (int c = 1; c <= ceps_len; ++c) out[c - 1] = (1 + lift_coef / 2 * sinf(kPiF * (float)c / lift_coef)); // as build_dct_matrix
}

void build_dct_matrix(int num_banks, int ceps_len, bool want_c0, float lift_coef, std::vector<float> &out)
{
    const int dct_len = ceps_len + (want_c0 ? 1 : 0);
    out.assign((size_t)num_banks * dct_len, 0.0f);
    const float norm = (float)std::sqrt(2.0 / num_banks);
    for (int bank = 0; bank < num_banks; ++bank) {
        float *row = out.data() + (size_t)bank * dct_len;
        for (int c = 1; c <= ceps_len; ++c) {
            float lifter = (1 + lift_coef / 2 * sinf(kPiF * (float)c / lift_coef));
            row[c - 1] = lifter * norm * cosf(kPiF * c * (bank + 0.5f) / num_banks);
        }
        if (want_c0) row[ceps_len] = norm;
    }
}

void build_alpha_runs(const float *alphas, const int64_t *frames, int n_utt, std::vector<float> &tables, std::vector<int32_t> &off,
                      std::vector<int64_t> &runs)
{
    tables.clear();
    std::unordered_map<uint32_t, int32_t> table_of; // by bit pattern
    std::vector<int32_t> tab((size_t)std::max(n_utt, 0));
    for (int u = 0; u < n_utt; ++u) {
        uint32_t bits;
        std::memcpy(&bits, &alphas[u], sizeof(bits));
        const auto it = table_of.emplace(bits, (int32_t)tables.size());
        if (it.second) tables.push_back(alphas[u]);
        tab[u] = it.first->second;
    }
    // per table its runs in utterance (= row) order; a run grows while the table's next utterance starts where it ends
    std::vector<std::vector<int64_t>> per(tables.size());
    int64_t row = 0;
    for (int u = 0; u < n_utt; ++u) {
        const int64_t T = frames[u] > 0 ? frames[u] : 0;
        std::vector<int64_t> &r = per[tab[u]];
        if (T > 0) {
            if (!r.empty() && r[r.size() - 2] + r.back() == row) {
                r.back() += T;
            } else {
                r.push_back(row);
                r.push_back(T);
            }
        }
        row += T;
    }
    off.assign(tables.size() + 1, 0);
    runs.clear();
    for (size_t a = 0; a < per.size(); ++a) {
        runs.insert(runs.end(), per[a].begin(), per[a].end());
        off[a + 1] = (int32_t)(runs.size() / 2);
    }
}

bool build_speaker_lists(const int32_t *utt_spk, const int64_t *frames, int n_utt, int n_spk, std::vector<int32_t> &off,
                         std::vector<int32_t> &list)
{
    if (n_spk < 0 || n_utt < 0) return false;
    for (int u = 0; u < n_utt; ++u)
        if (utt_spk[u] < 0 || utt_spk[u] >= n_spk) return false;
    off.assign((size_t)n_spk + 1, 0);
    for (int u = 0; u < n_utt; ++u)
        if (frames[u] > 0) ++off[(size_t)utt_spk[u] + 1];
    for (int s = 0; s < n_spk; ++s) off[(size_t)s + 1] += off[s];
    list.assign((size_t)off[n_spk], 0);
    std::vector<int32_t> next(off.begin(), off.end() - 1);
    for (int u = 0; u < n_utt; ++u) // (ascending u: every speaker's part comes out ascending)
        if (frames[u] > 0) list[(size_t)next[utt_spk[u]]++] = u;
    return true;
}

bool build_utt_tiling(const int64_t *frames, int n_utt, int rows, std::vector<int32_t> &item0, std::vector<int32_t> *item_utt)
{
    if (n_utt < 0 || rows < 1) return false;
    int64_t items = 0;
    for (int u = 0; u < n_utt; ++u) {
        if (frames[u] < 0) return false;
        items += (frames[u] + rows - 1) / rows;
        if (items > 0x7ffffff0) return false;
    }
    item0.assign((size_t)n_utt + 1, 0);
    if (item_utt) item_utt->assign((size_t)items, 0);
    int32_t i = 0;
    for (int u = 0; u < n_utt; ++u) {
        item0[u] = i;
        const int32_t n = (int32_t)((frames[u] + rows - 1) / rows);
        if (item_utt) std::fill_n(item_utt->begin() + i, n, u);
        i += n;
    }
    item0[n_utt] = i;
    return true;
}

void clip_alpha_runs(int64_t row0, int64_t rows, std::vector<int32_t> &off, std::vector<int64_t> &runs)
{
    const int64_t w0 = row0, w1 = row0 + rows;
    std::vector<int64_t> kept;
    int32_t r = 0;
    for (size_t a = 0; a + 1 < off.size(); ++a) {
        const int32_t end = off[a + 1];
        off[a] = (int32_t)(kept.size() / 2);
        for (; r < end; ++r) {
            const int64_t lo = std::max(runs[2 * (size_t)r], w0), hi = std::min(runs[2 * (size_t)r] + runs[2 * (size_t)r + 1], w1);
            if (hi > lo) {
                kept.push_back(lo);
                kept.push_back(hi - lo);
            }
        }
    }
    if (!off.empty()) off.back() = (int32_t)(kept.size() / 2);
    runs.swap(kept);
}

void build_twiddles(int n, int count, std::vector<float> &t)
{
    t.resize((size_t)2 * count);
    for (int k = 0; k < count; ++k) {
        double ang = -2.0 * 3.14159265358979323846264338 * (double)k / (double)n;
        t[2 * k] = (float)std::cos(ang);
        t[2 * k + 1] = (float)std::sin(ang);
    }
}

void build_split_twiddles(int fft_size, bool stuffed, std::vector<float> &split)
{
    const int WS = stuffed ? 512 : fft_size;
    std::vector<float> ws;
    build_twiddles(WS, WS / 2 + 1, ws); // W_{WS}^k
    split.resize(ws.size());
    for (int k = 0; k <= WS / 2; ++k) { // -i * W = (wi, -wr)
        split[2 * k] = ws[2 * k + 1];
        split[2 * k + 1] = -ws[2 * k];
    }
}

void build_reg_pass_twiddles(int fft_size, std::vector<float> &reg)
{
    const int M = fft_size / 2, R1 = fft_size == 1024 ? 8 : 16, n1 = M / R1, n2 = M / (R1 * R1);
    std::vector<float> tw;
    build_twiddles(M, M, tw); // W_M^e
    reg.resize((size_t)2 * (R1 - 1) * (n1 + n2));
    size_t o = 0;
    for (int k = 1; k < R1; ++k)
        for (int pp = 0; pp < n1; ++pp, ++o) {
            const int e = (pp * k) & (M - 1);
            reg[2 * o] = tw[2 * e];
            reg[2 * o + 1] = tw[2 * e + 1];
        }
    for (int k = 1; k < R1; ++k)
        for (int pp = 0; pp < n2; ++pp, ++o) {
            const int e = (pp * k * R1) & (M - 1);
            reg[2 * o] = tw[2 * e];
            reg[2 * o + 1] = tw[2 * e + 1];
        }
}

void build_pass256_twiddles(std::vector<float> &pass)
{
    std::vector<float> full;
    build_twiddles(256, 256, full); // W_256^e
    pass.resize(16 * 16 * 2);
    for (int l = 0; l < 16; ++l)
        for (int k = 0; k < 16; ++k) {
            int e = (l * k) & 255;
            pass[2 * (l * 16 + k)] = full[2 * e];
            pass[2 * (l * 16 + k) + 1] = full[2 * e + 1];
        }
}

void build_window_pairs(const std::vector<float> &padded, int fft_size, bool stuffed, std::vector<float> &wp)
{
    const float fold = 0.5f / (float)fft_size;
    wp.assign(16 * 16 * 2, 0.f);
    for (int l = 0; l < 16; ++l)
        for (int m = 0; m < 16; ++m) {
            int n = l + 16 * m;
            if (stuffed) {
                const int step = 256 / fft_size;
                if (n % step == 0 && n / step < fft_size) wp[2 * (l * 16 + m)] = padded[n / step] * fold;
                continue;
            }
            wp[2 * (l * 16 + m)] = padded[2 * n] * fold;
            wp[2 * (l * 16 + m) + 1] = padded[2 * n + 1] * fold;
        }
}

void build_front1024_phase_o(const std::vector<float> &padded, int fft_size, std::vector<float> &wo)
{
    const float fold = 0.5f / (float)fft_size;
    std::vector<float> tw512;
    build_twiddles(512, 256, tw512);
    wo.assign(16 * 16 * 4, 0.f);
    for (int l = 0; l < 16; ++l)
        for (int m = 0; m < 16; ++m) {
            const int n = l + 16 * m;
            const float t0 = padded[2 * n] * fold, t1 = padded[2 * n + 1] * fold;
            const float c = tw512[2 * n], sn = tw512[2 * n + 1];
            float *q = &wo[4 * (l * 16 + m)];
            q[0] = t0 * c;
            q[1] = -(t1 * sn);
            q[2] = t0 * sn;
            q[3] = t1 * c;
        }
}

void build_front1024_long_window(const std::vector<float> &padded, int fft_size, std::vector<float> &taps, std::vector<float> &tw)
{
    const float fold = 0.5f / (float)fft_size;
    std::vector<float> tw512;
    build_twiddles(512, 256, tw512);
    taps.assign(16 * 32 * 2, 0.f);
    tw.assign(16 * 16 * 2, 0.f);
    for (int l = 0; l < 16; ++l) {
        for (int m = 0; m < 32; ++m) {
            const int n = l + 16 * m;
            taps[2 * (l * 32 + m)] = padded[2 * n] * fold;
            taps[2 * (l * 32 + m) + 1] = padded[2 * n + 1] * fold;
        }
        for (int m = 0; m < 16; ++m) {
            const int n = l + 16 * m;
            tw[2 * (l * 16 + m)] = tw512[2 * n];
            tw[2 * (l * 16 + m) + 1] = tw512[2 * n + 1];
        }
    }
}

// ---- STFT log-mel front end

int64_t stft_frame_count(int64_t samples, int N, int S) { return samples <= N / 2 ? 0 : samples / S; }

int32_t session_stft_step(int N, int S, int64_t &n, int64_t &E, int64_t length, bool final_push, SessionStftStep &st)
{
    const int64_t half = N / 2, n_new = n + length;
    int64_t E_new = stft_frame_count(n_new, N, S);
    if (!final_push && n_new > half) E_new = std::min(E_new, (n_new - half) / S + 1);
    E_new = std::max(E_new, E); // (the rule is non-decreasing in n: a state outside it delivers nothing)
    st.c0_old = std::max<int64_t>(E * S - half, 0);
    st.c0_new = final_push ? n_new : std::max<int64_t>(E_new * S - half, 0);
    st.carry_in = (int32_t)(n - st.c0_old);
    st.carry_out = (int32_t)(n_new - st.c0_new);
    const int32_t n_out = (int32_t)(E_new - E);
    n = final_push ? 0 : n_new;
    E = final_push ? 0 : E_new;
    return n_out;
}

void cut_sess_stft_groups(const int32_t *n_out, int n, std::vector<SessStftCut> &groups)
{
    groups.clear();
    for (int32_t i = 0; i < n; ++i)
        for (int32_t r0 = 0; r0 < n_out[i]; r0 += 16) groups.push_back(SessStftCut{i, r0, std::min(16, n_out[i] - r0)});
}

void build_stft_basis(int N, const float *window, float *cos_sin)
{
    const int K1 = N / 2 + 1;
    const double two_pi = 6.283185307179586476925286766559;
    for (int k = 0; k < K1; ++k)
        for (int j = 0; j < N; ++j) {
            const double a = two_pi * (double)(((int64_t)k * j) % N) / (double)N, w = (double)window[j];
            cos_sin[(size_t)k * N + j] = (float)(w * std::cos(a));
            cos_sin[((size_t)K1 + k) * N + j] = (float)(-w * std::sin(a));
        }
}

namespace {
const double kSlaneyStep = 200.0 / 3.0, kSlaneyLogStep = std::log(6.4) / 27.0;
double slaney_hz_to_mel(double f) { return f < 1000.0 ? f / kSlaneyStep : 15.0 + std::log(f / 1000.0) / kSlaneyLogStep; }
double slaney_mel_to_hz(double m) { return m < 15.0 ? m * kSlaneyStep : 1000.0 * std::exp(kSlaneyLogStep * (m - 15.0)); }
} // namespace

void build_slaney_mel(int M, int N, float sample_rate, float low_freq, float high_freq, float *weights, int32_t *beg, int32_t *len)
{
    const int K1 = N / 2 + 1;
    const double sr = sample_rate, m_lo = slaney_hz_to_mel(low_freq), m_hi = slaney_hz_to_mel(high_freq);
    std::vector<double> p((size_t)M + 2);
    for (int i = 0; i < M + 2; ++i) p[i] = slaney_mel_to_hz(m_lo + (m_hi - m_lo) * (double)i / (double)(M + 1));
    for (int m = 0; m < M; ++m) {
        int first = -1, last = -2;
        for (int k = 0; k < K1; ++k) {
            const double f = (double)k * sr / (double)N;
            const double up = (f - p[m]) / (p[m + 1] - p[m]), down = (p[m + 2] - f) / (p[m + 2] - p[m + 1]);
            const float w = (float)(std::max(0.0, std::min(up, down)) * 2.0 / (p[m + 2] - p[m]));
            weights[(size_t)m * K1 + k] = w;
            if (w != 0.f) {
                if (first < 0) first = k;
                last = k;
            }
        }
        beg[m] = first < 0 ? 0 : first;
        len[m] = first < 0 ? 0 : last - first + 1;
    }
}

void build_stft_operands(const float *cos_sin, int N, int tb, std::vector<float> &out)
{
    const int K1 = N / 2 + 1, nbt = (K1 + 15) / 16, steps = (N + 3) / 4, passes = (nbt + tb - 1) / tb;
    out.assign((size_t)passes * steps * 2 * tb * 64, 0.f);
    for (int ps = 0; ps < passes; ++ps)
        for (int s = 0; s < steps; ++s)
            for (int tile = 0; tile < 2 * tb; ++tile)
                for (int lane = 0; lane < 64; ++lane) {
                    const int k = 16 * (ps * tb + tile / 2) + (lane & 15), j = 4 * s + (lane >> 4);
                    if (k < K1 && j < N)
                        out[(((size_t)ps * steps + s) * 2 * tb + tile) * 64 + lane] = cos_sin[((size_t)(tile & 1) * K1 + k) * N + j];
                }
}

void build_stft_fft_tables(int N, float *twid, float *split)
{
    std::vector<float> t;
    build_twiddles(N / 2, N / 2, t); // W_M^k, k < M
    std::copy(t.begin(), t.end(), twid);
    build_split_twiddles(N, false, t); // -i W_N^k, k <= M
    std::copy(t.begin(), t.end(), split);
}

void build_fft_operands(int W, int N, int n_split, const float *window, std::vector<float> &out)
{
    out.assign((size_t)2 * N + 2 * (size_t)n_split, 0.f);
    std::copy(window, window + W, out.begin());
    std::vector<float> split((size_t)N + 2);
    build_stft_fft_tables(N, out.data() + N, split.data());
    std::copy(split.begin(), split.begin() + 2 * (size_t)n_split, out.begin() + 2 * N);
}

void build_stft_fft_operands(int N, const float *window, std::vector<float> &out) { build_fft_operands(N, N, N / 2 + 1, window, out); }

void build_stft_form_operands(StftForm form, int N, const float *window, std::vector<float> &out)
{
    if (form == StftForm::Fft) return build_stft_fft_operands(N, window, out);
    std::vector<float> basis((size_t)2 * (N / 2 + 1) * N);
    build_stft_basis(N, window, basis.data());
    build_stft_operands(basis.data(), N, stft_pass_tiles(N), out);
}

void pack_mel_spans(const float *dense, int M, int row_width, std::vector<float> &w, std::vector<int32_t> &meta)
{
    w.clear();
    for (int m = 0; m < M; ++m) {
        const float *span = dense + (size_t)m * row_width + meta[m];
        meta[(size_t)2 * M + m] = (int32_t)w.size();
        w.insert(w.end(), span, span + meta[(size_t)M + m]);
    }
    if (w.empty()) w.push_back(0.f); // (every band empty or narrower than a bin: keep the buffer non-null)
}

void build_slaney_spans(int M, int N, float sample_rate, float low_freq, float high_freq, std::vector<float> &w, std::vector<int32_t> &meta)
{
    const int K1 = N / 2 + 1;
    std::vector<float> dense((size_t)M * K1);
    meta.assign((size_t)3 * M, 0);
    build_slaney_mel(M, N, sample_rate, low_freq, high_freq, dense.data(), meta.data(), meta.data() + M);
    pack_mel_spans(dense.data(), M, K1, w, meta);
}

bool kaldi_freqs_ok(float sample_rate, float low_freq, float high_freq, double *high_abs)
{
    const double nyq = (double)sample_rate / 2.0, hi = high_freq > 0.f ? (double)high_freq : nyq + (double)high_freq;
    if (high_abs) *high_abs = hi;
    return low_freq >= 0.f && (double)low_freq < hi && hi <= nyq; // (false for NaN)
}

int64_t kaldi_frame_count(int64_t samples, int W, int S, int flags)
{
    if (!(flags & kKaldiNoSnipEdges)) return frame_count(samples, W, S);
    return samples <= 0 ? 0 : (samples + S / 2) / S;
}

void kaldi_frame_samples(int64_t samples, int W, int S, int flags, int64_t t, int64_t *idx)
{
    const bool centred = (flags & kKaldiNoSnipEdges) != 0;
    const int64_t s0 = centred ? kaldi_centred_start(t, W, S) : t * S;
    for (int i = 0; i < W; ++i) idx[i] = centred ? kaldi_reflect(s0 + i, samples) : s0 + i;
}

void build_kaldi_mel(int M, int N, float sample_rate, float low_freq, double high_abs, float *weights, int32_t *beg, int32_t *len)
{
    const int K = N / 2;
    auto mel = [](double f) { return 1127.0 * std::log(1.0 + f / 700.0); };
    const double ml = mel((double)low_freq), mh = mel(high_abs), delta = (mh - ml) / (double)(M + 1);
    for (int m = 0; m < M; ++m) {
        const double l = ml + (double)m * delta, c = l + delta, r = l + 2.0 * delta;
        int first = -1, last = -2;
        for (int k = 0; k < K; ++k) {
            const double mk = mel((double)k * (double)sample_rate / (double)N);
            float w = 0.f;
            if (mk > l && mk < r) w = (float)(mk <= c ? (mk - l) / (c - l) : (r - mk) / (r - c));
            weights[(size_t)m * K + k] = w;
            if (w != 0.f) {
                if (first < 0) first = k;
                last = k;
            }
        }
        beg[m] = first < 0 ? 0 : first;
        len[m] = first < 0 ? 0 : last - first + 1;
    }
}

void build_kaldi_spans(int M, int N, float sample_rate, float low_freq, double high_abs, std::vector<float> &w, std::vector<int32_t> &meta)
{
    const int K = N / 2;
    std::vector<float> dense((size_t)M * K);
    meta.assign((size_t)3 * M, 0);
    build_kaldi_mel(M, N, sample_rate, low_freq, high_abs, dense.data(), meta.data(), meta.data() + M);
    pack_mel_spans(dense.data(), M, K, w, meta);
}

void build_kaldi_dct(int M, int C, float lifter, float *G)
{
    const double pi = 3.14159265358979323846264338, Q = (double)lifter;
    for (int i = 0; i < C; ++i) {
        const double l = Q > 0.0 ? 1.0 + Q / 2.0 * std::sin(pi * (double)i / Q) : 1.0;
        for (int m = 0; m < M; ++m) {
            const double D = i == 0 ? std::sqrt(1.0 / (double)M) : std::sqrt(2.0 / (double)M) * std::cos(pi / (double)M * ((double)m + 0.5) * (double)i);
            G[(size_t)i * M + m] = (float)(l * D);
        }
    }
}

// (the kernel splits bins k < M)
void build_kaldi_operands(int W, int N, const float *window, std::vector<float> &out) { build_fft_operands(W, N, N / 2, window, out); }

} // namespace mfx

namespace mfx {

// Start bins for the filters of one round: cands[j] lists lane j's admissible starts (its own first, then earlier ones);
// a start occupies residue (start / align) mod residues.  Returns one start per lane such that as many lanes as possible
// hold a residue of their own (maximum bipartite matching, augmenting paths; lanes left over keep their own start).
static std::vector<int> match_starts(const std::vector<std::vector<int>> &cands, int align, int residues)
{
    const int n = (int)cands.size();
    std::vector<int> owner(residues, -1), choice(n, -1);
    std::vector<char> seen;
    auto res = [&](int start) { return (start / align) % residues; };
    std::function<bool(int)> augment = [&](int j) {
        for (size_t c = 0; c < cands[j].size(); ++c) {
            const int q = res(cands[j][c]);
            if (seen[q]) continue;
            seen[q] = 1;
            if (owner[q] < 0 || augment(owner[q])) {
                owner[q] = j;
                choice[j] = (int)c;
                return true;
            }
        }
        return false;
    };
    for (int j = 0; j < n; ++j) {
        if (cands[j].empty()) continue;
        seen.assign(residues, 0);
        augment(j);
    }
    std::vector<int> pick(n, 0);
    for (int j = 0; j < n; ++j)
        if (!cands[j].empty()) pick[j] = cands[j][choice[j] < 0 ? 0 : choice[j]];
    return pick;
}

static int stride_4odd(int n)
{
    int q = (n + 3) / 4;
    if ((q & 1) == 0) ++q;
    return 4 * q;
}

bool build_mel_plan(const MelTable &t, int num_banks, int fft_size, int max_read_bin, int lanes, int align, MelPlan &out)
{
    if (lanes != 16 && lanes != 32 && lanes != 64) return false;
    std::vector<int> order(num_banks);
    for (int m = 0; m < num_banks; ++m) order[m] = m;
    auto span = [&](int m) { return t.beg[m + 2] - t.beg[m]; };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return span(a) > span(b); });
    out.lanes = lanes;
    out.rounds = (num_banks + lanes - 1) / lanes;
    if (out.rounds > 8) return false;
    out.start.assign((size_t)lanes * out.rounds, 0);
    out.fid.assign((size_t)lanes * out.rounds, -1);
    const int group = std::min(lanes, 32);
    int total = 0;
    for (int r = 0; r < out.rounds; ++r) {
        // Starts are multiples of `align` bins (an 8- or 16-byte LDS read).  A read is served in groups of `group` lanes
        // (the 16 lanes of a frame; 32 lanes of a wider plan's 8-byte read over 32 bank pairs): a group is conflict free
        // when (start / align) mod group differs from lane to lane, so a clashing filter may begin a few reads early (zero
        // weights: the sum keeps its bits) -- as long as the round does not get longer for it (a two-way bank conflict
        // costs one LDS cycle per read, a longer round a whole 8-bin trip on every lane).  Which filter moves where is a
        // maximum bipartite matching of a group's filters to residues.
        int natural = 8;
        for (int j = 0; j < lanes; ++j) {
            const int idx = r * lanes + j;
            if (idx >= num_banks) continue;
            const int m = order[idx];
            natural = std::max(natural, (t.beg[m + 2] - (t.beg[m] & ~(align - 1)) + 7) & ~7);
        }
        int longest = 0;
        for (int g0 = 0; g0 < lanes; g0 += group) {
            std::vector<std::vector<int>> cands(group);
            for (int j = g0; j < g0 + group; ++j) {
                const int idx = r * lanes + j;
                if (idx >= num_banks) continue;
                const int m = order[idx];
                for (int d = 0; d < group; ++d) {
                    const int cand = (t.beg[m] & ~(align - 1)) - align * d;
                    if (cand < 0 || t.beg[m + 2] - cand > natural) break;
                    cands[j - g0].push_back(cand);
                }
            }
            const std::vector<int> pick = match_starts(cands, align, group);
            for (int j = g0; j < g0 + group; ++j) {
                const int idx = r * lanes + j;
                if (idx >= num_banks) continue;
                const int m = order[idx];
                out.start[r * lanes + j] = pick[j - g0];
                out.fid[r * lanes + j] = m;
                longest = std::max(longest, t.beg[m + 2] - pick[j - g0]);
            }
        }
        out.L[r] = std::max(8, (longest + 7) & ~7);
        total += out.L[r];
    }
    out.row_stride = stride_4odd(total);
    out.w.assign((size_t)lanes * out.row_stride, 0.0f);
    int base = 0;
    for (int r = 0; r < out.rounds; ++r) {
        for (int j = 0; j < lanes; ++j) {
            const int m = out.fid[r * lanes + j];
            if (m < 0) continue;
            const int start = out.start[r * lanes + j];
            if (start + out.L[r] - 1 > max_read_bin) return false;
            const float *row = t.weights.data() + (size_t)(m & 1) * fft_size;
            float *dst = out.w.data() + (size_t)j * out.row_stride + base;
            for (int k = t.beg[m]; k < t.beg[m + 2]; ++k) dst[k - start] = row[k];
        }
        base += out.L[r];
    }
    return true;
}

void build_dct_mfma_operands(const std::vector<float> &dct, int num_banks, int dct_len, int &tiles, int &ksteps,
                             std::vector<float> &out)
{
    tiles = (dct_len + 15) / 16;
    ksteps = (num_banks + 3) / 4;
    out.assign((size_t)tiles * ksteps * 64, 0.0f);
    for (int tl = 0; tl < tiles; ++tl)
        for (int j = 0; j < ksteps; ++j)
            for (int lane = 0; lane < 64; ++lane) {
                const int m = 4 * j + (lane >> 4), c = 16 * tl + (lane & 15);
                if (m < num_banks && c < dct_len) out[((size_t)tl * ksteps + j) * 64 + lane] = dct[(size_t)m * dct_len + c];
            }
}

void build_dct_mfma_operands4(const std::vector<float> &dct, int num_banks, int dct_len, std::vector<float> &out)
{
    const int tiles = (dct_len + 63) / 64, ks = (num_banks + 3) / 4;
    out.assign((size_t)tiles * ks * 64 * 4, 0.0f);
    for (int tl = 0; tl < tiles; ++tl)
        for (int j4 = 0; j4 < ks; ++j4)
            for (int lane = 0; lane < 64; ++lane)
                for (int u = 0; u < 4; ++u) {
                    const int m = 4 * j4 + u, c = 64 * tl + lane;
                    if (m < num_banks && c < dct_len) out[(((size_t)tl * ks + j4) * 64 + lane) * 4 + u] = dct[(size_t)m * dct_len + c];
                }
}

int dct_split_mode(int num_banks, int dct_len)
{
    if (num_banks % 32 != 0 || num_banks > 256 || dct_len < 1) return 0;
    return dct_len <= 32 ? 1 : dct_len <= 40 ? 2 : 0;
}

void build_dct_mfma_operands4_split(const std::vector<float> &dct, int num_banks, int dct_len, std::vector<float> &out)
{
    const int mode = dct_split_mode(num_banks, dct_len);
    out.clear();
    if (mode == 0) return;
    const int H = num_banks / 2, E = num_banks / 8, ga = H / 4, gb = mode == 2 ? E / 4 : 0;
    out.assign((size_t)(ga + gb) * 64 * 4, 0.0f);
    for (int g = 0; g < ga; ++g)
        for (int lane = 0; lane < 64; ++lane)
            for (int u = 0; u < 4; ++u) {
                const int m = (lane >> 5) * H + 4 * g + u, c = lane & 31;
                if (c < dct_len) out[((size_t)g * 64 + lane) * 4 + u] = dct[(size_t)m * dct_len + c];
            }
    for (int g = 0; g < gb; ++g)
        for (int lane = 0; lane < 64; ++lane)
            for (int u = 0; u < 4; ++u) {
                const int m = (lane >> 3) * E + 4 * g + u, c = 32 + (lane & 7);
                if (c < dct_len) out[((size_t)(ga + g) * 64 + lane) * 4 + u] = dct[(size_t)m * dct_len + c];
            }
}

void build_dct_transposed(const std::vector<float> &dct, int num_banks, int dct_len, int &stride, int &nb_pad,
                          std::vector<float> &out)
{
    nb_pad = (num_banks + 3) & ~3;
    stride = stride_4odd(nb_pad);
    out.assign((size_t)dct_len * stride, 0.0f);
    for (int m = 0; m < num_banks; ++m)
        for (int c = 0; c < dct_len; ++c) out[(size_t)c * stride + m] = dct[(size_t)m * dct_len + c];
}

// ------------------------------------------------------------------------------------------------
// sample-rate conversion
// ------------------------------------------------------------------------------------------------

static int64_t gcd64(int64_t a, int64_t b)
{
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

int resample_shape(int32_t in_hz, int32_t out_hz, int32_t zeros, float rolloff, ResampleShape &s)
{
    if (in_hz < 1000 || in_hz > 768000 || out_hz < 1000 || out_hz > 768000) return -1;
    if (zeros == 0) zeros = 6;
    if (zeros < 1 || zeros > 64) return -2;
    const double ro = rolloff == 0.f ? 0.99 : (double)rolloff;
    if (!(ro > 0.0 && ro <= 1.0)) return -3;
    const int64_t g = gcd64(in_hz, out_hz);
    const int64_t L = out_hz / g, M = in_hz / g;
    if (L > 4096) return -4;
    const double c = ro * std::min(1.0, (double)L / (double)M);
    const double wh = std::ceil((double)zeros / c);
    if (2.0 * wh > 4096.0) return -5;
    const int64_t P = 2 * (int64_t)wh;
    if (L * P > ((int64_t)1 << 20)) return -6;
    s.L = (int32_t)L, s.M = (int32_t)M, s.P = (int32_t)P, s.Wh = (int32_t)wh, s.c = c;
    return 0;
}

void build_resample_taps(const ResampleShape &s, float *taps)
{
    const double pi = 3.14159265358979323846;
    for (int phi = 0; phi < s.L; ++phi)
        for (int k = 0; k < s.P; ++k) {
            const double t = (double)(k - s.Wh + 1) - (double)phi / (double)s.L;
            double h = 0.0;
            if (std::fabs(t) < (double)s.Wh) {
                const double x = s.c * t;
                const double sinc = x == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x);
                h = s.c * sinc * 0.5 * (1.0 + std::cos(pi * t / (double)s.Wh));
            }
            taps[(size_t)phi * s.P + k] = (float)h;
        }
}

int64_t resampled_length(int64_t samples, int32_t in_hz, int32_t out_hz)
{
    if (samples <= 0) return 0;
    const int64_t g = gcd64(in_hz, out_hz);
    const int64_t L = out_hz / g, M = in_hz / g;
    return (samples * L + M - 1) / M;
}

int64_t resample_layout(int32_t n_utt, const int64_t *lengths, const int32_t *rates_hz, int32_t out_hz, int64_t *offsets,
                        int64_t *out_lengths)
{
    int64_t off = 0;
    for (int u = 0; u < n_utt; ++u) {
        if (lengths[u] < 0 || rates_hz[u] < 1000 || rates_hz[u] > 768000) return -1;
        const int64_t n = resampled_length(lengths[u], rates_hz[u], out_hz);
        if (offsets) offsets[u] = off;
        if (out_lengths) out_lengths[u] = n;
        off += (n + 1) & ~(int64_t)1;
    }
    return off;
}

// outputs whose input span fits `budget` floats per channel
static int64_t fit_outputs(const ResRate &r, int64_t budget)
{
    const int64_t s = budget - r.P - 32;
    return s <= 0 ? 0 : s * r.L / r.M;
}

// Target: 2048 outputs per tile with the input span inside 32 KB of LDS (all channels); a ratio or a filter too long for that
// takes up to 64 KB, and fewer outputs (the limits of resample_shape leave at least 4).  R same-phase outputs per work item: 4
// where four periods of L fit the tile, else 2, else 1 (every phase then occurs at most once in a tile: nothing to share).  The
// table goes to LDS when its padded form is at most 64 KB.
void resample_geometry(int channels, ResRate &r)
{
    const int ch = channels == 2 ? 2 : 1;
    int64_t to = std::min<int64_t>(2048, fit_outputs(r, 8192 / ch));
    if (to < 64) to = std::min<int64_t>(2048, fit_outputs(r, 16384 / ch));
    to = std::max<int64_t>(to & ~(int64_t)1, 2);
    if (2 * (int64_t)r.L > to) {
        r.R = 1;
        r.items = (int32_t)to;
    } else {
        r.R = 4 * (int64_t)r.L <= to ? 4 : 2;
        r.items = r.L * (int32_t)(to / ((int64_t)r.R * r.L));
    }
    r.tile_out = r.R * r.items;
    r.in_lds = (int64_t)r.L * (r.P + 1) <= 16384 ? 1 : 0;
}

// (tile_out - 1) M / L + 1 input positions + P - 1 of halo + 1 for the parity step of a mono source, rounded up to whole groups
// of 8
int resample_span_floats(const ResRate &r)
{
    const int64_t span = ((int64_t)(r.tile_out - 1) * r.M) / r.L + r.P + 3;
    return (int)(((span + 7) & ~(int64_t)7) + 8);
}

const char *const kResampleWhy[7] = {"", "sample rates must lie in 1000 .. 768000 Hz", "zeros must be 1 .. 64 (0 = 6)",
                                     "rolloff must lie in (0, 1] (0 = 0.99)", "L = out_hz / gcd is larger than 4096",
                                     "the filter has more than 4096 taps per phase", "the tap table L x P is larger than 2^20 floats"};

int build_resample_rates(int channels, int32_t out_hz, const int32_t *in_hz, int n_rates, int32_t zeros, float rolloff, bool check_same_rate,
                         ResRateSet &set)
{
    set.rates.assign((size_t)n_rates, ResRate{});
    set.taps.clear();
    set.lds = ResLds{0, 8, 2};
    set.carry_cap = 8, set.tile_min = kResCopyTile;
    for (int k = 0; k < n_rates; ++k) {
        ResRate &r = set.rates[k];
        const bool same = in_hz[k] == out_hz;
        if (same && !check_same_rate) continue;
        ResampleShape sh;
        if (const int e = resample_shape(in_hz[k], out_hz, zeros, rolloff, sh); e != 0) return -e;
        if (same) continue;
        r.taps_off = (int64_t)set.taps.size();
        r.L = sh.L, r.M = sh.M, r.P = sh.P, r.Wh = sh.Wh;
        set.taps.resize(set.taps.size() + (size_t)sh.L * sh.P);
        build_resample_taps(sh, set.taps.data() + r.taps_off);
        resample_geometry(channels, r);
        if (r.in_lds) set.lds.taps_floats = std::max(set.lds.taps_floats, (r.L * (r.P + 1) + 3) & ~3);
        set.lds.x_floats = std::max(set.lds.x_floats, resample_span_floats(r));
        set.lds.out_elems = std::max(set.lds.out_elems, r.tile_out * channels);
        set.carry_cap = std::max(set.carry_cap, (2 * r.Wh + r.M / r.L + 2 + 7) & ~7);
        set.tile_min = std::min(set.tile_min, r.tile_out);
    }
    if (set.taps.empty()) set.taps.assign(4, 0.f);
    return 0;
}

int64_t session_resample_step(int32_t L, int32_t M, int32_t Wh, int64_t &N, int64_t &J, int64_t length, bool final_push,
                              SessionResampleStep &st)
{
    const bool pass = L == M;
    // (the first input sample output j reads; nothing before the stream's start is kept)
    auto first_needed = [&](int64_t j) { return std::max<int64_t>((j * M) / L - Wh + 1, 0); };
    const int64_t N_old = N, J_old = J, N_new = N + length;
    int64_t J_new;
    if (pass)
        J_new = N_new;
    else if (final_push)
        J_new = (N_new * L + M - 1) / M;
    else
        J_new = N_new > Wh ? ((N_new - Wh) * L + M - 1) / M : 0;
    st.c0_old = pass ? N_old : std::min(first_needed(J_old), N_old);
    st.c0_new = pass || final_push ? N_new : std::min(first_needed(J_new), N_new);
    st.carry_in = (int32_t)(N_old - st.c0_old), st.carry_out = (int32_t)(N_new - st.c0_new);
    N = final_push ? 0 : N_new, J = final_push ? 0 : J_new;
    return J_new - J_old;
}

// The online normaliser's definition (include/mfx.h, mfx_batch_set_online_norm) on host memory: per column the chunked
// prefix sums P of v and of q, then every row's window, prior, statistics and float32 apply.  Every double operation is
// a statement of its own and this file is compiled with -ffp-contract=off.
bool host_online_norm(const float *rows, int64_t T, int pitch, int Wn, int kind, int window, int prior_frames, int64_t prior_count,
                      const double *prior_acc, float *out)
{
    if (T < 0 || Wn < 1 || Wn > 256 || pitch < Wn || (kind != 1 && kind != 2)) return false;
    if (window < 0 || window > 4096 || window % 32 != 0 || prior_frames < 0 || prior_frames > (1 << 20) || prior_count < 0) return false;
    if ((prior_acc == nullptr) != (prior_count == 0) || (T > 0 && (!rows || !out))) return false;
    std::vector<double> Pv((size_t)T), Pq((size_t)T);
    for (int j = 0; j < Wn; ++j) {
        double Ov = 0.0, Oq = 0.0, Iv = 0.0, Iq = 0.0;
        for (int64_t t = 0; t < T; ++t) {
            const float v = rows[t * pitch + j];
            const float q = v * v;
            Iv = Iv + (double)v;
            Iq = Iq + (double)q;
            Pv[(size_t)t] = Ov + Iv;
            Pq[(size_t)t] = Oq + Iq;
            if (t % 32 == 31) { // the chunk's last row: Tot = I
                Ov = Ov + Iv;
                Oq = Oq + Iq;
                Iv = 0.0, Iq = 0.0;
            }
        }
        for (int64_t t = 0; t < T; ++t) {
            const float v = rows[t * pitch + j];
            double Sw = Pv[(size_t)t], Qw = Pq[(size_t)t];
            int64_t n = t + 1;
            if (window > 0 && t >= window) {
                Sw = Sw - Pv[(size_t)(t - window)];
                Qw = Qw - Pq[(size_t)(t - window)];
                n = window;
            }
            int64_t k = 0;
            if (prior_count > 0 && (int64_t)prior_frames > n) k = std::min<int64_t>(prior_count, (int64_t)prior_frames - n);
            if (k > 0) {
                const double r = (double)k / (double)prior_count;
                const double a = prior_acc[j] * r, b = prior_acc[Wn + j] * r;
                Sw = Sw + a;
                Qw = Qw + b;
            }
            const double nn = (double)(n + k);
            const double m = Sw / nn;
            const float mean = (float)m;
            float y = v - mean;
            if (kind == 2) {
                const double sm = Sw * m;
                const double d = Qw - sm;
                float mult = 1.0f;
                if (nn >= 2.0 && d > 0.0) {
                    const double ratio = (nn - 1.0) / d;
                    mult = (float)std::sqrt(ratio);
                }
                y = y * mult;
            }
            out[t * Wn + j] = y;
        }
    }
    return true;
}

// The sliding-window normaliser's definition (include/mfx.h, mfx_batch_set_sliding_norm) on host memory: per column the
// online normaliser's chunked prefix sums P of v and of q, then every row's window (slide_window), statistics and float32
// apply.  Every double operation is a statement of its own and this file is compiled with -ffp-contract=off.
bool host_sliding_norm(const float *rows, int64_t T, int W, int pitch, int window, int min_window, int center, int norm_vars, float *out,
                       int out_pitch)
{
    if (T < 0 || W < 1 || W > 256 || pitch < W || out_pitch < W) return false;
    if (window < 1 || window > 4096 || min_window < 0 || min_window > window) return false;
    if ((center != 0 && center != 1) || (norm_vars != 0 && norm_vars != 1) || (T > 0 && (!rows || !out))) return false;
    std::vector<double> Pv((size_t)T), Pq((size_t)T);
    for (int j = 0; j < W; ++j) {
        double Ov = 0.0, Oq = 0.0, Iv = 0.0, Iq = 0.0;
        for (int64_t t = 0; t < T; ++t) {
            const float v = rows[t * pitch + j];
            const float q = v * v;
            Iv = Iv + (double)v;
            Iq = Iq + (double)q;
            Pv[(size_t)t] = Ov + Iv;
            Pq[(size_t)t] = Oq + Iq;
            if (t % 32 == 31) { // the chunk's last row: Tot = I
                Ov = Ov + Iv;
                Oq = Oq + Iq;
                Iv = 0.0, Iq = 0.0;
            }
        }
        for (int64_t t = 0; t < T; ++t) {
            int64_t ws, we;
            slide_window(T, window, min_window, center != 0, t, ws, we);
            const double Sw = Pv[(size_t)(we - 1)] - (ws > 0 ? Pv[(size_t)(ws - 1)] : 0.0);
            const double Qw = Pq[(size_t)(we - 1)] - (ws > 0 ? Pq[(size_t)(ws - 1)] : 0.0);
            const int64_t n = we - ws;
            const float v = rows[t * pitch + j];
            const double nn = (double)n;
            const double m = Sw / nn;
            const float mean = (float)m;
            float y = v - mean;
            if (norm_vars) {
                if (n == 1) {
                    y = 0.0f;
                } else {
                    const double e2 = Qw / nn;
                    const double mm = m * m;
                    double var = e2 - mm;
                    if (var < 1e-10) var = 1e-10;
                    const double sd = std::sqrt(var);
                    const double inv = 1.0 / sd;
                    y = y * (float)inv;
                }
            }
            out[t * out_pitch + j] = y;
        }
    }
    return true;
}

// ---- pitch track (include/mfx.h, mfx_batch_set_pitch)

bool pitch_shape(int window, int lag_min, int lag_max, float ballast, float lag_cost, float penalty, int max_jump, PitchShape &s)
{
    if (window < 32 || window > 1024 || lag_min < 2 || lag_max > 1024) return false;
    const int64_t K = (int64_t)lag_max - lag_min + 1;
    if (K < 1 || K > 512) return false;
    if (!std::isfinite(ballast) || !std::isfinite(lag_cost) || !std::isfinite(penalty)) return false;
    if (ballast < 0.f || lag_cost < 0.f || lag_cost > 1.f || penalty < 0.f) return false;
    if (max_jump < 0 || max_jump > 511) return false;
    const int top = std::max((int)K - 1, 1);
    s.window = window, s.lag_min = lag_min, s.lag_max = lag_max, s.K = (int)K;
    s.J = max_jump == 0 ? top : std::min(max_jump, top);
    return true;
}

void build_pitch_tables(const PitchShape &s, float lag_cost, std::vector<float> &wt, std::vector<float> &lg)
{
    wt.assign((size_t)s.K, 0.f), lg.assign((size_t)s.K, 0.f);
    for (int k = 0; k < s.K; ++k) {
        const double l = (double)(s.lag_min + k);
        wt[(size_t)k] = (float)(1.0 - (double)lag_cost * l / (double)s.lag_max);
        lg[(size_t)k] = (float)std::log(l);
    }
}

int pitch_span_pad(int shift) { return shift >= 64 ? (2 - shift) & 63 : 0; }

int pitch_span_slots(int window, int lag_max, int shift, int frames)
{
    const int64_t last = (int64_t)(frames - 1) * shift + window + lag_max - 1; // the span's last sample
    const int64_t slots = last + (int64_t)pitch_span_pad(shift) * (last / shift) + 1;
    return slots > 0x7fffffff ? 0x7fffffff : (int)slots;
}

int pitch_tile_frames(int window, int lag_max, int shift)
{
    int f = 64;
    while (f > 1 && pitch_span_slots(window, lag_max, shift, f) > kPitchSpanMax) --f;
    return f;
}

// Every float32 and double operation below is a statement of its own and this file is compiled with -ffp-contract=off; the
// correlation is one std::fmaf chain per value.
bool host_pitch(const int16_t *pcm, int64_t n, int channels, int64_t T, int shift, int window, int lag_min, int lag_max, float ballast,
                float lag_cost, float penalty, int max_jump, float *pitch, int32_t *index, float *nccf)
{
    PitchShape s;
    if (!pitch_shape(window, lag_min, lag_max, ballast, lag_cost, penalty, max_jump, s)) return false;
    if (n < 0 || T < 0 || T > 0x7fffffff || shift < 1 || (channels != 1 && channels != 2) || (n > 0 && !pcm)) return false;
    if (T == 0) return true;
    const int W = s.window, K = s.K, J = s.J, Ls = W + s.lag_max;
    std::vector<float> wt, lg;
    build_pitch_tables(s, lag_cost, wt, lg);
    std::vector<float> own;
    if (!nccf) {
        own.resize((size_t)T * K);
        nccf = own.data();
    }
    // ---- the NCCF rows
    const float c1 = (float)(1.0 / (32768.0 * (double)Ls));
    std::vector<int32_t> p((size_t)Ls);
    std::vector<float> z((size_t)Ls);
    std::vector<double> P((size_t)Ls + 1);
    for (int64_t t = 0; t < T; ++t) {
        const int64_t i0 = t * shift;
        int64_t sI = 0;
        for (int j = 0; j < Ls; ++j) {
            const int64_t i = i0 + j;
            int32_t v = 0;
            if (i < n) v = channels == 2 ? ((int32_t)pcm[2 * i] + (int32_t)pcm[2 * i + 1]) >> 1 : (int32_t)pcm[i];
            p[(size_t)j] = v;
            sI += v;
        }
        const float m = (float)sI * c1;
        P[0] = 0.0;
        for (int j = 0; j < Ls; ++j) {
            const float x = (float)p[(size_t)j] * 0x1p-15f;
            const float zj = x - m;
            const float q = zj * zj;
            z[(size_t)j] = zj;
            P[(size_t)j + 1] = P[(size_t)j] + (double)q;
        }
        const float e0 = (float)(P[(size_t)W] - P[0]);
        float *rho = nccf + (size_t)t * K;
        for (int k = 0; k < K; ++k) {
            const int l = s.lag_min + k;
            float c = 0.f;
            for (int j = 0; j < W; ++j) c = std::fmaf(z[(size_t)j], z[(size_t)(j + l)], c);
            const float el = (float)(P[(size_t)(l + W)] - P[(size_t)l]);
            const float prod = e0 * el;
            const float sden = prod + ballast;
            float r = 0.f;
            if (sden > 0.f) {
                const float root = std::sqrt(sden);
                r = c / root;
            }
            rho[k] = r;
        }
    }
    // ---- the track
    std::vector<uint16_t> bp((size_t)T * K);
    std::vector<float> fwd((size_t)K), a((size_t)K);
    for (int64_t t = 0; t < T; ++t) {
        const float *rho = nccf + (size_t)t * K;
        for (int k = 0; k < K; ++k) {
            const float rw = rho[k] * wt[(size_t)k];
            const float loc = 1.0f - rw;
            if (t == 0) {
                a[(size_t)k] = loc;
                continue;
            }
            const int lo = std::max(0, k - J), hi = std::min(K - 1, k + J);
            float best = 0.f;
            int bk = -1;
            for (int kk = lo; kk <= hi; ++kk) {
                const float d = lg[(size_t)k] - lg[(size_t)kk];
                const float pd = penalty * d;
                const float tr = pd * d;
                const float cand = fwd[(size_t)kk] + tr;
                if (bk < 0 || cand < best) best = cand, bk = kk;
            }
            a[(size_t)k] = loc + best;
            bp[(size_t)t * K + k] = (uint16_t)bk;
        }
        int km = 0;
        for (int k = 1; k < K; ++k)
            if (a[(size_t)k] < a[(size_t)km]) km = k;
        const float mt = a[(size_t)km];
        for (int k = 0; k < K; ++k) fwd[(size_t)k] = a[(size_t)k] - mt;
    }
    int k = 0;
    for (int kk = 1; kk < K; ++kk)
        if (fwd[(size_t)kk] < fwd[(size_t)k]) k = kk;
    for (int64_t t = T - 1; t >= 0; --t) {
        const float *rho = nccf + (size_t)t * K;
        float delta = 0.f;
        if (k > 0 && k < K - 1) {
            const float ra = rho[k - 1], rb = rho[k], rc = rho[k + 1];
            const float d1 = ra - rb, d2 = rc - rb;
            const float den = d1 + d2;
            if (den < 0.f) {
                const float num = ra - rc;
                const float half = 0.5f * num;
                delta = half / den;
                delta = delta < -0.5f ? -0.5f : delta > 0.5f ? 0.5f : delta;
            }
        }
        if (index) index[t] = k;
        if (pitch) {
            pitch[2 * t] = (float)(s.lag_min + k) + delta;
            pitch[2 * t + 1] = rho[k];
        }
        if (t > 0) k = bp[(size_t)t * K + k];
    }
    return true;
}

// ---- pitch features (include/mfx.h, mfx_batch_set_pitch_feats)

bool pitch_feat_shape(int columns, int left, int right, int delta_window, float pov_scale, float pov_offset, float pitch_scale,
                      float delta_scale, PitchFeatShape &s)
{
    if (columns < 0 || columns > 15) return false;
    if (left < 0 || left > 1024 || right < 0 || right > 1024 || delta_window < 1 || delta_window > 16) return false;
    if (!std::isfinite(pov_scale) || !std::isfinite(pov_offset) || !std::isfinite(pitch_scale) || !std::isfinite(delta_scale)) return false;
    s.columns = columns == 0 ? 7 : columns;
    s.F = 0;
    for (int b = 1; b <= 8; b <<= 1) s.F += (s.columns & b) ? 1 : 0;
    s.left = left, s.right = right, s.D = delta_window;
    int den = 0;
    for (int l = 1; l <= delta_window; ++l) den += 2 * l * l;
    s.den = (double)den;
    return true;
}

// Every double operation below is a statement of its own and this file is compiled with -ffp-contract=off: k_pitch_feats
// (mfx_pitchfeat.hip) spells the same operations in the same order.
bool host_pitch_feats(const float *pitch, int64_t T, float sample_rate, int columns, int left, int right, int delta_window,
                      float pov_scale, float pov_offset, float pitch_scale, float delta_scale, float *feats)
{
    PitchFeatShape s;
    if (!pitch_feat_shape(columns, left, right, delta_window, pov_scale, pov_offset, pitch_scale, delta_scale, s)) return false;
    if (T < 0 || T > 0x7fffffff || !std::isfinite(sample_rate) || !(sample_rate > 0.f) || (T > 0 && (!pitch || !feats))) return false;
    std::vector<double> w((size_t)T), p((size_t)T);
    const double rate = (double)sample_rate;
    for (int64_t t = 0; t < T; ++t) {
        const double n = std::fmin(1.0, std::fmax(-1.0, (double)pitch[2 * t + 1]));
        const double a = std::fabs(n);
        const double a1 = a - 1.0;
        const double x1 = 7.5 * a1, x2 = -10.0 * a, x3 = 20.0 * a1;
        const double e1 = 5.4 * std::exp(x1), e2 = 4.8 * a, e3 = 2.0 * std::exp(x2), e4 = 4.2 * std::exp(x3);
        double r = -5.2 + e1;
        r = r + e2;
        r = r - e3;
        r = r + e4;
        const double en = std::exp(-r);
        const double dn = 1.0 + en;
        w[(size_t)t] = 1.0 / dn;
        const double ratio = rate / (double)pitch[2 * t];
        p[(size_t)t] = std::log(ratio);
    }
    for (int64_t t = 0; t < T; ++t) {
        float *out = feats + t * s.F;
        const double pt = p[(size_t)t];
        if (s.columns & 1) {
            const double n = std::fmin(1.0, std::fmax(-1.0, (double)pitch[2 * t + 1]));
            const double b = 1.0001 - n;
            const double y = std::pow(b, 0.15) - 1.0;
            const double v = (double)pov_scale * y;
            *out++ = (float)(v + (double)pov_offset);
        }
        if (s.columns & 2) {
            const int64_t lo = std::max<int64_t>(0, t - s.left), hi = std::min<int64_t>(T - 1, t + s.right);
            double sw = 0.0, sp = 0.0;
            for (int64_t i = lo; i <= hi; ++i) {
                const double wp = w[(size_t)i] * p[(size_t)i];
                sw = sw + w[(size_t)i];
                sp = sp + wp;
            }
            const double mean = sp / sw;
            const double d = pt - mean;
            *out++ = (float)((double)pitch_scale * d);
        }
        if (s.columns & 4) {
            double num = 0.0;
            for (int l = 1; l <= s.D; ++l) {
                const double d = p[(size_t)std::min<int64_t>(T - 1, t + l)] - p[(size_t)std::max<int64_t>(0, t - l)];
                const double ld = (double)l * d;
                num = num + ld;
            }
            const double v = (double)delta_scale * num;
            *out++ = (float)(v / s.den);
        }
        if (s.columns & 8) *out++ = (float)pt;
    }
    return true;
}

} // namespace mfx

extern "C" int mfx_host_pitch_feats(const float *pitch, int64_t T, float sample_rate, int32_t columns, int32_t left, int32_t right,
                                    int32_t delta_window, float pov_scale, float pov_offset, float pitch_scale, float delta_scale,
                                    float *feats)
{
    return mfx::host_pitch_feats(pitch, T, sample_rate, columns, left, right, delta_window, pov_scale, pov_offset, pitch_scale,
                                 delta_scale, feats)
               ? 0
               : -7 /* MFX_ERR_ARG */;
}

// (the C entry of include/mfx.h, here beside its definition so that the stand-alone sanitizer program links it without HIP)
extern "C" int mfx_host_pitch(const int16_t *pcm, int64_t n, int32_t channels, int64_t T, int32_t shift, int32_t window, int32_t lag_min,
                              int32_t lag_max, float ballast, float lag_cost, float penalty, int32_t max_jump, float *pitch, int32_t *index,
                              float *nccf)
{
    return mfx::host_pitch(pcm, n, channels, T, shift, window, lag_min, lag_max, ballast, lag_cost, penalty, max_jump, pitch, index, nccf)
               ? 0
               : -7 /* MFX_ERR_ARG */;
}

extern "C" int mfx_host_online_norm(const float *rows, int64_t T, int32_t pitch, int32_t Wn, int32_t kind, int32_t window,
                                    int32_t prior_frames, int64_t prior_count, const double *prior_acc, float *out)
{
    return mfx::host_online_norm(rows, T, pitch, Wn, kind, window, prior_frames, prior_count, prior_acc, out) ? 0 : -7 /* MFX_ERR_ARG */;
}

extern "C" int mfx_host_sliding_window(int64_t T, int32_t window, int32_t min_window, int32_t center, int64_t t, int64_t *ws, int64_t *we)
{
    if (window < 1 || window > 4096 || min_window < 0 || min_window > window || (center != 0 && center != 1) || t < 0 || t >= T || !ws || !we)
        return -7 /* MFX_ERR_ARG */;
    mfx::slide_window<int64_t>(T, window, min_window, center != 0, t, *ws, *we);
    return 0;
}

extern "C" int mfx_host_sliding_norm(const float *rows, int64_t T, int32_t W, int32_t pitch, int32_t window, int32_t min_window,
                                     int32_t center, int32_t norm_vars, float *out, int32_t out_pitch)
{
    return mfx::host_sliding_norm(rows, T, W, pitch, window, min_window, center, norm_vars, out, out_pitch) ? 0 : -7 /* MFX_ERR_ARG */;
}

// ------------------------------------------------------------------------------------------------
// dense padded tensor output (mfx_batch_set_tensor; DESIGN.md, "Tensor output")
// ------------------------------------------------------------------------------------------------
namespace mfx {

int64_t tensor_bytes(int64_t B, int64_t Wo, int64_t Tp, int dtype)
{
    if (B < 0 || Wo < 0 || Tp < 0 || Tp > kTensorPadMax || dtype < kDtypeF32 || dtype > kDtypeBf16) return -1;
    int64_t n = 0;
    if (__builtin_mul_overflow(B, Tp, &n) || __builtin_mul_overflow(n, Wo, &n) ||
        __builtin_mul_overflow(n, (int64_t)tensor_elem_bytes(dtype), &n))
        return -1;
    return n;
}

uint16_t f32_to_f16_bits(uint32_t u)
{
    const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((a >> 13) & 0x3ffu)); // NaN, made quiet
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u); // 65520 and above (inf included) round to inf
    if (a >= 0x38800000u) { // normal result: 2^-14 and above
        const uint32_t v = a - 0x38000000u; // exponent rebiased; a carry out of the mantissa moves into it
        return (uint16_t)(sign | ((v + 0xfffu + ((v >> 13) & 1u)) >> 13));
    }
    if (a < 0x33000000u) return (uint16_t)sign; // below 2^-25: zero (2^-25 itself is a tie to even: zero, handled below)
    // subnormal result: the 24-bit significand shifted down to units of 2^-24
    const uint32_t e = a >> 23, m = (a & 0x7fffffu) | 0x800000u;
    const uint32_t sh = 126u - e; // 14 .. 24
    const uint32_t q = m >> sh, rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1);
    return (uint16_t)(sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));
}

uint16_t f32_to_bf16_bits(uint32_t u)
{
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u); // NaN, made quiet
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16); // (a carry runs through the exponent: overflow gives inf)
}

bool tensor_pack_host(const float *rows, const int64_t *out_rows, const int32_t *lengths, int64_t B, int Wo, int64_t Tp, int layout,
                      int dtype, float pad, void *out)
{
    const int64_t bytes = tensor_bytes(B, Wo, Tp, dtype);
    if (bytes < 0 || Wo < 1 || (layout != kTensorTimeMajor && layout != kTensorChannelMajor)) return false;
    if (bytes == 0) return true;
    if (!out || !out_rows || !lengths) return false;
    for (int64_t u = 0; u < B; ++u)
        if (lengths[u] < 0 || out_rows[u] < 0 || (!rows && lengths[u] > 0 && Tp > 0)) return false;
    auto put = [&](int64_t idx, float v) {
        uint32_t bits;
        std::memcpy(&bits, &v, 4);
        if (dtype == kDtypeF32)
            std::memcpy((char *)out + idx * 4, &bits, 4);
        else {
            const uint16_t s = dtype == kDtypeF16 ? f32_to_f16_bits(bits) : f32_to_bf16_bits(bits);
            std::memcpy((char *)out + idx * 2, &s, 2);
        }
    };
    for (int64_t u = 0; u < B; ++u) {
        const int64_t len = std::min<int64_t>(lengths[u], Tp);
        for (int64_t t = 0; t < Tp; ++t)
            for (int64_t c = 0; c < Wo; ++c) {
                const float v = t < len ? rows[(out_rows[u] + t) * Wo + c] : pad;
                put(layout == kTensorTimeMajor ? (u * Tp + t) * Wo + c : (u * Wo + c) * Tp + t, v);
            }
    }
    return true;
}

} // namespace mfx

extern "C" int64_t mfx_host_tensor_bytes(int64_t B, int32_t Wo, int64_t Tp, int32_t dtype)
{
    const int64_t n = mfx::tensor_bytes(B, Wo, Tp, dtype);
    return n < 0 ? -7 /* MFX_ERR_ARG */ : n;
}

extern "C" int mfx_host_tensor_pack(const float *rows, const int64_t *out_rows, const int32_t *lengths, int64_t B, int32_t Wo, int64_t Tp,
                                    int32_t layout, int32_t dtype, float pad, void *out)
{
    return mfx::tensor_pack_host(rows, out_rows, lengths, B, Wo, Tp, layout, dtype, pad, out) ? 0 : -7 /* MFX_ERR_ARG */;
}

extern "C" int64_t mfx_host_tensor_lds_bytes(int32_t Wo, int32_t *tile_rows)
{
    if (Wo < 1) return -7 /* MFX_ERR_ARG */;
    if (tile_rows) *tile_rows = mfx::kTensorTileRows;
    return (int64_t)mfx::tensor_lds_bytes(Wo);
}
