// Sanitizer run of the host table builders (csrc/mfx_tables.cpp) under -fsanitize=address,undefined: mel table, DCT
// matrix, twiddles, the mel lane plans (16 lanes at 512 and 1024 points, 64 lanes, 32 lanes at 2048 points), over a grid of
// configurations (bank counts, transform sizes, sample rates, band edges, VTLN warps), and the front ends' FFT pass / split
// twiddle tables and window layouts, and the sample-rate converter's tap tables, lengths and layouts.  Built by `make -C csrc asan`.
#include <cstdio>
#include <vector>

#include "../../asr-featext-opencl_amd/csrc/mfx_tables.h"

int main()
{
    int n = 0;
    const int ffts[] = {64, 128, 256, 512, 1024, 2048, 4096};
    const int banks[] = {1, 2, 3, 15, 16, 17, 26, 40, 41, 64, 80, 128};
    const float srs[] = {8000.f, 16000.f, 44100.f};
    const float alphas[] = {0.8f, 1.0f, 1.2f};
    for (int fft : ffts)
        for (int nb : banks)
            for (float sr : srs)
                for (float alpha : alphas)
                    for (int lo = 0; lo < 2; ++lo) {
                        mfx::MelTable t;
                        mfx::build_mel_table(nb, fft, sr, lo ? 300.f : 0.f, lo ? sr / 2 - 100.f : sr / 2, alpha, t);
                        bool edges_ok = true;
                        for (int v : t.beg) edges_ok = edges_ok && v >= 0 && v <= fft / 2;
                        if (!edges_ok) continue; // the product refuses such a configuration (mfx_create: MFX_ERR_CONFIG)
                        mfx::MelPlan pl;
                        if (fft == 512) (void)mfx::build_mel_plan(t, nb, fft, 511 - 32, 16, 2, pl);
                        if (fft == 1024) (void)mfx::build_mel_plan(t, nb, fft, 527, 16, 4, pl);
                        (void)mfx::build_mel_plan(t, nb, fft, fft - 1, 64, 2, pl);
                        if (fft == 2048) (void)mfx::build_mel_plan(t, nb, fft, 1039, 32, 2, pl);
                        for (int ceps : {0, 1, 12, 13, 40}) {
                            if (ceps == 0) continue;
                            std::vector<float> m, mt;
                            mfx::build_dct_matrix(nb, ceps, (nb + ceps) & 1, 22.f, m);
                            int stride = 0, nb_pad = 0;
                            mfx::build_dct_transposed(m, nb, ceps + ((nb + ceps) & 1), stride, nb_pad, mt);
                        }
                        ++n;
                    }
    std::vector<float> tw;
    for (int fft : ffts) mfx::build_twiddles(fft, fft / 2 + 1, tw);
    // the FFT and window tables of the front ends, on the shapes the kernels use: every transform size, the zero-stuffed
    // forms below 512 points, a 400-sample window and a window longer than 512 samples at 1024 points
    int nt = 0;
    for (int fft : ffts) {
        std::vector<float> t, t2;
        for (bool stuffed : {false, true}) {
            if (stuffed && fft >= 512) continue; // (k_front512 stuffs 256 / 128 / 64 points only)
            mfx::build_split_twiddles(fft, stuffed, t);
            if (t.size() != (size_t)2 * ((stuffed ? 512 : fft) / 2 + 1)) return 1;
            ++nt;
        }
        if (fft >= 1024) mfx::build_reg_pass_twiddles(fft, t), ++nt;
        for (int W : {fft / 2 + 1, 400, 800, fft}) {
            if (W > fft) continue;
            std::vector<float> padded((size_t)fft, 0.f);
            for (int i = 0; i < W; ++i) padded[i] = 0.5f + 0.001f * (float)i;
            if (fft <= 512) mfx::build_window_pairs(padded, fft, /*stuffed=*/fft < 512, t), ++nt;
            if (fft == 1024 && W <= 512) {
                mfx::build_window_pairs(padded, fft, false, t);
                mfx::build_front1024_phase_o(padded, fft, t2);
                nt += 2;
            }
            if (fft == 1024 && W > 512) mfx::build_front1024_long_window(padded, fft, t, t2), ++nt;
        }
    }
    mfx::build_pass256_twiddles(tw);
    for (long s : {0L, 1L, 399L, 400L, 160000L, 57600000L, 1L << 31})
        for (int W : {400, 1024}) (void)mfx::frame_count(s, W, 160);
    // run lists of mfx_batch_set_alphas: ragged frame counts (frameless utterances included), few and many distinct factors,
    // clipped to slab windows of every size class; every row of the batch must come out exactly once
    int nr = 0;
    for (int n_utt : {0, 1, 9, 257, 5000})
        for (int distinct : {1, 3, 21, 4096}) {
            std::vector<float> alphas((size_t)n_utt);
            std::vector<int64_t> frames((size_t)n_utt);
            int64_t total = 0;
            for (int u = 0; u < n_utt; ++u) {
                alphas[u] = 0.8f + 1e-5f * (float)((u * 7) % distinct);
                frames[u] = (int64_t)((u * 37) % 11 == 0 ? 0 : (u * 131) % 1003);
                total += frames[u];
            }
            std::vector<float> tables;
            std::vector<int32_t> off;
            std::vector<int64_t> runs;
            mfx::build_alpha_runs(alphas.data(), frames.data(), n_utt, tables, off, runs);
            if (off.size() != tables.size() + 1 || (size_t)off.back() * 2 != runs.size()) return 1;
            for (int64_t slab : {(int64_t)1, (int64_t)64, (int64_t)4097, total + 1}) {
                int64_t seen = 0;
                for (int64_t w0 = 0; w0 < total; w0 += slab) {
                    std::vector<int32_t> o2 = off;
                    std::vector<int64_t> r2 = runs;
                    mfx::clip_alpha_runs(w0, slab, o2, r2);
                    for (size_t r = 0; r < r2.size(); r += 2) seen += r2[r + 1];
                    if (slab == 1 && total > 20000 && w0 > 2000) { // (the one-row slabs of the long batches: a sample)
                        seen += total - w0 - slab;
                        break;
                    }
                }
                if (seen != total) return 1;
                ++nr;
            }
        }
    // operands of k_splice_affine: exactly-sized input and output buffers at the corners of the limits
    int nx = 0;
    for (int od : {1, 15, 16, 17, 40, 256})
        for (int id : {1, 3, 4, 39, 351, 8192}) {
            std::vector<float> A((size_t)od * id, 1.f), ops((size_t)((id + 3) / 4) * ((od + 15) / 16) * 64);
            int tiles = 0, steps = 0;
            mfx::build_xform_operands(A.data(), od, id, tiles, steps, ops.data());
            double sum = 0;
            for (float v : ops) sum += v;
            if ((size_t)steps * tiles * 64 != ops.size() || sum != (double)od * id) return 1;
            ++nx;
        }
    // session entries: push sequences through the planner's step (empty, one-sample, sub-hop and long pushes; the flush as
    // a zero-sample final push): the rows delivered add up to the utterance's frames and the carry stays inside a slot
    int nq = 0;
    for (int W : {200, 400, 1102, 2048})
        for (int S : {80, 160, 441, 512})
            for (int D : {0, 2, 6, 20}) {
                if (S > W) continue;
                const int64_t pushes[] = {0, 1, S - 1, S, W - 1, W, 3000, 0, 7, 2 * W + 3, 1, 0};
                int64_t n = 0, E = 0, total = 0, rows = 0;
                const int count = (int)(sizeof(pushes) / sizeof(pushes[0]));
                for (int k = 0; k < count; ++k) {
                    mfx::SessionStep st;
                    total += pushes[k];
                    rows += mfx::session_step(W, S, D, n, E, pushes[k], k + 1 == count, st);
                    if (st.carry_samples < 0 || st.carry_samples >= W + S || st.carry_rows < 0 || st.carry_rows > 2 * D ||
                        st.static_off - st.shift != D || st.n_out < 0)
                        return 1;
                }
                const int64_t T = mfx::frame_count(total, W, S);
                if (rows != (T > 0 ? T : 0) || n != 0 || E != 0) return 1;
                ++nq;
            }
    // sample-rate conversion: exactly-sized tap tables at the corners of the limits, lengths and layouts
    int nv = 0;
    {
        const int pairs[][2] = {{48000, 16000}, {8000, 16000}, {44100, 16000}, {11025, 16000}, {17600, 16000}, {16000, 44100},
                                {768000, 1000}, {1000, 768000}, {4096, 4095}, {16000, 16000}};
        for (const auto &pr : pairs)
            for (int zeros : {0, 1, 6, 64})
                for (float ro : {0.f, 0.25f, 1.f}) {
                    mfx::ResampleShape sh;
                    if (mfx::resample_shape(pr[0], pr[1], zeros, ro, sh) != 0) continue; // (outside the limits: refused)
                    std::vector<float> taps((size_t)sh.L * sh.P);
                    mfx::build_resample_taps(sh, taps.data());
                    double sum = 0;
                    for (float v : taps) sum += v;
                    if (!(sum > 0.8 * sh.L && sum < 1.1 * sh.L)) return 1; // the phases sum to about 1 (0.82 at one zero crossing)
                    ++nv;
                }
        std::vector<int64_t> lens = {0, 1, 2, 4411, 16000, 7, 48001, 3, 0, 8000, (int64_t)1 << 40}, off(lens.size()), out(lens.size());
        std::vector<int32_t> rates = {8000, 44100, 16000, 44100, 16000, 16000, 48000, 11025, 16000, 8000, 48000};
        const int64_t total = mfx::resample_layout((int32_t)lens.size(), lens.data(), rates.data(), 16000, off.data(), out.data());
        if (total != off.back() + ((out.back() + 1) & ~(int64_t)1) || mfx::resampled_length(((int64_t)1 << 40) + 1, 48000, 16000) != 366503875926)
            return 1;
        rates[3] = 500;
        if (mfx::resample_layout((int32_t)lens.size(), lens.data(), rates.data(), 16000, nullptr, nullptr) != -1) return 1;
        // the rate-set builder of both planners: the rates the recorded cases use (tests/resample_bits_cases.py), the output rate
        // among them, mono and stereo; then what it refuses, and the one difference between its callers
        for (int ch : {1, 2}) {
            mfx::ResRateSet s;
            const int32_t to16[] = {48000, 8000, 16000, 44100, 11025, 12345}, to44[] = {44142, 200000, 44100};
            if (mfx::build_resample_rates(ch, 16000, to16, 6, 0, 0.f, true, s) != 0 || s.rates.size() != 6) return 1;
            size_t floats = 0;
            for (const mfx::ResRate &r : s.rates) {
                if ((r.tile_out == 0) != (&r == &s.rates[2]) || r.tile_out != r.R * r.items || (r.tile_out & 1)) return 1;
                if (r.tile_out && (r.taps_off != (int64_t)floats || mfx::resample_span_floats(r) > s.lds.x_floats)) return 1;
                floats += (size_t)r.L * r.P;
            }
            if (s.taps.size() != floats || s.lds.taps_floats != 9600 /* 11025 Hz: 640 x 15 */ || (s.lds.x_floats & 7) || (s.lds.out_elems & 1)) return 1;
            if (s.carry_cap != 48 /* 48000 Hz: 2 x 19 + 3 + 2, up to 8 */ || s.tile_min != 1280 /* 11025 Hz */) return 1;
            if (mfx::build_resample_rates(ch, 44100, to44, 3, 0, 0.f, false, s) != 0) return 1;
            if (ch == 1 && mfx::resample_lds_bytes(1, mfx::ResLds{s.rates[0].in_lds ? 15752 : 0, mfx::resample_span_floats(s.rates[0]), 2048}) != 75424) return 1;
            if (s.rates[1].in_lds || s.rates[1].R != (ch == 2 ? 2 : 4) || s.rates[2].tile_out != 0) return 1;
        }
        mfx::ResRateSet s;
        const int32_t far[] = {8000, 16001}, same[] = {16000};
        if (mfx::build_resample_rates(1, 16000, far, 2, 0, 0.f, true, s) != 4) return 1;       // L = 16000 > 4096
        if (mfx::build_resample_rates(1, 16000, far, 1, 65, 0.f, false, s) != 2) return 1;     // zeros
        if (mfx::build_resample_rates(1, 16000, same, 1, 65, 0.f, true, s) != 2) return 1;     // the sessions judge zeros at the output rate
        if (mfx::build_resample_rates(1, 16000, same, 1, 65, 0.f, false, s) != 0 || s.taps.size() != 4 || s.tile_min != mfx::kResCopyTile)
            return 1;                                                                         // a plan does not
        if (mfx::kResampleWhy[4][0] != 'L' || mfx::kResampleWhy[0][0] != 0) return 1;
        ++nv;
    }
    // STFT log-mel: exactly-sized basis, Slaney table and operand buffers at the corners of the method's limits
    int ns = 0;
    for (int N : {32, 34, 64, 400, 414, 416, 510, 512})
        for (int M : {1, 8, 80, 128}) {
            const int K1 = N / 2 + 1;
            std::vector<float> win((size_t)N, 0.5f), basis((size_t)2 * K1 * N), w((size_t)M * K1), ops;
            std::vector<int32_t> beg((size_t)M), len((size_t)M);
            mfx::build_stft_basis(N, win.data(), basis.data());
            for (float sr : {8000.f, 16000.f}) {
                mfx::build_slaney_mel(M, N, sr, 0.f, sr / 2, w.data(), beg.data(), len.data());
                for (int m = 0; m < M; ++m)
                    if (beg[m] < 0 || len[m] < 0 || beg[m] + len[m] > K1) return 1;
            }
            const int nbt = (K1 + 15) / 16, tb = nbt < 13 ? nbt : 13;
            mfx::build_stft_operands(basis.data(), N, tb, ops);
            if (ops.size() != (size_t)((nbt + tb - 1) / tb) * ((N + 3) / 4) * 2 * tb * 64) return 1;
            double a = 0, b = 0; // every basis value appears exactly once among the operands (the sums run in another order)
            size_t na = 0, nb = 0;
            for (float v : ops) a += (double)v * v, na += v != 0.f;
            for (float v : basis) b += (double)v * v, nb += v != 0.f;
            if (na != nb || !(a >= b * (1 - 1e-9) && a <= b * (1 + 1e-9))) return 1;
            std::vector<float> form_ops, spans; // the two builders the handle goes through: the same operands, the spans packed
            std::vector<int32_t> meta;
            mfx::build_stft_form_operands(mfx::stft_form(N), N, win.data(), form_ops);
            mfx::build_slaney_spans(M, N, 16000.f, 0.f, 8000.f, spans, meta);
            if (form_ops != ops || meta.size() != (size_t)3 * M || spans.empty()) return 1;
            for (int m = 0; m < M; ++m)
                if (meta[m] != beg[m] || meta[M + m] != len[m] || (len[m] > 0 && spans[meta[2 * M + m]] != w[(size_t)m * K1 + beg[m]])) return 1;
            ++ns;
        }
    for (long s : {0L, 200L, 201L, 159L, 160L, 1L << 40})
        if (mfx::stft_frame_count(s, 400, 160) != (s <= 200 ? 0 : s / 160)) return 1;
    std::printf("tables_asan: %d STFT table sets; ", ns);
    std::printf("tables_asan: %d resampler tables; ", nv);
    std::printf("tables_asan: %d configurations, %d front-end tables, %d run lists, %d transform operand sets, %d session push sequences clean\n",
                n, nt, nr, nx, nq);
    return 0;
}
