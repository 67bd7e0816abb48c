// Sanitizer run of the host side of mfx_batch_set_pitch (csrc/mfx_tables.cpp) under -fsanitize=address,undefined: the tile
// layout (build_utt_tiling: the empty batch, frameless utterances, lengths on, before and after the tile edge, a negative
// count, more tiles than an int32 holds), the padded span (every sample of a tile's span in a slot of its own below
// pitch_span_slots, frames of a tile on different banks) and the host restatement (host_pitch: K = 1, the largest span, stereo,
// shift 1, utterances shorter than a frame's span, null outputs, every refusal with nothing written).  Built by
// `make -C csrc asan`.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../asr-featext-opencl_amd/csrc/mfx_tables.h"

static bool layouts(int &n)
{
    const int64_t edge[] = {0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 4097, 360000};
    const int n_edge = (int)(sizeof(edge) / sizeof(edge[0]));
    for (int tf : {1, 7, 16, 64})
        for (int n_utt : {0, 1, 2, 14, 257, 3000}) {
            std::vector<int64_t> frames((size_t)n_utt);
            for (int u = 0; u < n_utt; ++u) frames[u] = n_utt <= 14 ? edge[(u * 5 + n_utt) % n_edge] : ((u * 37) % 11 == 0 ? 0 : (u * 131) % 901);
            std::vector<int32_t> t0, tu;
            if (!mfx::build_utt_tiling(frames.data(), n_utt, tf, t0, &tu)) return false;
            if (t0.size() != (size_t)n_utt + 1 || t0[0] != 0 || t0[n_utt] != (int32_t)tu.size()) return false;
            for (int u = 0; u < n_utt; ++u) {
                if (t0[u + 1] - t0[u] != (int32_t)((frames[u] + tf - 1) / tf)) return false;
                for (int32_t t = t0[u]; t < t0[u + 1]; ++t)
                    if (tu[(size_t)t] != u) return false;
            }
            ++n;
            if (n_utt > 0) { // a negative count is refused and nothing is written
                std::vector<int64_t> bad = frames;
                bad[(size_t)n_utt / 2] = -1;
                std::vector<int32_t> a(3, 7), b(2, 9);
                if (mfx::build_utt_tiling(bad.data(), n_utt, tf, a, &b) || a.size() != 3 || a[0] != 7 || b.size() != 2) return false;
            }
        }
    std::vector<int64_t> huge(80, (int64_t)0x7fffffff);
    std::vector<int32_t> a, b;
    if (mfx::build_utt_tiling(huge.data(), 80, 1, a, &b) || !a.empty() || !b.empty()) return false;
    if (mfx::build_utt_tiling(huge.data(), 1, 0, a, &b) || mfx::build_utt_tiling(huge.data(), -1, 1, a, &b) || !a.empty() || !b.empty()) return false;
    return true;
}

static bool spans(int &n)
{
    for (int window : {32, 400, 1024})
        for (int lag_max : {40, 320, 1024})
            for (int shift : {1, 3, 63, 64, 100, 160, 161, 400, 1024, 5000, 40000}) {
                const int tf = mfx::pitch_tile_frames(window, lag_max, shift), pad = mfx::pitch_span_pad(shift);
                const int slots = mfx::pitch_span_slots(window, lag_max, shift, tf);
                if (tf < 1 || tf > 64 || pad < 0 || pad > 63 || slots > mfx::kPitchSpanMax) return false;
                if (tf < 64 && mfx::pitch_span_slots(window, lag_max, shift, tf + 1) <= mfx::kPitchSpanMax) return false;
                const int span = (tf - 1) * shift + window + lag_max;
                std::vector<uint8_t> used((size_t)slots, 0);
                for (int i = 0; i < span; ++i) { // the slot the kernel gives sample i
                    const int at = i + pad * (i / shift);
                    if (at >= slots || used[(size_t)at]++) return false;
                }
                if (shift >= 64) // 32 consecutive frames start in 32 different banks (4-byte banks, 2-byte slots)
                    for (int f = 1; f < 32 && f < tf; ++f)
                        if ((((f * shift) + pad * f) / 2) % 32 != f % 32) return false;
                ++n;
            }
    return true;
}

static bool tracks(int &n)
{
    struct Case {
        int n, ch, shift, window, lag_min, lag_max, jump;
    };
    const Case cases[] = {{3000, 1, 160, 400, 40, 320, 16}, {1500, 2, 160, 400, 40, 320, 0},  {400, 1, 160, 400, 2, 2, 0},
                          {2300, 1, 160, 1024, 513, 1024, 511}, {120, 1, 1, 32, 2, 40, 1},     {31, 1, 7, 32, 2, 9, 3},
                          {0, 1, 160, 400, 40, 320, 16}};
    for (const Case &c : cases) {
        std::vector<int16_t> pcm((size_t)c.n * c.ch);
        for (size_t i = 0; i < pcm.size(); ++i) pcm[i] = (int16_t)(20000.0 * std::sin(0.05 * (double)i) + (double)((i * 7919) % 257) - 128.0);
        const int64_t T = c.n >= c.window ? (c.n - (c.window - c.shift)) / c.shift : 0;
        const int K = c.lag_max - c.lag_min + 1;
        std::vector<float> pitch((size_t)T * 2, -1.f), nccf((size_t)T * K, -9.f);
        std::vector<int32_t> index((size_t)T, -1);
        if (!mfx::host_pitch(pcm.data(), c.n, c.ch, T, c.shift, c.window, c.lag_min, c.lag_max, 0.f, 0.1f, 1.f, c.jump, pitch.data(),
                             index.data(), nccf.data()))
            return false;
        for (int64_t t = 0; t < T; ++t) {
            if (index[(size_t)t] < 0 || index[(size_t)t] >= K) return false;
            const float lag = pitch[2 * (size_t)t], rho = pitch[2 * (size_t)t + 1];
            if (!(lag >= (float)c.lag_min - 0.5f && lag <= (float)c.lag_max + 0.5f) || !std::isfinite(rho)) return false;
            if (rho != nccf[(size_t)t * K + index[(size_t)t]]) return false;
        }
        // any output may be null, and the rest is the same
        std::vector<int32_t> again((size_t)T, -1);
        if (!mfx::host_pitch(pcm.data(), c.n, c.ch, T, c.shift, c.window, c.lag_min, c.lag_max, 0.f, 0.1f, 1.f, c.jump, nullptr, again.data(),
                             nullptr) || again != index)
            return false;
        if (!mfx::host_pitch(pcm.data(), c.n, c.ch, T, c.shift, c.window, c.lag_min, c.lag_max, 0.f, 0.1f, 1.f, c.jump, nullptr, nullptr, nullptr))
            return false;
        ++n;
    }
    // refusals: nothing is written
    std::vector<int16_t> pcm(2000, 100);
    float canary[4] = {5.f, 5.f, 5.f, 5.f};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    auto refused = [&](int ch, int64_t T, int shift, int w, int l0, int l1, float bal, float lc, float pen, int mj) {
        return !mfx::host_pitch(pcm.data(), 2000 / ch, ch, T, shift, w, l0, l1, bal, lc, pen, mj, canary, nullptr, nullptr) && canary[0] == 5.f &&
               canary[1] == 5.f;
    };
    const bool all = refused(1, 1, 160, 31, 40, 320, 0, 0, 0, 0) && refused(1, 1, 160, 1025, 40, 320, 0, 0, 0, 0) &&
                     refused(1, 1, 160, 0, 40, 320, 0, 0, 0, 0) && refused(1, 1, 160, 400, 1, 320, 0, 0, 0, 0) &&
                     refused(1, 1, 160, 400, 40, 1025, 0, 0, 0, 0) && refused(1, 1, 160, 400, 40, 39, 0, 0, 0, 0) &&
                     refused(1, 1, 160, 400, 2, 514, 0, 0, 0, 0) && refused(1, 1, 160, 400, 40, 320, -1.f, 0, 0, 0) &&
                     refused(1, 1, 160, 400, 40, 320, inf, 0, 0, 0) && refused(1, 1, 160, 400, 40, 320, 0, nan, 0, 0) &&
                     refused(1, 1, 160, 400, 40, 320, 0, 1.5f, 0, 0) && refused(1, 1, 160, 400, 40, 320, 0, -0.1f, 0, 0) &&
                     refused(1, 1, 160, 400, 40, 320, 0, 0, -1.f, 0) && refused(1, 1, 160, 400, 40, 320, 0, 0, inf, 0) &&
                     refused(1, 1, 160, 400, 40, 320, 0, 0, 0, -1) && refused(1, 1, 160, 400, 40, 320, 0, 0, 0, 512) &&
                     refused(3, 1, 160, 400, 40, 320, 0, 0, 0, 0) && refused(1, -1, 160, 400, 40, 320, 0, 0, 0, 0) &&
                     refused(1, 1, 0, 400, 40, 320, 0, 0, 0, 0);
    if (!all) return false;
    if (mfx::host_pitch(nullptr, 5, 1, 0, 160, 400, 40, 320, 0, 0, 0, 0, nullptr, nullptr, nullptr)) return false;
    ++n;
    return true;
}

int main()
{
    int nl = 0, ns = 0, nt = 0;
    if (!layouts(nl)) return 1;
    if (!spans(ns)) return 2;
    if (!tracks(nt)) return 3;
    std::printf("pitch_asan: %d layouts, %d spans, %d tracks clean\n", nl, ns, nt);
    return 0;
}
