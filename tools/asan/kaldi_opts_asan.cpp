// kaldi_opts_asan.cpp -- the frame rule of the Kaldi front end under snip_edges = false (mfx_tables: kaldi_frame_count,
// kaldi_reflect, kaldi_frame_samples, which mfx_host_kaldi_frame_samples and k_kaldi_front_opts use) under AddressSanitizer +
// UBSan, CPU only (`make asan` in asr-featext-opencl_amd/csrc builds and runs it).  For every n in 0 .. 3 W the indices of every
// frame go into a buffer of exactly W elements; the closed form is held against Kaldi's loop, and every index must lie in [0, n).
// A chunk's staging span, gathered the way the kernel gathers it from the unreflected start, is held against the frames.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../asr-featext-opencl_amd/csrc/mfx_tables.h"

namespace {

// Kaldi's loop (feature-window.cc)
int64_t mirror_loop(int64_t s, int64_t n)
{
    while (s < 0 || s >= n) s = s < 0 ? -s - 1 : 2 * n - 1 - s;
    return s;
}

int fail(const char *what, int W, int S, int64_t n, int64_t t, int i)
{
    std::printf("FAILED %s: W %d S %d n %lld t %lld tap %d\n", what, W, S, (long long)n, (long long)t, i);
    return 1;
}

int check_shape(int W, int S)
{
    using namespace mfx;
    for (int64_t n = 0; n <= 3 * (int64_t)W; ++n) {
        const int64_t T = kaldi_frame_count(n, W, S, kKaldiNoSnipEdges);
        if (T != (n > 0 ? (n + S / 2) / S : 0)) return fail("frame count", W, S, n, T, 0);
        if (kaldi_frame_count(n, W, S, 0) != frame_count(n, W, S)) return fail("snip-edged count", W, S, n, 0, 0);
        for (int64_t t = 0; t < T; ++t) {
            std::unique_ptr<int64_t[]> idx(new int64_t[W]); // exactly W elements
            kaldi_frame_samples(n, W, S, kKaldiNoSnipEdges, t, idx.get());
            for (int i = 0; i < W; ++i) {
                if (idx[i] < 0 || idx[i] >= n) return fail("index outside the utterance", W, S, n, t, i);
                if (idx[i] != mirror_loop(t * S + S / 2 - W / 2 + i, n)) return fail("closed form != loop", W, S, n, t, i);
            }
        }
        // the span of a chunk of up to 16 frames from t0, as the kernel stages it: sample j of the span is tap j - f S of frame t0 + f
        for (int64_t t0 = 0; t0 < T; t0 += 16) {
            const int rows = (int)(T - t0 < 16 ? T - t0 : 16);
            const int span = (rows - 1) * S + W;
            std::vector<int64_t> sp((size_t)span);
            const int64_t s0 = kaldi_centred_start(t0, W, S);
            for (int j = 0; j < span; ++j) {
                int64_t s = s0 + j;
                if (s < 0 || s >= n) s = kaldi_reflect(s, n);
                sp[(size_t)j] = s;
            }
            std::unique_ptr<int64_t[]> idx(new int64_t[W]);
            for (int f = 0; f < rows; ++f) {
                kaldi_frame_samples(n, W, S, kKaldiNoSnipEdges, t0 + f, idx.get());
                for (int i = 0; i < W; ++i)
                    if (sp.at((size_t)f * S + i) != idx[i]) return fail("span != frame", W, S, n, t0 + f, i);
            }
        }
    }
    return 0;
}

} // namespace

int main()
{
    const int shapes[][2] = {{400, 160}, {401, 161}, {512, 512}, {65, 1}, {200, 80}, {512, 1}, {65, 65}, {255, 7}};
    for (const auto &s : shapes)
        if (check_shape(s[0], s[1])) return 1;
    // far outside: one sample, and indices of either sign near the int32 range
    for (int64_t s : {(int64_t)-3000000000LL, (int64_t)-1, (int64_t)0, (int64_t)3000000000LL})
        for (int64_t n : {(int64_t)1, (int64_t)7, (int64_t)1000})
            if (mfx::kaldi_reflect(s, n) < 0 || mfx::kaldi_reflect(s, n) >= n) return fail("far index", 0, 0, n, s, 0);
    for (int64_t s = -50; s < 50; ++s)
        if (mfx::kaldi_reflect(s, 7) != mirror_loop(s, 7)) return fail("small mirror", 0, 0, 7, s, 0);
    std::printf("frame rule clean\n");
    return 0;
}
