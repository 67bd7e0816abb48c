// Sanitizer run of the host layout of mfx_batch_set_vad (csrc/mfx_tables.cpp: build_utt_tiling at kVadTileRows and at
// kNormChunkRows) under -fsanitize=address,undefined: the empty batch, frameless utterances, lengths on, before and after the
// 64-row tile and the 4096-row chunk edges, one long stream, a negative count.  Every row must lie in exactly one tile and one
// chunk of its own utterance, in order; and the two tilings are the two layouts the VAD used to build in one pass, restated
// here.  Built by `make -C csrc asan`.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../asr-featext-opencl_amd/csrc/mfx_tables.h"

// the VAD's layout as one pass over the utterances built it before there was a shared builder
static void one_pass(const std::vector<int64_t> &frames, std::vector<int32_t> &t0, std::vector<int32_t> &tu, std::vector<int32_t> &c0,
                     std::vector<int32_t> &cu)
{
    t0.clear(), tu.clear(), c0.clear(), cu.clear();
    for (size_t u = 0; u < frames.size(); ++u) {
        t0.push_back((int32_t)tu.size()), c0.push_back((int32_t)cu.size());
        for (int64_t r = 0; r < frames[u]; r += 64) tu.push_back((int32_t)u);
        for (int64_t r = 0; r < frames[u]; r += 4096) cu.push_back((int32_t)u);
    }
    t0.push_back((int32_t)tu.size()), c0.push_back((int32_t)cu.size());
}

int main()
{
    static_assert(mfx::kVadTileRows == 64 && mfx::kNormChunkRows == 4096, "the sizes k_vad_flags and k_vad_sums are written for");
    int n = 0;
    const int64_t edge[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8192, 8193, 360000};
    const int n_edge = (int)(sizeof(edge) / sizeof(edge[0]));
    for (int n_utt : {0, 1, 2, 15, 257, 5000}) {
        std::vector<int64_t> frames((size_t)n_utt);
        for (int u = 0; u < n_utt; ++u) frames[u] = n_utt <= 15 ? edge[(u * 7 + n_utt) % n_edge] : ((u * 37) % 11 == 0 ? 0 : (u * 131) % 9001);
        std::vector<int32_t> t0, tu, c0, cu;
        if (!mfx::build_utt_tiling(frames.data(), n_utt, mfx::kVadTileRows, t0, &tu)) return 1;
        if (!mfx::build_utt_tiling(frames.data(), n_utt, mfx::kNormChunkRows, c0, &cu)) return 1;
        {
            std::vector<int32_t> a, b, c, d;
            one_pass(frames, a, b, c, d);
            if (a != t0 || b != tu || c != c0 || d != cu) return 1;
        }
        if (t0.size() != (size_t)n_utt + 1 || c0.size() != (size_t)n_utt + 1 || t0[0] != 0 || c0[0] != 0) return 1;
        if (t0[n_utt] != (int32_t)tu.size() || c0[n_utt] != (int32_t)cu.size()) return 1;
        for (int u = 0; u < n_utt; ++u) {
            if (t0[u + 1] - t0[u] != (int32_t)((frames[u] + 63) / 64) || c0[u + 1] - c0[u] != (int32_t)((frames[u] + 4095) / 4096)) return 1;
            for (int32_t t = t0[u]; t < t0[u + 1]; ++t)
                if (tu[(size_t)t] != u) return 1;
            for (int32_t c = c0[u]; c < c0[u + 1]; ++c)
                if (cu[(size_t)c] != u) return 1;
        }
        ++n;
        if (n_utt > 0) { // a negative count is refused and nothing is written
            std::vector<int64_t> bad = frames;
            bad[(size_t)n_utt / 2] = -1;
            std::vector<int32_t> a(3, 7), b(2, 9), c(1, 5), d(4, 3);
            if (mfx::build_utt_tiling(bad.data(), n_utt, mfx::kVadTileRows, a, &b) || mfx::build_utt_tiling(bad.data(), n_utt, mfx::kNormChunkRows, c, &d)) return 1;
            if (a.size() != 3 || a[0] != 7 || b.size() != 2 || c.size() != 1 || d.size() != 4 || d[3] != 3) return 1;
        }
    }
    {   // more tiles than an int32 holds: refused before anything is sized
        std::vector<int64_t> huge(80, (int64_t)0x7fffffff);
        std::vector<int32_t> a, b, c, d;
        if (mfx::build_utt_tiling(huge.data(), 80, mfx::kVadTileRows, a, &b) || !a.empty() || !b.empty()) return 1;
        // (the chunks of that batch do fit: the VAD's refusal was always the tiles')
        if (!mfx::build_utt_tiling(huge.data(), 80, mfx::kNormChunkRows, c, &d) || c.size() != 81 || c[80] != (int32_t)d.size()) return 1;
    }
    std::printf("vad_asan: %d layouts clean\n", n);
    return 0;
}
