// Sanitizer run of the host planner of mfx_batch_set_speakers (csrc/mfx_tables.cpp: build_speaker_lists) under
// -fsanitize=address,undefined: interleaved ids, speakers without utterances, frameless utterances, ids outside the range,
// the empty batch, many speakers.  Every utterance with frames must come out exactly once, under its own speaker, ascending.
// And the chunk0 list of k_spk_sums (build_utt_tiling at kNormChunkRows without item_utt): lengths on, before and after the
// chunk edge.
// Built by `make -C csrc asan`.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../asr-featext-opencl_amd/csrc/mfx_tables.h"

int main()
{
    int n = 0;
    for (int n_utt : {0, 1, 12, 257, 5000})
        for (int n_spk : {1, 2, 3, 100, 5000, 1 << 20}) {
            std::vector<int32_t> ids((size_t)n_utt);
            std::vector<int64_t> frames((size_t)n_utt);
            int64_t with_frames = 0;
            for (int u = 0; u < n_utt; ++u) {
                ids[u] = (int32_t)(((int64_t)u * 7919) % n_spk);
                frames[u] = (u * 37) % 11 == 0 ? 0 : (u * 131) % 9001; // (frameless ones among them; some past 4096 and 8192 rows)
                with_frames += frames[u] > 0;
            }
            std::vector<int32_t> off, list;
            if (!mfx::build_speaker_lists(ids.data(), frames.data(), n_utt, n_spk, off, list)) return 1;
            if (off.size() != (size_t)n_spk + 1 || off[0] != 0 || off.back() != (int32_t)list.size() || (int64_t)list.size() != with_frames)
                return 1;
            std::vector<char> seen((size_t)n_utt, 0);
            for (int s = 0; s < n_spk; ++s) {
                if (off[s + 1] < off[s]) return 1;
                for (int32_t k = off[s]; k < off[s + 1]; ++k) {
                    const int32_t u = list[k];
                    if (u < 0 || u >= n_utt || ids[u] != s || frames[u] <= 0 || seen[u]) return 1;
                    if (k > off[s] && list[k - 1] >= u) return 1;
                    seen[u] = 1;
                }
            }
            ++n;
            if (n_utt > 0) { // an id outside the range is refused and nothing is written
                std::vector<int32_t> bad = ids;
                bad[(size_t)n_utt / 2] = n_spk;
                std::vector<int32_t> o2(3, 7), l2(2, 9);
                if (mfx::build_speaker_lists(bad.data(), frames.data(), n_utt, n_spk, o2, l2)) return 1;
                bad[(size_t)n_utt / 2] = -1;
                if (mfx::build_speaker_lists(bad.data(), frames.data(), n_utt, n_spk, o2, l2)) return 1;
                if (o2.size() != 3 || o2[0] != 7 || l2.size() != 2 || l2[1] != 9) return 1;
            }
        }
    {   // chunk0: utterance u owns chunks [chunk0[u], chunk0[u + 1]) of kNormChunkRows rows; no item_utt is asked for
        const std::vector<int64_t> frames = {0, 1, 4096, 4097, 8200};
        const std::vector<int32_t> want = {0, 0, 1, 2, 4, 7};
        std::vector<int32_t> chunk0;
        if (!mfx::build_utt_tiling(frames.data(), (int)frames.size(), mfx::kNormChunkRows, chunk0, nullptr) || chunk0 != want) return 1;
        std::vector<int64_t> bad = frames;
        bad[2] = -1; // (refused, nothing written)
        if (mfx::build_utt_tiling(bad.data(), (int)bad.size(), mfx::kNormChunkRows, chunk0, nullptr) || chunk0 != want) return 1;
        ++n;
    }
    std::printf("speakers_asan: %d speaker lists clean\n", n);
    return 0;
}
