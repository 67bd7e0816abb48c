// Sanitizer run of the host side of mfx_batch_set_pitch_feats (csrc/mfx_tables.cpp) under -fsanitize=address,undefined: the
// tile layout k_pitch_feats walks (build_utt_tiling at kPitchFeatRows: the empty batch, frameless utterances, lengths on,
// before and after the tile edge; and that every tile's rows with the largest halo fit the kernel's LDS arrays), the limits
// (pitch_feat_shape) and the host restatement (host_pitch_feats: T = 0, 1, 2, windows longer than the utterance, the largest
// window and delta window, every column set, rho beyond +-1, output arrays of exactly T * F floats, every refusal with nothing
// written).  Built by `make -C csrc asan`.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../asr-featext-opencl_amd/csrc/mfx_tables.h"

static bool layouts(int &n)
{
    const int64_t edge[] = {0, 1, 2, 255, 256, 257, 511, 512, 513, 4097, 360000};
    const int n_edge = (int)(sizeof(edge) / sizeof(edge[0]));
    const int R = mfx::kPitchFeatRows;
    for (int n_utt : {0, 1, 2, 11, 257, 3000}) {
        std::vector<int64_t> frames((size_t)n_utt);
        for (int u = 0; u < n_utt; ++u) frames[u] = n_utt <= 11 ? edge[(u * 5 + n_utt) % n_edge] : ((u * 37) % 11 == 0 ? 0 : (u * 131) % 1901);
        std::vector<int32_t> t0, tu;
        if (!mfx::build_utt_tiling(frames.data(), n_utt, R, t0, &tu)) return false;
        if (t0.size() != (size_t)n_utt + 1 || t0[0] != 0 || t0[n_utt] != (int32_t)tu.size()) return false;
        for (int u = 0; u < n_utt; ++u) {
            if (t0[u + 1] - t0[u] != (int32_t)((frames[u] + R - 1) / R)) return false;
            for (int32_t t = t0[u]; t < t0[u + 1]; ++t) {
                if (tu[(size_t)t] != u) return false;
                // the rows a block stages, as the kernel cuts them, at the largest halo: inside the utterance and its arrays
                const int64_t T = frames[u], r0 = (int64_t)(t - t0[u]) * R, nr = std::min<int64_t>(R, T - r0);
                const int64_t lo = std::max<int64_t>(0, r0 - 1024), hi = std::min<int64_t>(T - 1, r0 + nr - 1 + 1024);
                if (nr < 1 || lo < 0 || hi >= T || hi - lo + 1 > R + 2048) return false;
            }
        }
        ++n;
    }
    return true;
}

static bool shapes()
{
    mfx::PitchFeatShape s;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    if (!mfx::pitch_feat_shape(0, 75, 75, 2, 2.f, 0.f, 2.f, 10.f, s) || s.columns != 7 || s.F != 3 || s.den != 10.0) return false;
    if (!mfx::pitch_feat_shape(15, 0, 1024, 16, -1.f, 1.f, 0.f, 1e30f, s) || s.F != 4 || s.den != 2992.0) return false;
    if (!mfx::pitch_feat_shape(8, 1024, 0, 1, 1.f, 1.f, 1.f, 1.f, s) || s.F != 1 || s.den != 2.0) return false;
    mfx::PitchFeatShape keep = s;
    if (mfx::pitch_feat_shape(16, 75, 75, 2, 2.f, 0.f, 2.f, 10.f, s) || mfx::pitch_feat_shape(-1, 75, 75, 2, 2.f, 0.f, 2.f, 10.f, s)) return false;
    if (mfx::pitch_feat_shape(0, -1, 75, 2, 2.f, 0.f, 2.f, 10.f, s) || mfx::pitch_feat_shape(0, 1025, 75, 2, 2.f, 0.f, 2.f, 10.f, s)) return false;
    if (mfx::pitch_feat_shape(0, 75, -1, 2, 2.f, 0.f, 2.f, 10.f, s) || mfx::pitch_feat_shape(0, 75, 1025, 2, 2.f, 0.f, 2.f, 10.f, s)) return false;
    if (mfx::pitch_feat_shape(0, 75, 75, 0, 2.f, 0.f, 2.f, 10.f, s) || mfx::pitch_feat_shape(0, 75, 75, 17, 2.f, 0.f, 2.f, 10.f, s)) return false;
    if (mfx::pitch_feat_shape(0, 75, 75, 2, inf, 0.f, 2.f, 10.f, s) || mfx::pitch_feat_shape(0, 75, 75, 2, 2.f, nan, 2.f, 10.f, s)) return false;
    if (mfx::pitch_feat_shape(0, 75, 75, 2, 2.f, 0.f, -inf, 10.f, s) || mfx::pitch_feat_shape(0, 75, 75, 2, 2.f, 0.f, 2.f, nan, s)) return false;
    return s.columns == keep.columns && s.F == keep.F && s.D == keep.D; // (a refusal writes nothing)
}

static bool restatement(int &n)
{
    for (int64_t T : {0, 1, 2, 3, 5, 76, 257, 600})
        for (int columns : {0, 1, 2, 4, 8, 15})
            for (int lr : {0, 1, 75, 1024})
                for (int D : {1, 2, 16}) {
                    std::vector<float> track((size_t)T * 2);
                    for (int64_t t = 0; t < T; ++t) {
                        track[(size_t)(2 * t)] = 40.f + (float)((t * 7) % 37) + 0.25f * (float)(t % 3);
                        track[(size_t)(2 * t + 1)] = -1.25f + 2.5f * (float)((t * 13) % 101) / 100.f; // (beyond +-1 at the ends)
                    }
                    const int F = columns == 0 ? 3 : __builtin_popcount((unsigned)columns);
                    std::vector<float> feats((size_t)T * F, 7.f); // (exactly T * F: one float more is a finding)
                    if (!mfx::host_pitch_feats(track.data(), T, 16000.f, columns, lr, lr / 2, D, 2.f, 0.f, 2.f, 10.f, feats.data())) return false;
                    for (float v : feats)
                        if (!std::isfinite(v)) return false;
                    ++n;
                }
    // a constant track: the delta column is exactly 0
    std::vector<float> flat(2 * 300), out(3 * 300);
    for (int t = 0; t < 300; ++t) flat[(size_t)(2 * t)] = 57.5f, flat[(size_t)(2 * t + 1)] = 0.1f * (float)(t % 10);
    if (!mfx::host_pitch_feats(flat.data(), 300, 16000.f, 0, 75, 75, 2, 2.f, 0.f, 2.f, 10.f, out.data())) return false;
    for (int t = 0; t < 300; ++t)
        if (out[(size_t)(3 * t + 2)] != 0.f) return false;
    // refusals: nothing is written
    float canary[8] = {5.f, 5.f, 5.f, 5.f, 5.f, 5.f, 5.f, 5.f};
    const float nan = std::numeric_limits<float>::quiet_NaN();
    auto refused = [&](int64_t T, float rate, int columns, int l, int r, int D, float s) {
        return !mfx::host_pitch_feats(flat.data(), T, rate, columns, l, r, D, s, 0.f, 2.f, 10.f, canary) && canary[0] == 5.f && canary[7] == 5.f;
    };
    if (!refused(-1, 16000.f, 0, 75, 75, 2, 2.f) || !refused(2, 0.f, 0, 75, 75, 2, 2.f) || !refused(2, nan, 0, 75, 75, 2, 2.f) ||
        !refused(2, 16000.f, 16, 75, 75, 2, 2.f) || !refused(2, 16000.f, 0, 1025, 75, 2, 2.f) || !refused(2, 16000.f, 0, 75, -1, 2, 2.f) ||
        !refused(2, 16000.f, 0, 75, 75, 17, 2.f) || !refused(2, 16000.f, 0, 75, 75, 0, 2.f) || !refused(2, 16000.f, 0, 75, 75, 2, nan))
        return false;
    if (mfx::host_pitch_feats(nullptr, 2, 16000.f, 0, 75, 75, 2, 2.f, 0.f, 2.f, 10.f, canary)) return false; // (rows without an array)
    if (mfx::host_pitch_feats(flat.data(), 2, 16000.f, 0, 75, 75, 2, 2.f, 0.f, 2.f, 10.f, nullptr)) return false;
    return mfx::host_pitch_feats(nullptr, 0, 16000.f, 0, 75, 75, 2, 2.f, 0.f, 2.f, 10.f, nullptr); // (T = 0 touches nothing)
}

int main()
{
    int n_layouts = 0, n_runs = 0;
    if (!layouts(n_layouts)) return std::printf("pitchfeat_asan: layout FAILED\n"), 1;
    if (!shapes()) return std::printf("pitchfeat_asan: limits FAILED\n"), 1;
    if (!restatement(n_runs)) return std::printf("pitchfeat_asan: restatement FAILED\n"), 1;
    std::printf("pitchfeat_asan: %d layouts, %d runs, pitch features clean\n", n_layouts, n_runs);
    return 0;
}
