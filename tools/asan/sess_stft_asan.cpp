// sess_stft_asan.cpp -- the host arithmetic of the session entries on an STFT log-mel handle (mfx_tables.cpp: session_stft_step,
// cut_sess_stft_groups) under AddressSanitizer + UBSan, CPU only (`make asan` in asr-featext-opencl_amd/csrc builds and runs
// it).  Every stream length up to 3 N + 5 S, cut in several ways, through the planner's step: E follows the delivery rule
// restated by brute force, never decreases and ends at the frame count; the carried samples stay below N + S; a flush delivers
// at most N / (2 S) + 1 rows and any push at most session_stft_rows_max; every tap a delivered frame reads -- reflected at the
// start and, on a final push, at the end of the stream -- lies among the samples the slot holds.  The cutter's groups cover
// every delivered row once, in order.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../asr-featext-opencl_amd/csrc/mfx_tables.h"

namespace {

// rows an OPEN stream of n samples has delivered, from the definition: frame t counts when its last tap t S + N / 2 - 1 has
// arrived, sample N / 2 (frame 0's left reflection) has, and every longer stream keeps it (T is non-decreasing past N / 2)
int64_t open_rows(int N, int S, int64_t n)
{
    if (n <= N / 2) return 0;
    int64_t E = 0;
    while ((E * S + N / 2 - 1) <= n - 1 && E < n / S) ++E;
    return E;
}

uint32_t rnd(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

} // namespace

int main()
{
    const int shapes[][2] = {{400, 160}, {512, 512}, {32, 1}, {512, 1}, {400, 400}, {400, 199}, {400, 201}, {64, 24}, {32, 17}, {34, 33}};
    int64_t pushes = 0;
    uint32_t seed = 12345;
    for (const auto &sh : shapes) {
        const int N = sh[0], S = sh[1];
        for (int64_t total = 0; total <= 3 * N + 5 * S; ++total) {
            for (int mode = 0; mode < 4; ++mode) { // whole; single samples; random cuts with empty pushes; a flush at the end
                if (mode == 1 && total > N + 2 * S) continue; // (one sample per push: the short streams)
                int64_t n = 0, E = 0, left = total, rows = 0;
                while (true) {
                    int64_t len = mode == 0 ? left : mode == 1 ? (left > 0 ? 1 : 0) : (int64_t)(rnd(seed) >> 8) % (2 * S + 3);
                    if (mode >= 2 && (rnd(seed) >> 20) % 5 == 0) len = (rnd(seed) >> 9) & 1;
                    if (len > left) len = left;
                    left -= len;
                    const bool fin = left == 0 && (mode != 3 || len == 0);
                    const int64_t n_old = n, E_old = E;
                    mfx::SessionStftStep st;
                    const int32_t k = mfx::session_stft_step(N, S, n, E, len, fin, st);
                    ++pushes;
                    const int64_t n_new = n_old + len, E_new = E_old + k;
                    const int64_t T = mfx::stft_frame_count(n_new, N, S);
                    if (k < 0 || E_new > T || E_new != (fin ? T : open_rows(N, S, n_new))) return 1;
                    if (fin ? (n != 0 || E != 0) : (n != n_new || E != E_new)) return 1;
                    if (st.carry_in < 0 || st.carry_in >= N + S || st.carry_out < 0 || st.carry_out >= N + S) return 2;
                    if (st.c0_old + st.carry_in != n_old || (fin ? st.carry_out != 0 : st.c0_new + st.carry_out != n_new)) return 2;
                    if (st.c0_new < st.c0_old) return 2;
                    if (k > mfx::session_stft_rows_max(N, S, len) || (len == 0 && k > N / (2 * S) + 1)) return 3;
                    for (int64_t t = E_old; t < E_new; ++t)
                        for (int c = 0; c < 3; ++c) { // (the reflections are monotone: the first tap, the last, the one at sample 0)
                            const int64_t j0 = N / 2 - t * S;
                            const int64_t j = c == 0 ? 0 : c == 1 ? N - 1 : (j0 > 0 && j0 < N ? j0 : 0);
                            int64_t i = t * S + j - N / 2;
                            if (i < 0) i = -i;
                            if (i >= n_new) {
                                if (!fin) return 4; // (an open stream never reflects at its end)
                                i = 2 * (n_new - 1) - i;
                            }
                            if (i < st.c0_old || i >= n_new) return 4; // (outside the samples the slot holds)
                        }
                    rows += k;
                    if (fin) break;
                }
                if (rows != mfx::stft_frame_count(total, N, S)) return 5;
            }
        }
    }
    int lists = 0;
    for (int n : {0, 1, 5, 13, 1000}) {
        std::vector<int32_t> n_out(n);
        std::vector<mfx::SessStftCut> cuts;
        for (int i = 0; i < n; ++i) n_out[i] = (i * 7) % 41 == 3 ? 0 : (i * 13) % 50;
        mfx::cut_sess_stft_groups(n_out.data(), n, cuts);
        std::vector<int32_t> seen(n, 0);
        int last = -1;
        for (const mfx::SessStftCut &g : cuts) {
            if (g.piece < last || g.rows < 1 || g.rows > 16 || g.r0 != seen[g.piece]) return 6;
            seen[g.piece] += g.rows, last = g.piece;
        }
        for (int i = 0; i < n; ++i)
            if (seen[i] != n_out[i]) return 6;
        ++lists;
    }
    std::printf("sess_stft_asan: %lld pushes, %d work lists clean\n", (long long)pushes, lists);
    return 0;
}
