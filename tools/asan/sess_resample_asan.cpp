// sess_resample_asan.cpp -- the session converter's host arithmetic (mfx_tables.cpp: session_resample_step over resample_shape)
// under AddressSanitizer + UBSan, CPU only (`make asan` in asr-featext-opencl_amd/csrc builds and runs it).  Random cuts of
// streams at the six rates of the tests: the converted counts follow the delivery rule and add up to ceil(N L / M), the carry a
// push leaves is the carry the next one takes and stays inside the slot (2 Wh + M div L + 2), every tap of every output a push
// converts lies in [c0_old, N_new) or outside the stream, and a final push leaves {0, 0}.
#include <cstdint>
#include <cstdio>
#include <random>

#include "../../asr-featext-opencl_amd/csrc/mfx_tables.h"

int main()
{
    int nq = 0;
    std::mt19937 rng(20260);
    for (int in_hz : {48000, 8000, 44100, 11025, 17600, 12345}) {
        mfx::ResampleShape sh;
        if (mfx::resample_shape(in_hz, 16000, 0, 0.f, sh) != 0) return 1;
        const int64_t L = sh.L, M = sh.M, Wh = sh.Wh;
        const int cap = (int)(2 * Wh + M / L + 2);
        for (int trial = 0; trial < 200; ++trial) {
            int64_t left = trial == 0 ? 0 : (int64_t)(rng() % (unsigned)(8 * Wh + 4000));
            const int64_t total = left;
            const bool flush = trial % 2 == 0;
            int64_t N = 0, J = 0, sum = 0;
            int32_t carry = 0;
            for (;;) {
                const unsigned k = rng() % 8;
                int64_t len = k == 0 ? 0 : k == 1 ? 1 : k == 2 ? Wh - 1 : k == 3 ? Wh : (int64_t)(rng() % (unsigned)(3 * Wh + 500));
                if (len > left) len = left;
                left -= len;
                const bool fin = left == 0 && (!flush || len == 0);
                const int64_t N_old = N, J_old = J;
                mfx::SessionResampleStep st;
                const int64_t n_out = mfx::session_resample_step(sh.L, sh.M, sh.Wh, N, J, len, fin, st);
                const int64_t N_new = N_old + len;
                const int64_t want = fin ? (N_new * L + M - 1) / M : N_new > Wh ? ((N_new - Wh) * L + M - 1) / M : 0;
                if (n_out < 0 || n_out != want - J_old) return 1;
                if (st.carry_in != carry || st.carry_out < 0 || st.carry_out > cap || st.c0_old + st.carry_in != N_old) return 1;
                if (st.c0_new + st.carry_out != N_new || st.c0_new < st.c0_old) return 1;
                for (int64_t j = J_old; j < want; ++j) { // every tap inside what the push holds, or outside the stream
                    const int64_t n = (j * M) / L;
                    if (n - Wh + 1 < st.c0_old && n - Wh + 1 >= 0) return 1;
                    if (!fin && n + Wh > N_new - 1) return 1;
                }
                if (fin ? (N != 0 || J != 0 || st.carry_out != 0) : (N != N_new || J != want)) return 1;
                sum += n_out, carry = st.carry_out;
                if (fin) break;
            }
            if (sum != (total * L + M - 1) / M) return 1;
            ++nq;
        }
    }
    // a pass-through rate: every sample at once, nothing carried
    int64_t N = 0, J = 0;
    mfx::SessionResampleStep st;
    if (mfx::session_resample_step(1, 1, 0, N, J, 7, false, st) != 7 || st.carry_out != 0 || N != 7 || J != 7) return 1;
    if (mfx::session_resample_step(1, 1, 0, N, J, 0, true, st) != 0 || st.carry_in != 0 || N != 0 || J != 0) return 1;
    std::printf("sess_resample_asan: %d streams clean\n", nq);
    return 0;
}
