// Sanitizer run of the host restatement of the online normaliser (csrc/mfx_tables.cpp: host_online_norm) under
// -fsanitize=address,undefined: stream lengths on, before and after the 32-row chunk and the window edges, both kinds, with and
// without a prior, a pitch wider than the columns with the input cut off right behind its last value, and the refusals,
// which must write nothing.  A constant column must come out as exact zeros (CVN: d <= 0 leaves the multiplier at 1).  Built by `make -C csrc asan`.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../asr-featext-opencl_amd/csrc/mfx_tables.h"

int main()
{
    int n = 0;
    const int Wn = 5;
    const double prior[2 * Wn] = {600.0, -30.0, 0.5, 725.0, 1e5, 4e4, 900.0, 3.0, 5256.25, 1e8};
    for (int64_t T : {0, 1, 31, 32, 33, 95, 96, 97, 133, 199, 4097})
        for (int pitch : {Wn, Wn + 3})
            for (int window : {0, 32, 96, 4096})
                for (int kind : {1, 2})
                    for (int p : {0, 100}) {
                        // exactly the floats the entry may read: nothing behind the last row's Wn columns
                        std::vector<float> rows(T > 0 ? (size_t)((T - 1) * pitch + Wn) : 0);
                        uint32_t s = 12345u + (uint32_t)T;
                        for (size_t i = 0; i < rows.size(); ++i) {
                            s = s * 1664525u + 1013904223u;
                            const int c = (int)(i % (size_t)pitch);
                            rows[i] = c == 3 ? 7.25f : (float)((int)(s >> 20) - 2048) * 0.01f + (c == 4 ? 1000.0f : 0.0f);
                        }
                        std::vector<float> out((size_t)T * Wn, -1.0f);
                        if (!mfx::host_online_norm(rows.data(), T, pitch, Wn, kind, window, p ? 64 : 0, p, p ? prior : nullptr, out.data())) return 1;
                        for (int64_t t = 0; t < T; ++t) // (the constant column, whose prior has the same mean: float32 mean 7.25, exact 0)
                            if (out[(size_t)t * Wn + 3] != 0.0f) return 1;
                        ++n;
                    }
    {   // refusals: nothing is written
        std::vector<float> rows(40 * Wn, 1.0f), out(40 * Wn, 7.0f);
        const bool any = mfx::host_online_norm(rows.data(), 40, Wn, Wn, 3, 32, 0, 0, nullptr, out.data()) ||
                         mfx::host_online_norm(rows.data(), 40, Wn, Wn, 1, 48, 0, 0, nullptr, out.data()) ||
                         mfx::host_online_norm(rows.data(), 40, Wn - 1, Wn, 1, 32, 0, 0, nullptr, out.data()) ||
                         mfx::host_online_norm(rows.data(), 40, Wn, Wn, 1, 32, 64, 5, nullptr, out.data()) ||
                         mfx::host_online_norm(rows.data(), 40, Wn, Wn, 1, 32, 64, 0, prior, out.data()) ||
                         mfx::host_online_norm(rows.data(), -1, Wn, Wn, 1, 32, 0, 0, nullptr, out.data());
        if (any) return 1;
        for (float v : out)
            if (v != 7.0f) return 1;
    }
    std::printf("onorm_asan: %d streams clean\n", n);
    return 0;
}
