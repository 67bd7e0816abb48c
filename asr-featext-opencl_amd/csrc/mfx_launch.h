// mfx_launch.h -- launch-side helpers shared by the kernel translation units (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mfx {

// Row-run forms (RowRuns, mfx_kernels.h) from the host's copies of the lists: the largest number of groups of `group_rows`
// rows any of the n_tables tables has inside the window [row0, row0 + rows) -- counted as the kernels count them, per
// clipped run -- and in `active` the number of tables that have any.  Sizes the grid; O(runs), nothing allocated.
inline int64_t run_groups_in_window(const int32_t *off, const int64_t *runs, int n_tables, int64_t row0, int64_t rows, int group_rows,
                                    int &active)
{
    const int64_t w0 = row0, w1 = row0 + rows;
    int64_t most = 0;
    active = 0;
    for (int a = 0; a < n_tables; ++a) {
        int64_t g = 0;
        for (int32_t r = off[a]; r < off[a + 1]; ++r) {
            const int64_t lo = runs[2 * r] > w0 ? runs[2 * r] : w0;
            const int64_t hi = runs[2 * r] + runs[2 * r + 1] < w1 ? runs[2 * r] + runs[2 * r + 1] : w1;
            if (hi > lo) g += (hi - lo + group_rows - 1) / group_rows;
        }
        if (g > 0) ++active;
        if (g > most) most = g;
    }
    return most;
}

// compute units of the CURRENT device (cached per device: one thread may drive handles on several GPUs -- afet_hip --devs,
// multi-rank setups)
int num_cus();
// hipOccupancyMaxActiveBlocksPerMultiprocessor cached per (device, function, threads, LDS bytes); `fallback` when the query fails
int blocks_per_cu(const void *func, int threads, size_t lds_bytes, int fallback);

// a kernel launched with more than 64 KB of dynamic LDS must be told so once (hipFuncAttributeMaxDynamicSharedMemorySize); the
// largest size granted is remembered per (device, function), so that the per-launch cost is a table lookup
hipError_t allow_dynamic_lds(const void *func, size_t lds_bytes);

} // namespace mfx
