// mfx_launch.h -- launch-side helpers shared by the kernel translation units (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>

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

constexpr int kGridYMax = 65535;          // blocks a launch may have along grid.y (and tables along it)
constexpr size_t kLdsMax = 160 * 1024;    // LDS a block may ask for on gfx950
constexpr size_t kTileLdsTarget = 40 * 1024; // tile kernels: four blocks (16 waves) per CU where the shape allows

// a kernel whose only argument is the parameter struct `q`, through its address (the instantiation is picked once)
template <class P>
inline hipError_t launch_kernel(const void *fn, dim3 grid, dim3 block, size_t lds, hipStream_t stream, P &q)
{
    void *args[] = {&q};
    return hipLaunchKernel(fn, grid, block, args, lds, stream);
}

// grid.y is limited to kGridYMax: f(s0, count) for consecutive slices of a list of n segments, until one fails.  What a
// kernel indexes with blockIdx.y (segments, their statistics, ...) is moved up by s0 in f.
template <class F>
inline hipError_t for_seg_slices(int n, F &&f)
{
    for (int s0 = 0; s0 < n; s0 += kGridYMax)
        if (hipError_t e = f(s0, n - s0 < kGridYMax ? n - s0 : kGridYMax); e != hipSuccess) return e;
    return hipSuccess;
}

// the magnitude rows a wave-per-row-group kernel stages: whole 16-byte words, a wave buffer that holds a row
inline bool spec_rows_ok(int mag_floats, int spec_pitch) { return mag_floats >= spec_pitch && !(spec_pitch & 3) && !(mag_floats & 3); }

// Grid of a wave-per-row-group kernel (k_melcep, k_plp and their row-run forms) whose blocks stay resident and walk
// `groups` row groups: as many of 4 waves per block as the LDS holds (lds_of(waves) bytes), as many blocks as are resident at
// once (at most 8 per CU) -- shared among the `active` tables that have rows (1 for the plain forms; the others' blocks leave
// at once) -- and no more than there are groups.
struct ResidentGrid {
    int waves;
    size_t lds;
    unsigned blocks;
};
template <class LdsOf>
inline hipError_t resident_grid(const void *fn, LdsOf lds_of, int64_t groups, int active, ResidentGrid &g)
{
    g.waves = 4;
    while (g.waves > 1 && lds_of(g.waves) > kLdsMax) g.waves >>= 1;
    g.lds = lds_of(g.waves);
    if (g.lds > kLdsMax) return hipErrorInvalidValue;
    if (hipError_t e = allow_dynamic_lds(fn, g.lds); e != hipSuccess) return e;
    // (registers allow 6 blocks of 4 waves; see launch_front_generic.  Cached per device and launch shape)
    int per_cu = blocks_per_cu(fn, 64 * g.waves, g.lds, (int)(kLdsMax / g.lds < 4 ? kLdsMax / g.lds : 4));
    if (per_cu > 8) per_cu = 8;
    const int64_t cap = (num_cus() * (per_cu < 1 ? 1 : per_cu) + active - 1) / active;
    const int64_t blocks = (groups + g.waves - 1) / g.waves;
    g.blocks = (unsigned)(blocks < cap ? blocks : cap);
    return hipSuccess;
}

// Rows per block of a tile kernel (k_traps, k_splice_affine): the largest of 64 / 32 / 16 whose LDS (lds_of(rows) bytes) stays
// under `target`, else the largest that fits at all; 0 when none does.
template <class LdsOf>
inline int tile_rows_for(LdsOf lds_of, size_t target)
{
    for (size_t limit : {target, kLdsMax})
        for (int r : {64, 32, 16})
            if (lds_of(r) <= limit) return r;
    return 0;
}

} // namespace mfx
