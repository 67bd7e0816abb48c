// mfx_tail.hip -- everything behind the front end, and their launchers:
//   k_melcep      stored magnitudes -> mel -> log -> DCT (streaming apply(), VTLN sweeps, the 4096-point batch path)
//   k_delta16 / k_delta4 / k_delta   delta + delta-delta (deltacpu.cpp:16-29, mfcccpu.cpp:234-263), whole output rows
//   k_norm_seg / k_norm_stats / k_norm_finalize / k_norm_apply   CMN / CVN / MINMAX (normalizercpu.cpp:22-89)
//   k_copy_small  small streaming blocks through pinned memory
// See DESIGN.md section 5.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_dev.h"
#include "mfx_launch.h"

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <vector>
#include "mfx_delta_dev.h"
#include "mfx_norm_dev.h"
#include "mfx_tile_dev.h"

// build knobs: output rows per tile of the wide-row delta kernels (less LDS per block: more blocks per CU in flight)
#ifndef MFX_DELTA_WIDE_ROWS
#define MFX_DELTA_WIDE_ROWS 32   // k_delta<false, .> (C5: k_delta 0.072 -> 0.055 ms; 16 rows: 0.063)
#endif
#ifndef MFX_DELTA_WIDE_ROWS_V
#define MFX_DELTA_WIDE_ROWS_V 32 // k_delta4
#endif

namespace mfx {

namespace {

// ------------------------------------------------------------------------------------------------
// melcep: stored magnitudes -> mel -> log -> DCT (streaming apply(), VTLN sweeps, the 4096-point batch path).  A wave
// takes 4 consecutive rows at a time: each row's magnitudes go to the wave's LDS buffer, its filters are walked on the
// wave's 64 lanes (MelPlan: whole filters in ascending bin order, mfcccpu.cpp:206-217), the log energies wait in
// lm[4][FS], and the DCT of the four rows runs on the matrix pipe (dct_mfma4) -- the same mel stage as the fused batch
// kernels (round 3: the round-1 piece plan and its vector-pipe DCT are gone).  blockIdx.y = filterbank of a VTLN sweep.
// melcep_rows is the kernel's body over the row groups `groups(first, stride)` deals to this wave: all rows [0, n_rows) in
// k_melcep, the table's row runs in k_melcep_runs.  (n_threads: blockDim.x, read once in the kernel -- read inside the
// body it became a vector load in front of the staging.)
// ------------------------------------------------------------------------------------------------
template <class MakeGroups>
__device__ __forceinline__ void melcep_rows(const MelcepParams &p, int table, float *feat, unsigned n_threads, MakeGroups groups)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n_waves = n_threads >> 6;
    const int nb = p.num_banks, RS = p.mel.row_stride, rounds = p.mel.rounds;
    const int FS = lm_fs4(nb), MF = p.mag_floats;
    const int WR = mel64_rows(nb);
    MelPlanLds plan;
    float *s_wave = stage_mel_plan(smem, p.mel, nb, table, tid, n_threads, plan) + wave * (MF + 4 * FS);
    float *mag = s_wave, *lm = s_wave + MF;
    for (int i = lane; i < MF + 4 * FS; i += 64) s_wave[i] = 0.f; // words past the last bin stay zero (finite) for good
    __syncthreads();

    const int dct_ks = p.dct_ksteps, dct_tiles64 = (p.dct_len + 63) >> 6;
    const int dct_bytes = p.dct_b4 ? dct_tiles64 * dct_ks * 1024 : 0;
    const __amdgpu_buffer_rsrc_t dct_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)p.dct_b4, 0, dct_bytes, 0x00020000);
    const int q4 = p.spec_pitch >> 2; // rows are whole 16-byte words (spec_pitch is a multiple of 4, rows 16-byte aligned)
    const int nbins = (p.fft_size >> 1) + 1;
    for (auto it = groups((int64_t)blockIdx.x * n_waves + wave, (int64_t)gridDim.x * n_waves); it.valid(); it.advance()) {
        const int64_t row0 = it.row0;
        const int count = it.count;
        for (int f = 0; f < count; ++f) {
            const float4 *src = (const float4 *)(p.spec + (row0 + f) * p.spec_pitch);
            for (int k = lane; k < q4; k += 64) ((float4 *)mag)[k] = src[k];
            // the row's padding words (bins > W2/2) are never written in memory: they meet zero weights in the walk and
            // must be finite (0 x NaN is NaN)
            if (nbins + lane < 4 * q4) mag[nbins + lane] = 0.f;
            wave_sync();
            mel64_walk_log(mag, lm + f * FS, FS - 1, plan.s_mw, plan.s_mst, plan.s_mfid, plan.s_L, rounds, RS, lane, WR);
            wave_sync();
        }
        dct4_store<3>(lm, FS, dct_rsrc, dct_bytes, dct_ks, dct_tiles64, p.dct_b4 != nullptr, lane, p.cols, feat, (int64_t)p.feat_pitch,
                   row0, count);
        wave_sync();
    }
}

__global__ void __launch_bounds__(256) k_melcep(MelcepParams p)
{
    const int table = blockIdx.y;
    melcep_rows(p, table, p.feat + (int64_t)table * p.feat_table_stride, blockDim.x,
                [&](int64_t first, int64_t stride) { return PlainGroups<4>(p.n_rows, first, stride); });
}

// k_melcep_runs (per-utterance warp factors of the batch entries): blockIdx.y is still the table, staged in LDS exactly as
// in k_melcep, but instead of all rows [0, n_rows) the block walks that table's row runs (RowRuns), each clipped to the
// slab's window.  The groups of 4 rows of the table's clipped runs are numbered through in run order and dealt to the
// waves of the grid's blockIdx.y plane (RunGroups, mfx_dev.h): a group starts at a clipped run's first row + 4 k and never
// spans two runs, only a run's last group is short.  spec and feat address absolute rows (one output).
__global__ void __launch_bounds__(256) k_melcep_runs(MelcepParams p, RowRuns rr)
{
    const int table = blockIdx.y;
    int run0, run1; // the table's runs that reach into the window (none: nothing to stage; uniform over the block)
    if (!runs_in_window(rr, table, run0, run1)) return;
    melcep_rows(p, table, p.feat, blockDim.x, [&](int64_t first, int64_t stride) { return RunGroups<4>(rr, run0, run1, first, stride); });
}

// ------------------------------------------------------------------------------------------------
// delta: regression coefficients over time (deltacpu.cpp:16-29) with the edge handling of
// MfccCpu::do_delta (mfcccpu.cpp:234-263) expressed as a clamped row accessor (Segment).
// grid = (tiles, segments); one tile = ROWS output rows.  The tile itself is delta_tile (mfx_tile_dev.h), typed for
// float here (FAST16: cols <= 16) and for float4 in k_delta4.
// ------------------------------------------------------------------------------------------------
template <bool FAST16, int ROWS>
__global__ void __launch_bounds__(256) k_delta(DeltaParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    delta_tile<float, FAST16, ROWS>(p, smem);
}

// The same stage for wide rows whose column count is a multiple of 4 (BASELINE configs[4]: 40 columns, 120-float rows): a
// work item is 4 consecutive columns, every load / LDS access / store a 16-byte word -- a quarter of k_delta's memory
// instructions and no per-element index arithmetic.  Same arithmetic per element as k_delta (delta_quot), same tile shape;
// requires cols % 4 == 0, src_pitch % 4 == 0, out_pitch == cols * groups, 16-byte aligned src / out.
template <int ROWS>
__global__ void __launch_bounds__(256) k_delta4(DeltaParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    delta_tile<float4, false, ROWS>(p, (float4 *)smem);
}

// Delta stage from the compact statics (pitch 16) to whole output rows: the tile function of the fused
// delta wave run by a block.  grid = (tiles, segments) as k_delta; requires cols <= 16, l1 > 0,
// out_pitch == cols * (l2 > 0 ? 3 : 2), src_pitch == 16 and a 16-byte aligned `out`.
constexpr int kDelta16TilesPerBlock = 2;

template <int L1, int L2>
__global__ void __launch_bounds__(256, 7) k_delta16(DeltaParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Segment sg = p.inline_seg ? p.seg0 : p.segs[blockIdx.y];
    int r0 = blockIdx.x * (kDelta16TilesPerBlock * kDeltaRows);
    if (r0 >= sg.n_out) return;
    // a block walks 2 consecutive tiles (measured on C2: 1 -> 62 us, 2 -> 59 us, 4 -> 62 us, 8 -> 71 us per launch); the
    // statics of the second are in flight while the first is computed
    DeltaFill<256> fill;
    fill.issue(sg, r0, min(kDeltaRows, sg.n_out - r0), p.l1 + p.l2, p.src, threadIdx.x);
#pragma unroll 1
    for (int t = 0; t < kDelta16TilesPerBlock && r0 < sg.n_out; ++t, r0 += kDeltaRows) {
        const int rows = min(kDeltaRows, sg.n_out - r0);
        const int nr0 = r0 + kDeltaRows;
        const int nrows = (t + 1 < kDelta16TilesPerBlock && nr0 < sg.n_out) ? min(kDeltaRows, sg.n_out - nr0) : 0;
        delta_tile16<L1, L2, 256>(sg, r0, rows, p.src, p.out, p.out_pitch, p.cols, p.l1, p.l2, smem, threadIdx.x, fill, nr0,
                                  nrows);
    }
}

// ------------------------------------------------------------------------------------------------
// normalisation (normalizercpu.cpp:22-89): per segment, per column statistics in double.
// stats layout [seg][2][cols]: mean, multiplier.
//
// k_norm_stats: one block per (row chunk, segment).  The block reads its rows as they lie in memory: a thread is
// (row rr of the pass, column c), consecutive threads read consecutive floats of a row, a pass covers 256 / Cp
// whole rows (Cp = columns rounded up to a power of two).  Sums in double as the reference's (sum2 takes the
// float product v * v, normalizercpu.cpp:44); the partial results of the passes' rows are combined through LDS
// in a fixed order.  A segment longer than kNormChunkRows rows is cut into chunks whose partial results go to
// a scratch array and are combined, again in a fixed order, by k_norm_finalize -- results do not depend on timing.
// Statistics cover the first `stat_rows` rows of the segment (Segment::pad; 0 = all n_out rows): the reference
// computes them over the block it delivers and re-uses them for the flush rows (mfcccpu.cpp:377-388).
// ------------------------------------------------------------------------------------------------
constexpr size_t kNormSegLdsBytes = 54 * 1024; // k_norm_seg: dynamic LDS per block (1024 rows of 13 columns: a 10 s utterance; two blocks per CU)

// (norm_finish_to and the summation itself, norm_rows_totals: mfx_norm_dev.h, shared with mfx_speakers.hip; kNormChunkRows:
// mfx_tables.h, shared with the host that lays the speakers' and the VAD's chunks out)
__device__ __forceinline__ void norm_finish(const NormParams &p, int seg, int c, int n, double S, double S2, float mn, float mx)
{
    norm_finish_to(p.stats + (int64_t)seg * 2 * p.cols, p.cols, p.norm_type, c, n, S, S2, mn, mx);
}

__global__ void __launch_bounds__(256) k_norm_stats(NormParams p)
{
    __shared__ double s_sum[256], s_sum2[256];
    __shared__ float s_min[256], s_max[256];
    const Segment sg = p.inline_seg ? p.seg0 : p.segs[blockIdx.y];
    const int n = sg.pad > 0 ? sg.pad : sg.n_out;
    const int r0 = blockIdx.x * kNormChunkRows;
    if (r0 >= n && blockIdx.x > 0) return;
    const int r1 = min(n, r0 + kNormChunkRows);
    const int lg = norm_lg(p.cols);                   // 2^lg threads per row of threads, 256 >> lg rows per pass (cols <= 256)
    const int tid = threadIdx.x, rr = tid >> lg, c = tid & ((1 << lg) - 1);
    const float *base = p.data + (sg.out_row0 + p.row_off) * (int64_t)p.pitch + p.col0;
    norm_rows_totals<false>([&](int r, int cc) { return base[(int64_t)r * p.pitch + cc]; }, r0, r1, p.cols, lg, tid, s_sum, s_sum2, s_min,
                            s_max);
    if (rr == 0 && c < p.cols) {
        if (p.chunks <= 1) {
            norm_finish(p, blockIdx.y, c, n, s_sum[tid], s_sum2[tid], s_min[tid], s_max[tid]);
        } else {
            double *q = p.partial + ((int64_t)blockIdx.y * p.chunks + blockIdx.x) * 4 * p.cols;
            q[c] = s_sum[tid];
            q[p.cols + c] = s_sum2[tid];
            q[2 * p.cols + c] = (double)s_min[tid];
            q[3 * p.cols + c] = (double)s_max[tid];
        }
    }
}

// chunks > 1: combine the chunk results of a segment in ascending chunk order
__global__ void __launch_bounds__(256) k_norm_finalize(NormParams p)
{
    const Segment sg = p.inline_seg ? p.seg0 : p.segs[blockIdx.x];
    const int n = sg.pad > 0 ? sg.pad : sg.n_out;
    const int used = (n + kNormChunkRows - 1) / kNormChunkRows;
    for (int c = threadIdx.x; c < p.cols; c += 256) {
        double S = 0, S2 = 0;
        float mn = 3.402823466e+38f, mx = -3.402823466e+38f;
        for (int k = 0; k < used; ++k) {
            const double *q = p.partial + ((int64_t)blockIdx.x * p.chunks + k) * 4 * p.cols;
            S += q[c];
            S2 += q[p.cols + c];
            mn = fminf(mn, (float)q[2 * p.cols + c]);
            mx = fmaxf(mx, (float)q[3 * p.cols + c]);
        }
        norm_finish(p, blockIdx.x, c, n, S, S2, mn, mx);
    }
}

// (x - mean) [* multiplier] in place over all n_out rows of the segment; grid.x is sized from the row count
__global__ void __launch_bounds__(256) k_norm_apply(NormParams p)
{
    const Segment sg = p.inline_seg ? p.seg0 : p.segs[blockIdx.y];
    const int cols = p.cols;
    const int64_t total = (int64_t)sg.n_out * cols;
    const float *st = p.stats + (int64_t)blockIdx.y * 2 * cols;
    float *base = p.data + (sg.out_row0 + p.row_off) * (int64_t)p.pitch + p.col0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cols;
        const int c = (int)(i - r * cols);
        float *q = base + r * p.pitch + c;
        const float v = *q;
        if (p.norm_type == 1)
            *q = v - st[c];
        else
            *q = (v - st[c]) * st[cols + c];
    }
}

// Statistics + apply of one SHORT segment in one block (an utterance of the batch entries, a small streaming block):
// the segment's rows are read once into LDS, the statistics are formed exactly as k_norm_stats forms them (same thread
// per (row class, column), same order of the double additions, same tree -- the results are the same bits), then every
// row is normalised from LDS and written back.  One read and one write of the data instead of two reads and one write,
// one launch instead of two: the reference's default configuration (CVN on 13 columns, ASR_OCL.cpp:560) spends
// 0.051 ms per 998 000 frames in the two-kernel form.  p.chunks = rows the block's LDS holds (a longer segment is
// processed from memory, correct but slow: the launcher does not choose this kernel for those).
#ifndef MFX_NORM_SEG_THREADS
#define MFX_NORM_SEG_THREADS 1024
#endif
constexpr int kNormSegThreads = MFX_NORM_SEG_THREADS; // the statistics keep k_norm_stats' 256-thread mapping; all threads move the rows
__global__ void __launch_bounds__(kNormSegThreads) k_norm_seg(NormParams p)
{
    extern __shared__ __attribute__((aligned(16))) float s_rows[];
    __shared__ double s_sum[256], s_sum2[256];
    __shared__ float s_min[256], s_max[256], s_st[512];
    const Segment sg = p.inline_seg ? p.seg0 : p.segs[blockIdx.x];
    const int cols = p.cols, n_out = sg.n_out;
    const int n = sg.pad > 0 ? sg.pad : sg.n_out;
    const int tid = threadIdx.x;
    // blockIdx.y = column group (static | delta | delta-delta blocks of the row, each with its own statistics)
    float *base = p.data + (sg.out_row0 + p.row_off) * (int64_t)p.pitch + p.col0 + blockIdx.y * cols;
    float *stats = p.stats + (int64_t)blockIdx.y * p.group_stats_stride + (int64_t)blockIdx.x * 2 * cols;
    const bool in_lds = n_out <= p.chunks;
    const int total = n_out * cols;
    // i / cols for the LDS-sized products (at most kNormSegLdsBytes / 4 elements)
    const uint32_t magic = div_magic(cols);
    const auto row_of = [&](int i) -> int { return div_small(i, cols, magic); };
    if (in_lds) { // 16 reads in flight per thread (a plain loop waits for every read before the next)
        const bool contig = p.pitch == cols;
        for (int i0 = tid; i0 < total; i0 += kNormSegThreads * 16) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int i = min(i0 + kNormSegThreads * k, total - 1); // (clamped, not predicated: no branch, all reads issued at once)
                const int r = row_of(i), c = i - r * cols;
                v[k] = base[contig ? (int64_t)i : (int64_t)r * p.pitch + c];
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int i = i0 + kNormSegThreads * k;
                if (i < total) s_rows[i] = v[k];
            }
        }
        __syncthreads();
    }
    const int lg = norm_lg(cols);
    const int rr = tid >> lg, c = tid & ((1 << lg) - 1);
    norm_rows_totals<true>([&](int r, int cc) { return in_lds ? s_rows[r * cols + cc] : base[(int64_t)r * p.pitch + cc]; }, 0, n, cols, lg,
                           tid, s_sum, s_sum2, s_min, s_max);
    if (rr == 0 && c < cols) {
        norm_finish_to(stats, cols, p.norm_type, c, n, s_sum[tid], s_sum2[tid], s_min[tid], s_max[tid]);
        s_st[c] = stats[c]; // (this thread's own writes)
        s_st[256 + c] = stats[cols + c];
    }
    __syncthreads();
    if (in_lds) {
        for (int i = tid; i < total; i += kNormSegThreads) {
            const int r = row_of(i), cc = i - r * cols;
            const float v = s_rows[i];
            base[(int64_t)r * p.pitch + cc] = p.norm_type == 1 ? v - s_st[cc] : (v - s_st[cc]) * s_st[256 + cc];
        }
    } else {
        for (int64_t i = tid; i < (int64_t)n_out * cols; i += kNormSegThreads) {
            const int64_t r = i / cols;
            const int cc = (int)(i - r * cols);
            float *q = base + r * p.pitch + cc;
            const float v = *q;
            *q = p.norm_type == 1 ? v - s_st[cc] : (v - s_st[cc]) * s_st[256 + cc];
        }
    }
}

// Copy of a small block by a kernel instead of a DMA command (streaming interface, blocks under 1 MB: an SDMA copy of a few
// hundred KB costs more in command latency than in transfer time).  Either side may be page-locked host memory (mapped into
// the device's address space).  vec: dst and src are congruent modulo 16 -- 16-byte words between a head and a tail of
// 2-byte units; else 2-byte units throughout (byte counts are even: int16 samples or float rows).
__global__ void __launch_bounds__(256) k_copy_small(char *dst, const char *src, size_t bytes, int vec)
{
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    if (vec) {
        size_t head = (16 - ((uintptr_t)dst & 15)) & 15;
        if (head > bytes) head = bytes;
        const size_t nvec = (bytes - head) >> 4, tail0 = head + (nvec << 4);
        const uint4 *s4 = (const uint4 *)(src + head);
        uint4 *d4 = (uint4 *)(dst + head);
        for (size_t v = gid; v < nvec; v += stride) d4[v] = s4[v];
        if (gid < (head >> 1)) ((short *)dst)[gid] = ((const short *)src)[gid];
        if (gid < ((bytes - tail0) >> 1)) ((short *)(dst + tail0))[gid] = ((const short *)(src + tail0))[gid];
    } else {
        for (size_t i = gid; i < (bytes >> 1); i += stride) ((short *)dst)[i] = ((const short *)src)[i];
    }
}

} // namespace

int num_cus()
{
    static thread_local int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (cached[dev] == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess) cached[dev] = prop.multiProcessorCount;
        if (cached[dev] <= 0) cached[dev] = 256;
    }
    return cached[dev];
}

hipError_t allow_dynamic_lds(const void *func, size_t lds_bytes)
{
    if (lds_bytes <= 64 * 1024) return hipSuccess;
    // The attribute belongs to the function on the device, for the whole process: the grant is cached process-wide and
    // only ever raised.  (A per-thread cache let a thread with a smaller need set it DOWN under another thread that had
    // cached its larger grant and went on launching with it: DESIGN.md B14.)
    struct Key {
        int dev;
        const void *func;
        size_t granted;
    };
    static std::mutex mu;
    static std::vector<Key> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lock(mu);
    Key *slot = nullptr;
    for (Key &k : cache)
        if (k.dev == dev && k.func == func) {
            if (k.granted >= lds_bytes) return hipSuccess;
            slot = &k;
            break;
        }
    const hipError_t e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    if (slot)
        slot->granted = lds_bytes;
    else
        cache.push_back(Key{dev, func, lds_bytes});
    return hipSuccess;
}

int blocks_per_cu(const void *func, int threads, size_t lds_bytes, int fallback)
{
    struct Key {
        int dev, threads;
        const void *func;
        size_t lds;
        int value;
    };
    static thread_local Key cache[16];
    static thread_local int used = 0, next = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    for (int i = 0; i < used; ++i)
        if (cache[i].dev == dev && cache[i].func == func && cache[i].threads == threads && cache[i].lds == lds_bytes) return cache[i].value;
    int v = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, func, threads, lds_bytes) != hipSuccess || v < 1) {
        (void)hipGetLastError();
        v = fallback;
    }
    cache[next] = Key{dev, threads, func, lds_bytes, v};
    next = (next + 1) % 16;
    if (used < 16) ++used;
    return v;
}

size_t melcep_lds_bytes(const MelcepParams &p, int n_waves)
{
    const size_t f = mel64_lds_floats(p.num_banks, p.mel.rounds, p.mel.row_stride) + 8 +
                     (size_t)n_waves * ((size_t)p.mag_floats + 4 * (size_t)lm_fs4(p.num_banks));
    return f * sizeof(float);
}

hipError_t launch_melcep(const MelcepParams &p, hipStream_t stream)
{
    if (p.n_rows <= 0) return hipSuccess;
    const int tables = p.n_tables > 1 ? p.n_tables : 1;
    if (!spec_rows_ok(p.mag_floats, p.spec_pitch) || tables > kGridYMax) return hipErrorInvalidValue;
    ResidentGrid g;
    if (hipError_t e = resident_grid((const void *)k_melcep, [&](int nw) { return melcep_lds_bytes(p, nw); }, (p.n_rows + 3) / 4, 1, g); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_melcep, dim3(g.blocks, (unsigned)tables), dim3(64 * g.waves), g.lds, stream, p);
    return hipGetLastError();
}

hipError_t launch_melcep_runs(const MelcepParams &p, const RowRuns &rr, const int32_t *h_off, const int64_t *h_runs, hipStream_t stream)
{
    const int tables = p.n_tables > 1 ? p.n_tables : 1;
    int active = 0;
    const int64_t groups = run_groups_in_window(h_off, h_runs, tables, rr.row0, rr.rows, 4, active); // of the busiest table
    if (groups <= 0) return hipSuccess;
    if (!spec_rows_ok(p.mag_floats, p.spec_pitch) || tables > kGridYMax) return hipErrorInvalidValue;
    ResidentGrid g;
    if (hipError_t e = resident_grid((const void *)k_melcep_runs, [&](int nw) { return melcep_lds_bytes(p, nw); }, groups, active, g); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_melcep_runs, dim3(g.blocks, (unsigned)tables), dim3(64 * g.waves), g.lds, stream, p, rr);
    return hipGetLastError();
}

hipError_t launch_delta(const DeltaParams &p, hipStream_t stream)
{
    if (p.n_segs <= 0 || p.tiles_per_seg_max <= 0) return hipSuccess;
    const int D = p.l1 + p.l2;
    const int groups = p.l2 > 0 ? 3 : 2;
    const bool whole_rows = p.out_pitch == p.cols * groups && ((uintptr_t)p.out & 15) == 0 && ((uintptr_t)p.src & 15) == 0;
    const auto tile_lds = [&](int rows, int cw) { return (size_t)((rows + 2 * D) + (rows + 2 * p.l2) + rows) * cw * sizeof(float); };
    constexpr int R4 = MFX_DELTA_WIDE_ROWS_V, RW = MFX_DELTA_WIDE_ROWS;
    const void *fn;
    int rows_t = kDeltaRows; // output rows per block
    size_t lds;
    if (p.cols <= 16 && p.l1 > 0 && D <= 16 && p.src_pitch == 16 && whole_rows) {
        fn = p.l1 == 3 && p.l2 == 3 ? (const void *)k_delta16<3, 3> : (const void *)k_delta16<0, 0>;
        rows_t = kDelta16TilesPerBlock * kDeltaRows;
        lds = (size_t)delta_wave_lds_floats(p.l1, p.l2) * sizeof(float);
    } else if (p.cols > 16 && (p.cols & 3) == 0 && p.l1 > 0 && (p.src_pitch & 3) == 0 && whole_rows && tile_lds(R4, p.cols) <= 64 * 1024) {
        // wide rows in whole 16-byte words: the vectorised form (C5: k_delta 0.052 ms -> see profiles/r03)
        fn = (const void *)k_delta4<R4>;
        rows_t = R4;
        lds = tile_lds(R4, p.cols);
    } else if (p.cols <= 16) {
        fn = (const void *)k_delta<true, kDeltaRows>;
        lds = tile_lds(kDeltaRows, 16);
    } else { // wide rows: tiles of MFX_DELTA_WIDE_ROWS output rows (less LDS per block: more blocks per CU in flight)
        fn = (const void *)k_delta<false, RW>;
        rows_t = RW;
        lds = tile_lds(RW, p.cols);
    }
    if (hipError_t e = allow_dynamic_lds(fn, lds); e != hipSuccess) return e;
    const int tiles_x = (int)(((int64_t)p.tiles_per_seg_max * kDeltaRows + rows_t - 1) / rows_t);
    return for_seg_slices(p.n_segs, [&](int s0, int n) {
        DeltaParams q = p;
        q.segs = p.segs + s0;
        q.n_segs = n;
        return launch_kernel(fn, dim3(tiles_x, n), dim3(256), lds, stream, q);
    });
}

static int norm_chunks(int max_rows) { return max_rows <= kNormChunkRows ? 1 : (max_rows + kNormChunkRows - 1) / kNormChunkRows; }

// the statistics of a slice's segments lie s0 segments further on
static void norm_slice_stats(NormParams &q, int s0) { q.stats += (int64_t)s0 * 2 * q.cols; }

hipError_t launch_norm_stats(const NormParams &p, hipStream_t stream)
{
    if (p.n_segs <= 0) return hipSuccess;
    if (p.cols > 256) return hipErrorInvalidValue;
    const int chunks = norm_chunks(p.max_rows);
    if (chunks > 1 && !p.partial) return hipErrorInvalidValue;
    return for_seg_slices(p.n_segs, [&](int s0, int n) {
        NormParams q = p;
        q.segs = p.segs + s0;
        q.n_segs = n;
        norm_slice_stats(q, s0);
        q.chunks = chunks;
        if (chunks > 1) q.partial = p.partial + (int64_t)s0 * chunks * 4 * p.cols;
        if (hipError_t e = launch_kernel((const void *)k_norm_stats, dim3(chunks, n), dim3(256), 0, stream, q); e != hipSuccess) return e;
        return chunks > 1 ? launch_kernel((const void *)k_norm_finalize, dim3(n), dim3(256), 0, stream, q) : hipSuccess;
    });
}

// stats + apply in one launch when every segment's rows fit one block's LDS (see k_norm_seg)
bool norm_fused_fits(int max_rows, int cols)
{
    return max_rows > 0 && cols > 0 && cols <= 256 && (size_t)max_rows * cols * sizeof(float) <= kNormSegLdsBytes;
}

hipError_t launch_norm_fused(const NormParams &p, hipStream_t stream)
{
    if (p.n_segs <= 0) return hipSuccess;
    if (!norm_fused_fits(p.max_rows, p.cols)) return hipErrorInvalidValue;
    const size_t lds = (size_t)p.max_rows * p.cols * sizeof(float);
    return for_seg_slices(p.n_segs, [&](int s0, int n) { // (segments along grid.x here; the same limit serves)
        NormParams q = p;
        q.segs = p.segs + s0;
        q.n_segs = n;
        norm_slice_stats(q, s0);
        q.chunks = p.max_rows; // rows the block's LDS holds
        return launch_kernel((const void *)k_norm_seg, dim3(n, p.groups > 1 ? p.groups : 1), dim3(kNormSegThreads), lds, stream, q);
    });
}

hipError_t launch_copy_small(void *dst, const void *src, size_t bytes, hipStream_t stream)
{
    if (bytes == 0) return hipSuccess;
    if (bytes & 1) return hipErrorInvalidValue;
    const int vec = (((uintptr_t)dst ^ (uintptr_t)src) & 15) == 0 ? 1 : 0;
    const size_t items = vec ? (bytes >> 4) + 16 : (bytes >> 1);
    size_t blocks = (items + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_copy_small, dim3((unsigned)blocks), dim3(256), 0, stream, (char *)dst, (const char *)src, bytes, vec);
    return hipGetLastError();
}

size_t norm_partial_doubles(int n_segs, int max_rows, int cols)
{
    const int ch = norm_chunks(max_rows);
    return ch <= 1 ? 0 : (size_t)n_segs * ch * 4 * cols;
}

hipError_t launch_norm_apply(const NormParams &p, hipStream_t stream)
{
    if (p.n_segs <= 0) return hipSuccess;
    // about 2048 elements per block, whatever the row count (a streaming block is one long segment)
    int64_t gx = ((int64_t)(p.max_rows > 0 ? p.max_rows : 1) * p.cols + 2047) / 2048;
    if (gx < 1) gx = 1;
    if (gx > 4096) gx = 4096;
    return for_seg_slices(p.n_segs, [&](int s0, int n) {
        NormParams q = p;
        q.segs = p.segs + s0;
        q.n_segs = n;
        norm_slice_stats(q, s0);
        return launch_kernel((const void *)k_norm_apply, dim3((unsigned)gx, n), dim3(256), 0, stream, q);
    });
}

} // namespace mfx
