// mfx_front_dev.h -- what the register front ends share (k_front512 and k_front1024 in mfx_front512.hip, k_front2048 in
// mfx_front2048.hip), each piece once: the per-chunk PCM descriptor, the block-local work draw, the PCM loads, the real
// split's bin pair and partner fetches, the mel walk's batches, the row sum of the quartered DCT, and the staging of the
// lane-major tables into LDS.  Only what leaves every instantiation's machine code as it was is here: see
// profiles/r06/README.md for the pieces that had to stay in the kernel bodies.
#pragma once
#include "mfx_dev.h"

namespace mfx {
namespace {

constexpr int kTabStride = 36;   // dwords per lane row of the window / pass-twiddle tables in LDS (16 complex + pad)
constexpr int kSplitStride = 20; // dwords per lane row of the split-twiddle table (8 complex + pad)

// Dev-only in-kernel stamps (-DMFX_STAMPS): per-wave cycle sums per phase (st_acc / st_last of the kernel), written by lane 0
// to p.spec (which is unused by the fused path); tools/stamps.py and tools/stamps2048.py read them.  Never part of a timed build.
#ifdef MFX_STAMPS
#define MFX_STAMP(i)                                                                   \
    do {                                                                               \
        unsigned long long t_;                                                         \
        __builtin_amdgcn_sched_barrier(0);                                             \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");     \
        __builtin_amdgcn_sched_barrier(0);                                             \
        st_acc[i] += t_ - st_last;                                                     \
        st_last = t_;                                                                  \
    } while (0)
#else
#define MFX_STAMP(i)
#endif

// ---- chunk descriptor: a chunk's rows and a buffer descriptor over [chunk start, end of PCM) -- out-of-range lanes read 0
struct ChunkCtx {
    int64_t out_row;
    int n_live; // frames of the chunk below the row limit
    int odd0;   // ODD: the chunk starts on an odd sample (its descriptor on the even one before)
    __amdgpu_buffer_rsrc_t rsrc;
};

// EL: int16 elements per sample (2: interleaved stereo -- p.pcm_total counts elements, every sample is a whole, aligned word).
// ODD: a mono chunk may start on an odd sample.  c >= p.n_chunks gives an empty chunk over an empty range.
template <int EL, bool ODD>
__device__ __forceinline__ ChunkCtx chunk_ctx(const FrontParams &p, int c)
{
    ChunkCtx x;
    const bool valid = c < p.n_chunks;
    const Chunk *chp = p.chunks + (valid ? c : 0);
    const int64_t pcm_off = chp->pcm_off;
    x.out_row = chp->out_row;
    const int n_frames = valid ? chp->n_frames : 0;
    const int64_t rows_left = p.row_limit - x.out_row;
    x.n_live = (int)(rows_left < n_frames ? (rows_left < 0 ? 0 : rows_left) : n_frames);
    const int64_t base_s = EL == 2 ? pcm_off * 2 : ODD ? (pcm_off & ~(int64_t)1) : pcm_off;
    x.odd0 = (EL == 1 && ODD) ? (int)(pcm_off & 1) : 0;
    // (rounded up to whole 32-bit words: with an odd sample count the array's last sample sits in a word whose
    // upper half lies past the end, and the range check would drop the whole word -- the base is 4-byte aligned,
    // so that word is inside the allocation, and the half past the end only ever meets a zero window tap)
    int64_t bytes_left = valid ? (((p.pcm_total - base_s) * 2 + 3) & ~(int64_t)3) : 0;
    if (bytes_left > 0xfffffff0ll) bytes_left = 0xfffffff0ll;
    if (bytes_left < 0) bytes_left = 0;
    const uintptr_t bp = (uintptr_t)(p.pcm + base_s);
    const uint32_t bp_lo = __builtin_amdgcn_readfirstlane((uint32_t)bp);
    const uint32_t bp_hi = __builtin_amdgcn_readfirstlane((uint32_t)(bp >> 32));
    const uint32_t nbytes = __builtin_amdgcn_readfirstlane((uint32_t)bytes_left);
    x.rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(((uintptr_t)bp_hi << 32) | bp_lo), 0, nbytes, 0x00020000);
    return x;
}

// ---- work draw.  Block b owns chunks b, b + B, b + 2B, ...; its waves draw from that list through a counter in LDS (a
// ds_add_rtn costs ~100 cycles and contends with the block's other waves only), so waves that the SIMD arbiter favours
// simply take more chunks instead of finishing early and idling the CU.
__device__ __forceinline__ int draw_index(int *s_ctr, int lane)
{
    int k = 0;
    if (lane == 0) k = __hip_atomic_fetch_add(s_ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return k;
}

// chunk of the k-th draw of block `block_id` (xcd_block_id: consecutive ids, i.e. consecutive chunks, on one XCD's L2);
// n_chunks when the list is exhausted
__device__ __forceinline__ int chunk_of_draw(int block_id, int k, int n_chunks)
{
    const long long c = (long long)block_id + (long long)k * gridDim.x;
    return c < n_chunks ? (int)c : n_chunks;
}

// ---- PCM loads.  PCM is fetched with buffer loads (hardware range check: reads past the end of the array return 0) one
// iteration ahead of its use.
template <bool ALIGNED, int NM>
struct PcmRegs {
    uint32_t d[ALIGNED ? NM : 2 * NM];
};

// issue the loads of one iteration (4 frames); `voff` = byte offset of this lane's first pair
template <bool ALIGNED, int NM>
__device__ __forceinline__ void pcm_issue(PcmRegs<ALIGNED, NM> &r, __amdgpu_buffer_rsrc_t rsrc, int voff)
{
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        if (ALIGNED) {
            r.d[m] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff + 64 * m, 0, 0);
        } else {
            r.d[2 * m] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff + 64 * m, 0, 0);
            r.d[2 * m + 1] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff + 64 * m + 4, 0, 0);
        }
    }
}

// The zero-stuffed form (256-point transforms on the 512-point core, k_front512<.., STUFF>): ONE sample per lane and row,
// 16 samples per row; `voff` = byte offset of this lane's first sample
template <int NM>
__device__ __forceinline__ void pcm_issue_stuffed(PcmRegs<true, NM> &r, __amdgpu_buffer_rsrc_t rsrc, int voff, int row_bytes)
{
#pragma unroll
    for (int m = 0; m < NM; ++m) r.d[m] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(rsrc, voff, row_bytes * m, 0);
}

// value i of a row of complex pairs held as 16-byte words (two per word)
template <int N>
__device__ __forceinline__ float2 pair_at(const float4 (&q)[N], int i)
{
    return (i & 1) ? make_float2(q[i >> 1].z, q[i >> 1].w) : make_float2(q[i >> 1].x, q[i >> 1].y);
}

// ---- real split.  Partner fetch: lanes l >= 1 get x[16 - l] (mirror, then shift right by one inside the row);
// lane 0, which the shift leaves without a source, keeps `own` -- its partner lives in its own registers.
__device__ __forceinline__ float row_partner_own0(float own, float x)
{
    int t = __builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x140, 0xf, 0xf, true);   // row_mirror
    t = __builtin_amdgcn_update_dpp(__float_as_int(own), t, 0x111, 0xf, 0xf, false);    // row_shr:1, lane 0 keeps old
    return __int_as_float(t);
}

// x of lane 15 - l of the same 16-lane row
__device__ __forceinline__ float row_mirror(float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x140, 0xf, 0xf, true));
}

// One bin pair (k, N - k) of the split, a = Z[k], (zr, zi) = the partner Z[N - k], cs = -i W^k:
//   S = Z[k] + conj Z[N-k], T = cs (Z[k] - conj Z[N-k]):  X[k] = S + T,  X[N-k] = conj(S - T)
// (the twiddle of bin N - k is the conjugate of bin k's); mk = |X[k]|, mp = |X[N-k]| (the window taps carry 0.5 / W2)
__device__ __forceinline__ void split_pair(float2 a, float zr, float zi, float2 cs, float &mk, float &mp)
{
    const float sr = a.x + zr, si = a.y - zi;
    const float dr = a.x - zr, di = a.y + zi;
    const float tr = cs.x * dr - cs.y * di;
    const float ti = cs.x * di + cs.y * dr;
    const float xr = sr + tr, xi = si + ti;
    const float yr = sr - tr, yi = si - ti;
    mk = __builtin_amdgcn_sqrtf(xr * xr + xi * xi);
    mp = __builtin_amdgcn_sqrtf(yr * yr + yi * yi);
}

// ---- mel walk.  One batch: NB bins (8 or 16) of a round, every read issued before the first multiply -- the weights as
// 16-byte words, the magnitudes as 8-byte words that stay apart (lds_read_b64), all at immediate offsets from the batch's two
// addresses -- so that a batch is ONE dependent LDS round trip whatever its size.  (The barrier: left alone the scheduler
// keeps three magnitude reads in flight and issues the rest between the multiplies.)  The products are added to the one
// accumulator in ascending bin order (mfcccpu.cpp:192-220): the same chain of multiply-adds as 8 bins at a time.
template <int NB>
__device__ __forceinline__ float mel_batch(float acc, const float *w, const float *m)
{
    float4 wq[NB / 4];
    float2 mm[NB / 2];
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) wq[q] = *(const float4 *)(w + 4 * q);
#pragma unroll
    for (int q = 0; q < NB / 2; ++q) mm[q] = lds_read_b64((const float2 *)(m + 2 * q));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) {
        acc += wq[q].x * mm[2 * q].x;
        acc += wq[q].y * mm[2 * q].y;
        acc += wq[q].z * mm[2 * q + 1].x;
        acc += wq[q].w * mm[2 * q + 1].y;
    }
    return acc;
}

// One round of the walk (L bins, a multiple of 8): 16 bins at a time, then the 8-bin remainder.  The 32 registers of a
// 16-bin batch are free in the walk (the frame loop needs its 128 in pass A only); 32-bin batches spill
// (profiles/r05/abx_c2_mel_round_batches.txt).  L is uniform: scalar branches.
__device__ __forceinline__ float mel_round(const float *w, const float *m, int L)
{
    float acc = 0.f;
    int s = 0;
    for (; s + 16 <= L; s += 16) acc = mel_batch<16>(acc, w + s, m + s);
    if (s < L) acc = mel_batch<8>(acc, w + s, m + s);
    return acc;
}

// ---- quartered DCT on the matrix pipe (k_front512: kDctQ, k_front1024: kDctQL bands per quarter), the cross-row sum:
// dacc + dacc2 (the even / odd band chains) hold in register i of lane (kb, c) frame i's partial sum of column c over quarter
// kb; the lane that stores out[slot][l] is (row slot, column l): the quarters are added across the four 16-lane rows while
// frame i's sums move to row i (two butterfly steps: rows 1 <-> 0 / 3 <-> 2, then the two halves of the wave).
__device__ __forceinline__ float dct_quarters_sum(f32x4 dacc, f32x4 dacc2)
{
    const auto r01 = __builtin_amdgcn_permlane16_swap(__float_as_uint(dacc[0] + dacc2[0]), __float_as_uint(dacc[1] + dacc2[1]), false, false);
    const auto r23 = __builtin_amdgcn_permlane16_swap(__float_as_uint(dacc[2] + dacc2[2]), __float_as_uint(dacc[3] + dacc2[3]), false, false);
    const float s01 = __uint_as_float(r01[0]) + __uint_as_float(r01[1]);
    const float s23 = __uint_as_float(r23[0]) + __uint_as_float(r23[1]);
    const auto rr = __builtin_amdgcn_permlane32_swap(__float_as_uint(s01), __float_as_uint(s23), false, false);
    return __uint_as_float(rr[0]) + __uint_as_float(rr[1]);
}

// ---- staging of the shared tables into LDS (every thread of the block, before the block's first barrier)
// window pairs / pass twiddles: HBM tables are [lane][m] as well; value i of `src` to its lane row of `dst`
__device__ __forceinline__ void stage_lane_row(float *dst, const float *src, int i)
{
    ((float2 *)(dst + (i >> 4) * kTabStride))[i & 15] = ((const float2 *)src)[i];
}
// split twiddles: bin i = l + 16 p of the natural order to lane row l, place p
__device__ __forceinline__ void stage_split(float *dst, int i, float2 v)
{
    ((float2 *)(dst + (i & 15) * kSplitStride))[i >> 4] = v;
}
__device__ __forceinline__ void stage_mel_weights(float *s_melw, const FrontParams &p, int tid, int threads)
{
    for (int i = tid; i < 16 * p.mel16.row_stride; i += threads) s_melw[i] = p.mel16.w[i];
}
} // namespace
} // namespace mfx
