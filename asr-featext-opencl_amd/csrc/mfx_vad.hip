// mfx_vad.hip -- energy voice-activity decision and voiced-frame selection of the batch entries (mfx_batch_set_vad), and
// their launcher.  See DESIGN.md section 5, "Voice activity and frame selection"; tiles and chunks are utterance tilings
// (UttTiling, mfx_kernels.h; utt_item, mfx_dev.h).
//
// Per utterance of T frames, e[t] = y[t][column] of the finished rows y (before a transform):
//   thr     = (float)(energy_threshold + energy_mean_scale * (S / T)),  S = sum of e[t] in double
//   flag[t] = (float)num >= (float)den * proportion_threshold, over the window [t - ctx, t + ctx] cut at the utterance ends:
//             den frames in it, num of them with e > thr (float32, a NaN is "not greater")
//
//   k_vad_sums    S of every chunk (kNormChunkRows rows) of every utterance: 256 threads, thread i adds rows i, i + 256, ... of the chunk
//                 in ascending order, then a halving tree through LDS -- one owner and one order per sum
//   k_vad_thresh  one thread per utterance: its chunks in ascending order from zero -> thr
//   k_vad_flags   one wave per tile of 64 consecutive rows of one utterance.  The "loud" bits e > thr of the tile, of the 64
//                 rows in front of it and of the 64 behind it are three ballots (of the neighbours only the ctx rows next
//                 to the tile are loaded); ctx <= 64, so every window lies inside those 192 bits and num is three masked
//                 population counts: no LDS, no barrier.  The flags' ballot is the tile's
//                 mask; flags go out as bytes, consecutive lanes on consecutive bytes.
//   k_vad_scan    one wave per utterance: population counts of its tile masks -> exclusive prefix (the tile's first voiced
//                 row inside the utterance) and the total voiced[u]
//   k_vad_pack    one block: exclusive prefix of voiced[] over the batch -> packed_row0 [n_utt + 1]
//   k_vad_select  one block per tile: every voiced row whole from the scratch to its destination row (rank inside the tile =
//                 population count of the mask below the row), and zeros into the destination rows no voiced row lands on.
//                 Destination row k of an utterance (SELECT) or of the batch (PACK) is zeroed by the tile that owns SOURCE
//                 row k, so every destination row has exactly one writer.  16-byte words where width and pointer allow.
// Nothing here is atomic and no result depends on timing.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include <type_traits>

#include "mfx_dev.h"
#include "mfx_launch.h"
#include "mfx_norm_dev.h"

namespace mfx {

namespace {

// bits a .. b (inclusive) of a 64-bit mask counted, the range cut to 0 .. 63
__device__ __forceinline__ int bits_between(uint64_t m, int a, int b)
{
    a = max(a, 0), b = min(b, 63);
    if (b < a) return 0;
    const int w = b - a + 1;
    const uint64_t sel = (w == 64 ? ~0ull : ((1ull << w) - 1)) << a;
    return __popcll(m & sel);
}

// grid = chunks of the utterance range
__global__ void __launch_bounds__(256) k_vad_sums(VadParams p)
{
    __shared__ double s_sum[256];
    const int c = p.chunks.first + blockIdx.x;
    const UttItem ch = utt_item<kNormChunkRows>(p.chunks, p.segs, c);
    const int r0 = ch.t0, r1 = ch.t0 + ch.n;
    const float *e = p.y + ch.row0 * (int64_t)p.y_pitch + p.column;
    const int tid = threadIdx.x;
    double sum = 0;
    for (int r = r0 + tid; r < r1; r += 256) sum += (double)e[(int64_t)r * p.y_pitch];
    s_sum[tid] = sum;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) s_sum[tid] += s_sum[tid + s];
        __syncthreads();
    }
    if (tid == 0) p.partial[c] = s_sum[0];
}

// grid = utterances of the range / 256
__global__ void __launch_bounds__(256) k_vad_thresh(VadParams p)
{
    const int u = p.u0 + blockIdx.x * 256 + threadIdx.x;
    if (u >= p.u1) return;
    const int T = p.segs[u].n_out;
    double S = 0;
    for (int c = p.chunks.utt_item0[u]; c < p.chunks.utt_item0[u + 1]; ++c) S += p.partial[c];
    // (the two roundings spelled out: no fused multiply-add between them)
    p.thr[u] = T > 0 ? (float)__dadd_rn((double)p.energy_threshold, __dmul_rn((double)p.energy_mean_scale, S / (double)T)) : p.energy_threshold;
}

// grid = tiles of the range / 4; a wave per tile
__global__ void __launch_bounds__(256) k_vad_flags(VadParams p)
{
    const int lane = threadIdx.x & 63;
    const int tile = p.tiles.first + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= p.tiles.first + p.tiles.count) return; // (whole waves leave; nothing below synchronises the block)
    const UttItem v = utt_item<kVadTileRows>(p.tiles, p.segs, tile);
    const float thr = p.thr[v.u];
    const float *e = p.y + v.row0 * (int64_t)p.y_pitch + p.column;
    const int ctx = p.frames_context;
    const int t = v.t0 + lane;
    auto loud = [&](int tt) { return tt >= 0 && tt < v.T && e[(int64_t)tt * p.y_pitch] > thr; };
    const uint64_t cur = __ballot(loud(t));
    uint64_t prev = 0, next = 0;
    if (ctx > 0) { // (wave-uniform) only the ctx rows next to the tile are ever counted: the other lanes load nothing
        prev = __ballot(lane >= 64 - ctx && loud(t - 64));
        next = __ballot(lane < ctx && loud(t + 64));
    }
    bool flag = false;
    if (t < v.T) {
        const int lo = max(t - ctx, 0), hi = min(t + ctx, v.T - 1);
        const int den = hi - lo + 1;
        const int a = lo - v.t0, b = hi - v.t0; // relative to the tile: -64 .. 127
        const int num = bits_between(prev, a + 64, b + 64) + bits_between(cur, a, b) + bits_between(next, a - 64, b - 64);
        flag = (float)num >= (float)den * p.proportion_threshold;
        p.flags[v.row0 + t] = flag ? 1 : 0;
    }
    const uint64_t voiced = __ballot(flag);
    if (lane == 0) p.mask[tile] = voiced;
}

// grid = utterances of the range / 4; a wave per utterance
__global__ void __launch_bounds__(256) k_vad_scan(VadParams p)
{
    const int lane = threadIdx.x & 63;
    const int u = p.u0 + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= p.u1) return;
    const int i0 = p.tiles.utt_item0[u], i1 = p.tiles.utt_item0[u + 1];
    int running = 0;
    for (int b = i0; b < i1; b += 64) {
        const int i = b + lane;
        const int c = i < i1 ? __popcll(p.mask[i]) : 0;
        int x = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (i < i1) p.tile_base[i] = running + x - c;
        running += __shfl(x, 63, 64);
    }
    if (lane == 0) p.voiced[u] = running;
}

// one block of 1024: packed_row0[u] = voiced[0] + ... + voiced[u - 1], packed_row0[n_utt] = the batch's voiced rows
__global__ void __launch_bounds__(1024) k_vad_pack(VadParams p)
{
    __shared__ int64_t s[2][1024];
    const int tid = threadIdx.x;
    int64_t running = 0;
    for (int b = 0; b < p.n_utt; b += 1024) {
        const int u = b + tid;
        const int64_t c = u < p.n_utt ? p.voiced[u] : 0;
        int cur = 0;
        s[0][tid] = c;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            s[cur ^ 1][tid] = s[cur][tid] + (tid >= d ? s[cur][tid - d] : 0);
            cur ^= 1;
            __syncthreads();
        }
        if (u < p.n_utt) p.packed_row0[u] = running + s[cur][tid] - c;
        running += s[cur][1023];
        __syncthreads(); // (the next round writes s[0])
    }
    if (tid == 0) p.packed_row0[p.n_utt] = running;
}

// grid = tiles of the range.  VEC: rows as 16-byte words (width a multiple of 4, both pointers 16-byte aligned)
template <bool VEC>
__global__ void __launch_bounds__(256) k_vad_select(VadParams p)
{
    typedef typename std::conditional<VEC, f32x4, float>::type word;
    const int tile = p.tiles.first + blockIdx.x;
    const UttItem v = utt_item<kVadTileRows>(p.tiles, p.segs, tile);
    const uint64_t mask = p.mask[tile];
    const bool pack = p.mode == 2;
    // first destination row of the tile's voiced rows; destination rows from `zero_from` on (of the utterance, or of the
    // batch when packing) hold no voiced row
    const int64_t dst0 = (pack ? p.packed_row0[v.u] : v.row0) + p.tile_base[tile];
    const int64_t zero_from = pack ? p.packed_row0[p.n_utt] : v.row0 + p.voiced[v.u];
    const int Wq = VEC ? p.width >> 2 : p.width; // words of a row
    const word *src = (const word *)p.rows + (v.row0 + v.t0) * (int64_t)Wq;
    word *out = (word *)p.out;
    const uint32_t magic = Wq > 1 ? 0xffffffffu / (uint32_t)Wq + 1 : 0; // i / Wq for i < 2^16 (64 rows of at most 1023 words)
    const int total = v.n * Wq;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int r = Wq > 1 ? (int)__umulhi((uint32_t)i, magic) : i;
        const int c = i - r * Wq;
        if ((mask >> r) & 1) {
            const int rank = __popcll(mask & ((1ull << r) - 1));
            out[(dst0 + rank) * Wq + c] = src[i];
        }
        const int64_t own = v.row0 + v.t0 + r; // the destination row this source row answers for
        if (own >= zero_from) out[own * Wq + c] = word{};
    }
}

} // namespace

bool vad_shape_ok(const VadParams &p)
{
    return p.frames_context >= 0 && p.frames_context <= kVadTileRows && p.column >= 0 && p.column < p.y_pitch && p.width >= 1 && p.width <= 1023 &&
           p.mode >= 0 && p.mode <= 2;
}

// the launches of one run over utterances [u0, u1): the tiles and the chunks of that range
hipError_t launch_vad(const VadParams &p, hipStream_t stream)
{
    if (p.u1 <= p.u0) return hipSuccess;
    if (!vad_shape_ok(p)) return hipErrorInvalidValue;
    if (p.mode != 0 && (!p.rows || !p.out || p.rows == p.out)) return hipErrorInvalidValue;
    if (p.tiles.rows != kVadTileRows || p.chunks.rows != kNormChunkRows) return hipErrorInvalidValue; // (the kernels' constants)
    const int n_tiles = p.tiles.count, n_chunks = p.chunks.count;
    const int n = p.u1 - p.u0;
    if (n_chunks > 0) hipLaunchKernelGGL(k_vad_sums, dim3(n_chunks), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(k_vad_thresh, dim3((n + 255) / 256), dim3(256), 0, stream, p);
    if (n_tiles > 0) hipLaunchKernelGGL(k_vad_flags, dim3((n_tiles + 3) / 4), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(k_vad_scan, dim3((n + 3) / 4), dim3(256), 0, stream, p);
    if (p.u1 == p.n_utt) hipLaunchKernelGGL(k_vad_pack, dim3(1), dim3(1024), 0, stream, p); // (every count is final by now)
    if (p.mode != 0 && n_tiles > 0) {
        const bool vec = (p.width & 3) == 0 && (((uintptr_t)p.rows | (uintptr_t)p.out) & 15) == 0;
        if (vec)
            hipLaunchKernelGGL(k_vad_select<true>, dim3(n_tiles), dim3(256), 0, stream, p);
        else
            hipLaunchKernelGGL(k_vad_select<false>, dim3(n_tiles), dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

} // namespace mfx
