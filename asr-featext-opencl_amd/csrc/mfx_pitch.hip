// mfx_pitch.hip -- pitch track of the batch entries (mfx_batch_set_pitch): normalised cross-correlation of the PCM the front
// end reads, then a Viterbi path through its lag states, and their launcher.  See DESIGN.md section 5, "Pitch track"; the
// definition both kernels follow operation for operation is in include/mfx.h.
//
//   k_pitch_nccf   one block of 4 waves per tile of at most 64 consecutive frames of one utterance (an utterance tiling,
//                  UttTiling of mfx_kernels.h, at pitch_tile_frames frames: the one item size that is no constant).  The tile's PCM span goes
//                  into LDS once as int16, zero behind the utterance's own end (explicit bounds: a neighbour is never read),
//                  with pitch_span_pad empty slots behind every `shift` samples, so that the frames of the tile start on
//                  different banks.  Then, one frame per lane (16 lanes of every wave): the integer sum, m, and the double
//                  prefix as two chains that run `window` samples apart -- P[l + window] and P[l], each the ascending sum the
//                  definition asks for -- whose differences e(l_k) are parked in the frame's NCCF row.  Then, one frame per
//                  wave (or per half wave, pitch_groups): z = x - m into an LDS row, and the correlation chains, lags across
//                  lanes and four consecutive lags per lane.  A step of four samples is one broadcast 16-byte read of z[j .. j + 3] and one
//                  lane-consecutive 16-byte read of z[j + l + 4 .. j + l + 7] (the lane's lags start on a multiple of 4) for
//                  16 multiply-adds: every chain is whole, in ascending j, on one lane.  rho overwrites e in the row.
//   k_pitch_track  one block per utterance, one state per thread.  fwd lives in LDS (two buffers), ln(lag) too; per frame a
//                  scan of the 2 J + 1 predecessors in ascending order, eight at a time, and an argmin over the block that
//                  carries the index (ties go to the smaller state).  The frames go through in groups of 16: a group's rho rows
//                  are fetched together and its back-pointer rows written together, because every barrier waits for the
//                  block's loads in flight (an hour's stream 1073 -> 952 ms).  The backtrace pulls the back-pointer rows through LDS the same way, 16 frames at a
//                  time from the end: one thread walks them there, then 16 threads write those rows' lag, rho and index.
// Nothing here is atomic, no result depends on timing or on the other utterances of the batch.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_dev.h"
#include "mfx_launch.h"

// every float32 / double operation below is rounded on its own (the chains are spelled fmaf)
#pragma clang fp contract(off)

namespace mfx {

namespace {

constexpr int kPitchRows = 16; // frames whose rho and back-pointer rows a block of k_pitch_track holds in LDS at a time

// dynamic LDS of k_pitch_track at n threads: fwd [2][n], ln(lag) [n], rho [kPitchRows][n] floats, back-pointers [kPitchRows][n]
inline size_t pitch_track_lds_bytes(int n) { return (size_t)n * ((3 + kPitchRows) * sizeof(float) + kPitchRows * sizeof(uint16_t)); }

// floats of a wave's z row: the frame's span, and what the last 4-sample step of the last lane reads past it (zeros)
__host__ __device__ inline int pitch_z_floats(int window, int lag_max) { return (window + lag_max + 8 + 3) & ~3; }

// int16 slots of the staged span of `frames` frames (pitch_span_slots of mfx_tables.cpp)
__host__ __device__ inline int pitch_slots(int window, int lag_max, int shift, int pad, int frames)
{
    const int last = (frames - 1) * shift + window + lag_max - 1;
    return last + pad * (last / shift) + 1;
}

// a walk through the padded span, sample by sample
struct SpanWalk {
    int pos, left;
    __device__ __forceinline__ SpanWalk(int i, int shift, int pad) : pos(i + pad * (i / shift)), left(shift - i % shift) {}
    __device__ __forceinline__ void next(int shift, int pad)
    {
        ++pos;
        if (--left == 0) pos += pad, left = shift;
    }
};

// grid = tiles of the utterance range
__global__ void __launch_bounds__(256) k_pitch_nccf(PitchParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const UttItem tl = utt_item<0>(p.tiles, p.segs, p.tiles.first + blockIdx.x);
    const int u = tl.u, t0 = tl.t0, nf = tl.n;
    const int W = p.window, S = p.shift, pad = p.span_pad, K = p.K, Ls = W + p.lag_max;
    const int zs = pitch_z_floats(W, p.lag_max);
    const int G = p.groups, gl_n = 64 / G; // frames a wave takes at a time, lanes of each
    float *s_z = (float *)smem;           // [4 G][zs]
    float *s_m = s_z + 4 * G * zs;        // [64]
    float *s_e0 = s_m + 64;               // [64]
    int16_t *s_pcm = (int16_t *)(s_e0 + 64);

    // ---- the tile's span, zero from the utterance's end on
    {
        const int64_t off = p.utt[2 * u], n = p.utt[2 * u + 1];
        const int64_t g0 = (int64_t)t0 * S;
        const int span = (nf - 1) * S + Ls;
        for (int i = tid; i < span; i += 256) {
            const int64_t g = g0 + i;
            int v = 0;
            if (g < n) {
                if (p.channels == 2) {
                    const uint32_t d = ((const uint32_t *)p.pcm)[off + g];
                    v = ((int)(int16_t)(d & 0xffffu) + ((int)d >> 16)) >> 1;
                } else {
                    v = p.pcm[off + g];
                }
            }
            s_pcm[i + pad * (i / S)] = (int16_t)v;
        }
    }
    __syncthreads();

    float *rows = p.nccf + (tl.row0 + t0) * (int64_t)K;
    // ---- one frame per lane: sum, mean, the two prefix chains
    if (lane < 16 && wave * 16 + lane < nf) {
        const int f = wave * 16 + lane;
        int sI = 0;
        {
            SpanWalk w(f * S, S, pad);
            for (int j = 0; j < Ls; ++j, w.next(S, pad)) sI += s_pcm[w.pos];
        }
        const float m = (float)sI * p.c1;
        auto q = [&](int pos) {
            const float z = (float)s_pcm[pos] * 0x1p-15f - m;
            const float zz = z * z;
            return (double)zz;
        };
        double A = 0.0, B = 0.0; // P[l], P[l + W]
        SpanWalk wa(f * S, S, pad), wb(f * S, S, pad);
        for (int j = 0; j < W; ++j, wb.next(S, pad)) B = B + q(wb.pos);
        s_m[f] = m;
        s_e0[f] = (float)B;
        float *e = rows + (int64_t)f * K;
        for (int l = 0;; ++l) {
            if (l >= p.lag_min) e[l - p.lag_min] = (float)(B - A);
            if (l == p.lag_max) break;
            A = A + q(wa.pos);
            B = B + q(wb.pos);
            wa.next(S, pad), wb.next(S, pad);
        }
    }
    __syncthreads(); // (the rows' e, written above, are read below by other waves of this block)

    // ---- one frame per group of gl_n lanes (G = 1: per wave): z, then the chains
    const int g = lane / gl_n, gl = lane - g * gl_n;
    float *z = s_z + (wave * G + g) * zs;
    const int lag_lo4 = p.lag_min & ~3;
    const int passes = (p.lag_max - lag_lo4) / (4 * gl_n) + 1;
    const int W4 = W & ~3;
    for (int f0 = 0; f0 < nf; f0 += 4 * G) {
        const int f = f0 + wave * G + g;
        const bool live = f < nf;
        const float m = live ? s_m[f] : 0.f, e0 = live ? s_e0[f] : 0.f;
        wave_sync(); // (the previous frames' reads of z are done)
        if (live) {
            for (int j = gl; j < Ls; j += gl_n) {
                const int i = f * S + j;
                z[j] = (float)s_pcm[i + pad * (i / S)] * 0x1p-15f - m;
            }
            for (int j = Ls + gl; j < zs; j += gl_n) z[j] = 0.f;
        }
        wave_sync();
        if (!live) continue; // (whole groups; nothing below synchronises)
        float *row = rows + (int64_t)f * K;
        for (int ps = 0; ps < passes; ++ps) {
            const int base = lag_lo4 + 4 * gl_n * ps + 4 * gl; // this lane's lags: base .. base + 3
            if (base > p.lag_max) continue;
            float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
            const float *zb = z + base;
            float4 b0 = lds_read_b128((const float4 *)zb);
            int j = 0;
            for (; j < W4; j += 4) {
                const float4 a = lds_read_b128((const float4 *)(z + j));
                const float4 b1 = lds_read_b128((const float4 *)(zb + j + 4));
                c0 = fmaf(a.x, b0.x, c0), c1 = fmaf(a.x, b0.y, c1), c2 = fmaf(a.x, b0.z, c2), c3 = fmaf(a.x, b0.w, c3);
                c0 = fmaf(a.y, b0.y, c0), c1 = fmaf(a.y, b0.z, c1), c2 = fmaf(a.y, b0.w, c2), c3 = fmaf(a.y, b1.x, c3);
                c0 = fmaf(a.z, b0.z, c0), c1 = fmaf(a.z, b0.w, c1), c2 = fmaf(a.z, b1.x, c2), c3 = fmaf(a.z, b1.y, c3);
                c0 = fmaf(a.w, b0.w, c0), c1 = fmaf(a.w, b1.x, c1), c2 = fmaf(a.w, b1.y, c2), c3 = fmaf(a.w, b1.z, c3);
                b0 = b1;
            }
            for (; j < W; ++j) {
                const float a = z[j];
                c0 = fmaf(a, zb[j], c0), c1 = fmaf(a, zb[j + 1], c1), c2 = fmaf(a, zb[j + 2], c2), c3 = fmaf(a, zb[j + 3], c3);
            }
            const float c[4] = {c0, c1, c2, c3};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int l = base + r;
                if (l < p.lag_min || l > p.lag_max) continue;
                const float prod = e0 * row[l - p.lag_min];
                const float s = prod + p.ballast;
                row[l - p.lag_min] = s > 0.f ? c[r] / __builtin_sqrtf(s) : 0.f;
            }
        }
    }
}

// the smallest index among the smallest values of the block: (v, i) of every thread in, the winner's out (all threads)
__device__ __forceinline__ void block_argmin(float &v, int &i, float *s_v, int *s_i, int n_waves)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const float ov = __shfl_xor(v, d, 64);
        const int oi = __shfl_xor(i, d, 64);
        if (ov < v || (ov == v && oi < i)) v = ov, i = oi;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_v[wave] = v, s_i[wave] = i;
    __syncthreads();
    v = s_v[0], i = s_i[0];
    for (int w = 1; w < n_waves; ++w) // (ascending waves hold ascending states: a tie keeps the earlier)
        if (s_v[w] < v) v = s_v[w], i = s_i[w];
}

// grid = utterances of the range; block = K rounded up to whole waves; pitch_track_lds_bytes of dynamic LDS
__global__ void __launch_bounds__(512) k_pitch_track(PitchParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float s_v[8];
    __shared__ int s_i[8];
    __shared__ int s_path[kPitchRows];
    __shared__ int s_k;
    const int u = p.u0 + blockIdx.x;
    const Segment sg = p.segs[u];
    const int T = sg.n_out;
    if (T <= 0) return; // (uniform: the whole block leaves)
    const int K = p.K, J = p.J, tid = threadIdx.x, n = blockDim.x, n_waves = n >> 6;
    float *s_fwd = (float *)smem;                              // [2][n]
    float *s_lg = s_fwd + 2 * n;                               // [n]
    float *s_rho = s_lg + n;                                   // [kPitchRows][n]: every thread reads its own column only
    uint16_t *s_bp = (uint16_t *)(s_rho + kPitchRows * n);     // [kPitchRows][n]
    const bool act = tid < K;
    const float *nccf = p.nccf + sg.out_row0 * (int64_t)K;
    uint16_t *bp = p.bp + sg.out_row0 * (int64_t)K;
    const float lgk = act ? p.lg[tid] : 0.f, wtk = act ? p.wt[tid] : 0.f;
    s_lg[tid] = lgk;
    float fwd = 0.f;
    int end = 0;
    __syncthreads();
    // kPitchRows frames at a time: their rho rows come in together (one HBM round trip, not one per frame: every barrier
    // below waits for the loads in flight), their back-pointer rows go out together
    for (int c0 = 0; c0 < T; c0 += kPitchRows) {
        const int nc = min(kPitchRows, T - c0);
        if (act) {
            float in[kPitchRows];
#pragma unroll
            for (int r = 0; r < kPitchRows; ++r) in[r] = r < nc ? nccf[(int64_t)(c0 + r) * K + tid] : 0.f;
#pragma unroll
            for (int r = 0; r < kPitchRows; ++r) s_rho[r * n + tid] = in[r];
        }
        for (int r = 0; r < nc; ++r) {
            const int t = c0 + r;
            const float rw = (act ? s_rho[r * n + tid] : 0.f) * wtk;
            const float loc = 1.0f - rw;
            float a = loc;
            if (t > 0 && act) {
                const float *prev = s_fwd + ((t - 1) & 1) * n;
                float best = __builtin_inff();
                int bk = 0;
                const int hi = min(K - 1, tid + J);
                int kk = max(0, tid - J);
                // eight predecessors at a time: their 16 LDS reads are in flight together, the comparisons stay in ascending order
                for (; kk + 7 <= hi; kk += 8) {
                    float f[8], l[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) f[i] = prev[kk + i], l[i] = s_lg[kk + i];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const float d = lgk - l[i];
                        const float pd = p.penalty * d;
                        const float tr = pd * d;
                        const float cand = f[i] + tr;
                        if (cand < best) best = cand, bk = kk + i;
                    }
                }
                for (; kk <= hi; ++kk) {
                    const float d = lgk - s_lg[kk];
                    const float pd = p.penalty * d;
                    const float tr = pd * d;
                    const float cand = prev[kk] + tr;
                    if (cand < best) best = cand, bk = kk;
                }
                a = loc + best;
                s_bp[r * n + tid] = (uint16_t)bk;
            }
            float v = act ? a : __builtin_inff();
            int i = tid;
            block_argmin(v, i, s_v, s_i, n_waves);
            fwd = a - v;
            if (act) s_fwd[(t & 1) * n + tid] = fwd;
            __syncthreads();
        }
        if (act)
            for (int r = c0 == 0 ? 1 : 0; r < nc; ++r) bp[(int64_t)(c0 + r) * K + tid] = s_bp[r * n + tid];
    }
    {   // the end state: the smallest k that minimises fwd of the last frame
        float v = act ? fwd : __builtin_inff();
        end = tid;
        block_argmin(v, end, s_v, s_i, n_waves);
    }
    if (tid == 0) s_k = end;
    __syncthreads(); // (also: every back-pointer of the block is written)

    // ---- backtrace, kPitchRows frames at a time from the end
    for (int r1 = T; r1 > 0;) {
        const int r0 = max(0, r1 - kPitchRows), nr = r1 - r0;
        if (act)
            for (int r = 0; r < nr; ++r) s_bp[r * n + tid] = r0 + r > 0 ? bp[(int64_t)(r0 + r) * K + tid] : 0;
        __syncthreads();
        if (tid == 0) {
            int k = s_k;
            for (int r = nr - 1; r >= 0; --r) {
                s_path[r] = k;
                if (r0 + r > 0) k = s_bp[r * n + k];
            }
            s_k = k;
        }
        __syncthreads();
        if (tid < nr) {
            const int t = r0 + tid, k = s_path[tid];
            const float *row = nccf + (int64_t)t * K;
            const float rb = row[k];
            float delta = 0.f;
            if (k > 0 && k < K - 1) {
                const float ra = row[k - 1], rc = row[k + 1];
                const float d1 = ra - rb, d2 = rc - rb;
                const float den = d1 + d2;
                if (den < 0.f) {
                    const float num = ra - rc;
                    const float half = 0.5f * num;
                    delta = half / den;
                    delta = delta < -0.5f ? -0.5f : delta > 0.5f ? 0.5f : delta;
                }
            }
            const int64_t o = sg.out_row0 + t;
            p.index[o] = k;
            p.pitch[2 * o] = (float)(p.lag_min + k) + delta;
            p.pitch[2 * o + 1] = rb;
        }
        __syncthreads(); // (the next round rewrites s_bp and s_path)
        r1 = r0;
    }
}

} // namespace

bool pitch_params_ok(const PitchParams &p)
{
    if (p.window < 32 || p.window > 1024 || p.lag_min < 2 || p.lag_max > 1024 || p.K != p.lag_max - p.lag_min + 1 || p.K < 1 || p.K > 512)
        return false;
    if (p.J < 1 || p.J > 511 || p.shift < 1 || p.tiles.rows < 1 || p.tiles.rows > 64 || (p.channels != 1 && p.channels != 2)) return false;
    if (p.span_pad < 0 || p.span_pad > 63 || (p.groups != 1 && p.groups != 2)) return false;
    if ((int64_t)(p.tiles.rows - 1) * p.shift > (1 << 24)) return false; // (the span arithmetic stays far inside an int)
    return pitch_nccf_lds_bytes(p) <= kLdsMax;
}

size_t pitch_nccf_lds_bytes(const PitchParams &p)
{
    const size_t slots = (size_t)pitch_slots(p.window, p.lag_max, p.shift, p.span_pad, p.tiles.rows);
    return ((size_t)4 * p.groups * pitch_z_floats(p.window, p.lag_max) + 128) * sizeof(float) + ((slots + 7) & ~(size_t)7) * sizeof(int16_t);
}

// frames a wave of k_pitch_nccf takes at a time: a group of 64 / G lanes covers 256 / G lags per pass, so two groups need
// fewer lane slots when the lags fill the last pass of a whole wave badly (K = 281: 3 passes of 128 for two frames, against
// 2 passes of 256 for each)
int pitch_groups(int lag_min, int lag_max)
{
    const int lags = lag_max - (lag_min & ~3) + 1;
    return 2 * ((lags + 255) / 256) > (lags + 127) / 128 ? 2 : 1;
}

hipError_t launch_pitch(const PitchParams &p, hipStream_t stream)
{
    if (p.u1 <= p.u0 || p.tiles.count <= 0) return hipSuccess; // (no utterance of the range has a frame)
    if (!pitch_params_ok(p)) return hipErrorInvalidValue;
    const size_t lds = pitch_nccf_lds_bytes(p);
    if (hipError_t e = allow_dynamic_lds((const void *)k_pitch_nccf, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pitch_nccf, dim3(p.tiles.count), dim3(256), lds, stream, p);
    const int threads = 64 * ((p.K + 63) / 64);
    hipLaunchKernelGGL(k_pitch_track, dim3(p.u1 - p.u0), dim3(threads), pitch_track_lds_bytes(threads), stream, p); // (at most 54 KB)
    return hipGetLastError();
}

} // namespace mfx
