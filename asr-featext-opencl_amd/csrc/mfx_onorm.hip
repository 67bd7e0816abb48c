// mfx_onorm.hip -- the online (causal, sliding-window) CMN / CVN of the batch entries (mfx_batch_set_online_norm) and of the
// session entries (mfx_sessions_set_online_norm), and their launchers:
//   k_onorm_totals   per (chunk of kOnormChunk = 32 rows, column): the chunk's totals of v and of q = (double)(float)(v * v)
//   k_onorm_offsets  per (utterance, column): the totals turned into the exclusive ascending chain O, in place
//   k_onorm_apply    per chunk: lead chain, trail chain (chunk c - N / 32), statistics, write
//   k_onorm_sess     per (session, column): the same chains carried from push to push, with a ring of the last N raw rows
// Every sum has one owner and a fixed order (include/mfx.h states it); nothing is atomic.  mfx_onorm_dev.h holds the
// arithmetic all four share.  See DESIGN.md section 5, "Online normalisation"; the batch kernels' chunks are an utterance tiling
// (UttTiling, mfx_kernels.h; utt_item, mfx_dev.h).
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_dev.h"
#include "mfx_launch.h"
#include "mfx_onorm_dev.h"

#include <algorithm>

namespace mfx {

namespace {

// (the block's tiles, G = onorm_tiles(Wn) of them, and their LDS image: mfx_onorm_dev.h)

// first row (absolute), row count and local index of chunk c
__device__ __forceinline__ void onorm_chunk(const OnormParams &p, int c, int64_t &row0, int &rows, int &lc)
{
    const UttItem ch = utt_item<kOnormChunk>(p.chunks, p.segs, c);
    lc = ch.local;
    row0 = ch.row0 + ch.t0;
    rows = ch.n;
}

// grid = ceil(n_chunks / G), 256 threads.  Lanes of consecutive j read consecutive floats of a row.
__global__ void __launch_bounds__(256) k_onorm_totals(OnormParams p)
{
    const int Wn = p.Wn, G = onorm_tiles(Wn);
    const int g = threadIdx.x / Wn, j = threadIdx.x - g * Wn;
    const int ci = blockIdx.x * G + g;
    if (g >= G || ci >= p.chunks.count) return;
    const int c = p.chunks.first + ci;
    int64_t row0;
    int rows, lc;
    onorm_chunk(p, c, row0, rows, lc);
    const float *q = p.src + row0 * (int64_t)p.src_pitch + j;
    // all of the chunk's loads are in flight before the chain waits for the first: a load per link would leave the kernel at
    // 32 memory latencies per block.  (Rows past the utterance's end are neither read nor added: -0.0 + 0.0 is not -0.0.)
    float v[kOnormChunk];
#pragma unroll
    for (int r = 0; r < kOnormChunk; ++r) v[r] = r < rows ? q[(int64_t)r * p.src_pitch] : 0.f;
    double Iv = 0.0, Iq = 0.0;
#pragma unroll
    for (int r = 0; r < kOnormChunk; ++r)
        if (r < rows) {
            Iv = onorm_add(Iv, (double)v[r]);
            Iq = onorm_add(Iq, onorm_sq(v[r]));
        }
    double *t = p.tot + (int64_t)c * 2 * Wn + j;
    t[0] = Iv;
    t[Wn] = Iq;
}

// one thread per (utterance, v | q, column): O[0] = 0, O[c + 1] = O[c] + Tot[c], ascending; slot c ends up holding O[c].
// Four totals are read ahead of the four dependent additions, so that the loads of a long stream overlap.
__global__ void __launch_bounds__(256) k_onorm_offsets(OnormParams p)
{
    const int per = 2 * p.Wn;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)p.n_utt * per) return;
    const int u = p.u0 + (int)(i / per), k = (int)(i % per);
    const int c0 = p.chunks.utt_item0[u], c1 = p.chunks.utt_item0[u + 1];
    double *t = p.tot + (int64_t)c0 * per + k;
    double O = 0.0;
    int c = c0;
    for (; c + 4 <= c1; c += 4, t += 4 * (int64_t)per) {
        const double a = t[0], b = t[per], d = t[2 * (int64_t)per], e = t[3 * (int64_t)per];
        t[0] = O;
        O = onorm_add(O, a);
        t[per] = O;
        O = onorm_add(O, b);
        t[2 * (int64_t)per] = O;
        O = onorm_add(O, d);
        t[3 * (int64_t)per] = O;
        O = onorm_add(O, e);
    }
    for (; c < c1; ++c, t += per) {
        const double a = t[0];
        t[0] = O;
        O = onorm_add(O, a);
    }
}

// grid = ceil(n_chunks / G), 256 threads, dynamic LDS: the tiles' descriptors and the lead tiles [32][G * Wn].  Row r of ALL
// the block's tiles is one run of G * Wn floats, so the column walk of thread tid reads word r * G * Wn + tid: the lanes of a
// wave touch consecutive words at every width (no bank conflict, no padding needed), and the staging loops walk the same
// words in order: HBM is read and written in whole row pieces of Wn floats.  The trail tile goes straight into the column
// thread's registers (the lanes of a wave still read whole row pieces): with it in LDS as well a block held 64 KB, two
// blocks fitted a CU, and the kernel waited on memory with 8 waves per CU.
__global__ void __launch_bounds__(256) k_onorm_apply(OnormParams p)
{
    extern __shared__ int64_t s_dyn[]; // row0 [G] | rows [G] | local chunk [G] | lead tiles
    const int Wn = p.Wn, G = onorm_tiles(Wn), GW = G * Wn;
    const int tid = threadIdx.x;
    const int back = p.window / kOnormChunk; // chunks between a lead chunk and its trail chunk
    int64_t *s_row0 = s_dyn;
    int32_t *s_rows = (int32_t *)(s_row0 + G), *s_lc = s_rows + G;
    float *lead = (float *)(s_lc + G);
    if (tid < G) {
        const int ci = blockIdx.x * G + tid;
        int64_t row0 = 0;
        int rows = 0, lc = 0;
        if (ci < p.chunks.count) onorm_chunk(p, p.chunks.first + ci, row0, rows, lc);
        s_row0[tid] = row0, s_rows[tid] = rows, s_lc[tid] = lc;
    }
    __syncthreads();
    const int g = tid / Wn, j = tid - g * Wn;
    const bool mine = g < G && s_rows[g] > 0;
    const bool windowed = mine && back > 0 && s_lc[g] >= back;
    // the trail rows of this thread's column: an earlier chunk of the same utterance, so all of its 32 rows exist.  Issued
    // ahead of the lead tile's staging, which they overlap.
    float w[kOnormChunk];
    if (windowed) {
        const float *tsrc = p.src + (s_row0[g] - p.window) * (int64_t)p.src_pitch + j;
#pragma unroll
        for (int r = 0; r < kOnormChunk; ++r) w[r] = tsrc[(int64_t)r * p.src_pitch];
    } else {
#pragma unroll
        for (int r = 0; r < kOnormChunk; ++r) w[r] = 0.f;
    }
    const OnormTileIndex ix(Wn, G);
    onorm_tiles_load(ix, p.src, p.src_pitch, s_row0, s_rows, lead, tid);
    __syncthreads();
    if (mine) {
        const int lc = s_lc[g];
        const int c = p.chunks.first + blockIdx.x * G + g;
        OnormStat st;
        st.cvn = p.cvn, st.prior_frames = p.prior_frames, st.prior_count = p.prior_count;
        const double ps = p.prior_count > 0 ? p.prior_acc[j] : 0.0, pq = p.prior_count > 0 ? p.prior_acc[Wn + j] : 0.0;
        const double *o = p.tot + (int64_t)c * 2 * Wn + j;
        const double Olv = o[0], Olq = o[Wn];
        double Otv = 0.0, Otq = 0.0;
        if (windowed) {
            const double *ot = o - (int64_t)back * 2 * Wn;
            Otv = ot[0], Otq = ot[Wn];
        }
        double Ilv = 0.0, Ilq = 0.0, Itv = 0.0, Itq = 0.0;
        // (all 32 rows whatever the tile holds: the staging left zeros behind its last row and nothing stores them; the
        // fixed trip count keeps w[] in registers and lets the rows' divisions overlap, while the chains themselves stay
        // one addition after the other)
#pragma unroll
        for (int r = 0; r < kOnormChunk; ++r) {
            const float v = lead[r * GW + tid];
            Ilv = onorm_add(Ilv, (double)v);
            Ilq = onorm_add(Ilq, onorm_sq(v));
            double Sw = onorm_add(Olv, Ilv), Qw = onorm_add(Olq, Ilq);
            int64_t n = (int64_t)lc * kOnormChunk + r + 1;
            if (windowed) {
                Itv = onorm_add(Itv, (double)w[r]);
                Itq = onorm_add(Itq, onorm_sq(w[r]));
                Sw = onorm_sub(Sw, onorm_add(Otv, Itv));
                Qw = onorm_sub(Qw, onorm_add(Otq, Itq));
                n = p.window;
            }
            lead[r * GW + tid] = onorm_row(v, Sw, Qw, n, st, ps, pq);
        }
    }
    __syncthreads();
    onorm_tiles_store(ix, p.out, p.out_pitch, s_row0, s_rows, lead, tid);
}

// one thread per (descriptor, column): the push's rows in ascending order, in place.  Slot t mod N of the ring holds raw row
// t - N just when row t needs it, and takes row t afterwards; a push longer than N rows walks the ring more than once.
__global__ void __launch_bounds__(256) k_onorm_sess(OnormSessParams p)
{
    const int Wn = p.Wn;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)p.n_descs * Wn) return;
    const int di = (int)(i / Wn), j = (int)(i - (int64_t)di * Wn);
    const OnormSessDesc d = p.descs[di];
    if (d.n_rows <= 0) return;
    const int N = p.window;
    double *s = p.state + (int64_t)d.session * 8 * Wn + j;
    double Olv = 0.0, Olq = 0.0, Ilv = 0.0, Ilq = 0.0, Otv = 0.0, Otq = 0.0, Itv = 0.0, Itq = 0.0;
    if (d.t0 > 0) {
        Olv = s[0], Olq = s[Wn], Ilv = s[2 * Wn], Ilq = s[3 * Wn];
        Otv = s[4 * Wn], Otq = s[5 * Wn], Itv = s[6 * Wn], Itq = s[7 * Wn];
    }
    OnormStat st;
    st.cvn = p.cvn, st.prior_frames = p.prior_frames, st.prior_count = p.prior_count;
    const double ps = p.prior_count > 0 ? p.prior_acc[j] : 0.0, pq = p.prior_count > 0 ? p.prior_acc[Wn + j] : 0.0;
    float *ring = N > 0 ? p.ring + (int64_t)d.session * N * Wn + j : nullptr;
    float *q = p.data + d.row0 * (int64_t)p.pitch + j;
    int slot = N > 0 ? (int)(d.t0 % N) : 0;
    int64_t t = d.t0;
    for (int r = 0; r < d.n_rows; ++r, ++t, q += p.pitch) {
        const float v = *q;
        Ilv = onorm_add(Ilv, (double)v);
        Ilq = onorm_add(Ilq, onorm_sq(v));
        double Sw = onorm_add(Olv, Ilv), Qw = onorm_add(Olq, Ilq);
        int64_t n = t + 1;
        if (N > 0) {
            float *rs = ring + (int64_t)slot * Wn;
            if (t >= N) {
                const float w = *rs;
                Itv = onorm_add(Itv, (double)w);
                Itq = onorm_add(Itq, onorm_sq(w));
                Sw = onorm_sub(Sw, onorm_add(Otv, Itv));
                Qw = onorm_sub(Qw, onorm_add(Otq, Itq));
                n = N;
                if (((t - N) & (kOnormChunk - 1)) == kOnormChunk - 1) {
                    Otv = onorm_add(Otv, Itv), Otq = onorm_add(Otq, Itq);
                    Itv = 0.0, Itq = 0.0;
                }
            }
            *rs = v;
            if (++slot == N) slot = 0;
        }
        if ((t & (kOnormChunk - 1)) == kOnormChunk - 1) {
            Olv = onorm_add(Olv, Ilv), Olq = onorm_add(Olq, Ilq);
            Ilv = 0.0, Ilq = 0.0;
        }
        *q = onorm_row(v, Sw, Qw, n, st, ps, pq);
    }
    s[0] = Olv, s[Wn] = Olq, s[2 * Wn] = Ilv, s[3 * Wn] = Ilq;
    s[4 * Wn] = Otv, s[5 * Wn] = Otq, s[6 * Wn] = Itv, s[7 * Wn] = Itq;
}

bool onorm_shape_ok(int Wn, int window, int prior_frames, int64_t prior_count, const double *prior_acc)
{
    return Wn >= 1 && Wn <= 256 && window >= 0 && window <= 4096 && window % kOnormChunk == 0 && prior_frames >= 0 && prior_count >= 0 &&
           (prior_count == 0 || prior_acc != nullptr);
}

} // namespace

// k_onorm_totals, then k_onorm_offsets: p.tot holds the offsets O of v and q of every chunk of the range.  Reads src, src_pitch,
// Wn, segs, chunks, tot, u0, n_utt of `p` (the sliding-window normaliser, mfx_slide.hip, builds its sums on the same chains).
hipError_t launch_onorm_prefix(const OnormParams &p, hipStream_t stream)
{
    if (p.n_utt <= 0 || p.chunks.count <= 0) return hipSuccess;
    if (p.Wn < 1 || p.Wn > 256 || p.src_pitch < p.Wn || p.chunks.rows != kOnormChunk) return hipErrorInvalidValue;
    const int G = p.Wn >= 256 ? 1 : 256 / p.Wn;
    const int blocks = (p.chunks.count + G - 1) / G;
    hipLaunchKernelGGL(k_onorm_totals, dim3(blocks), dim3(256), 0, stream, p);
    const int64_t chains = (int64_t)p.n_utt * 2 * p.Wn;
    hipLaunchKernelGGL(k_onorm_offsets, dim3((unsigned)((chains + 255) / 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_onorm(const OnormParams &p, hipStream_t stream)
{
    if (p.n_utt <= 0 || p.chunks.count <= 0) return hipSuccess;
    if (!onorm_shape_ok(p.Wn, p.window, p.prior_frames, p.prior_count, p.prior_acc) || p.src == p.out || p.src_pitch < p.Wn ||
        p.out_pitch < p.Wn || p.chunks.rows != kOnormChunk) // (the chunk size is the kernels' constant)
        return hipErrorInvalidValue;
    const int G = p.Wn >= 256 ? 1 : 256 / p.Wn;
    const int blocks = (p.chunks.count + G - 1) / G;
    if (hipError_t e = launch_onorm_prefix(p, stream); e != hipSuccess) return e;
    const size_t lds = (size_t)G * 16 + (size_t)kOnormChunk * G * p.Wn * sizeof(float); // descriptors + lead tiles: <= 36 KB
    hipLaunchKernelGGL(k_onorm_apply, dim3(blocks), dim3(256), lds, stream, p);
    return hipGetLastError();
}

hipError_t launch_onorm_sess(const OnormSessParams &p, hipStream_t stream)
{
    if (p.n_descs <= 0) return hipSuccess;
    if (!onorm_shape_ok(p.Wn, p.window, p.prior_frames, p.prior_count, p.prior_acc) || p.pitch < p.Wn || (p.window > 0 && !p.ring))
        return hipErrorInvalidValue;
    const int64_t threads = (int64_t)p.n_descs * p.Wn;
    hipLaunchKernelGGL(k_onorm_sess, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

} // namespace mfx
