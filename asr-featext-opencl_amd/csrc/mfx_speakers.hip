// mfx_speakers.hip -- per-speaker CMN / CVN / MINMAX of the batch entries (mfx_batch_set_speakers), and their launchers:
//   k_spk_sums    per-column totals of every 4096-row chunk of every utterance, formed as k_norm_stats forms a segment's
//   k_spk_finish  one block per speaker: prior, then the speaker's utterances in ascending order -> accumulator, statistics
//   k_spk_apply   (v - mean[spk]) [* multiplier[spk]] in place over every row of the batch
// Nothing here is atomic and no result depends on timing: every sum has one owner and a fixed order.
// See DESIGN.md section 5, "Per-speaker normalisation".
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_launch.h"
#include "mfx_norm_dev.h"

namespace mfx {

namespace {

constexpr int kSpkTileFloats = 8192; // k_spk_apply: floats of a tile (whole rows); below 2^16 for the multiply-high division

// grid = (row chunk, utterance, column group); block = 256 threads in k_norm_stats' mapping.  The totals of chunk k of
// utterance u land in partial[utt_chunk0[u] + k][4][Wn] (S, S2, min, max) at the group's columns.
__global__ void __launch_bounds__(256) k_spk_sums(SpkParams p)
{
    __shared__ double s_sum[256], s_sum2[256];
    __shared__ float s_min[256], s_max[256];
    const int u = p.u0 + blockIdx.y;
    const Segment sg = p.segs[u];
    const int T = sg.n_out;
    const int r0 = blockIdx.x * kNormChunkRows;
    if (r0 >= T) return;
    const int r1 = min(T, r0 + kNormChunkRows);
    const int cols = p.cols, Wn = p.cols * p.groups;
    const int lg = norm_lg(cols);
    const int tid = threadIdx.x, rr = tid >> lg, c = tid & ((1 << lg) - 1);
    const float *base = p.data + sg.out_row0 * (int64_t)p.pitch + blockIdx.z * cols;
    norm_rows_totals<false>([&](int r, int cc) { return base[(int64_t)r * p.pitch + cc]; }, r0, r1, cols, lg, tid, s_sum, s_sum2, s_min,
                            s_max);
    if (rr == 0 && c < cols) {
        double *q = p.partial + ((int64_t)p.utt_chunk0[u] + blockIdx.x) * 4 * Wn + blockIdx.z * cols;
        q[c] = s_sum[tid];
        q[Wn + c] = s_sum2[tid];
        q[2 * Wn + c] = (double)s_min[tid];
        q[3 * Wn + c] = (double)s_max[tid];
    }
}

// grid = speakers; a thread owns columns tid, tid + 256, ... of the Wn.  An utterance's totals are its one chunk's as they
// are, or its chunks' combined in ascending order from zero as k_norm_finalize combines them; the speaker's accumulator
// starts from its prior (a prior of count 0 is no prior), else from its first utterance's totals as they are, and takes
// the remaining utterances in list order (ascending utterance index).
__global__ void __launch_bounds__(256) k_spk_finish(SpkParams p)
{
    const int s = blockIdx.x;
    const int Wn = p.cols * p.groups;
    const bool prior = p.prior_count != nullptr && p.prior_count[s] > 0;
    const bool pool = p.mode == 0;
    const int k0 = p.spk_off[s], k1 = pool ? p.spk_off[s + 1] : k0;
    int64_t n = prior ? p.prior_count[s] : 0;
    for (int k = k0; k < k1; ++k) n += p.segs[p.spk_list[k]].n_out;
    if (threadIdx.x == 0) p.count[s] = n;
    const double *pa = prior ? p.prior_acc + (int64_t)s * 4 * Wn : nullptr;
    double *acc = p.acc + (int64_t)s * 4 * Wn;
    float *st = p.stats + (int64_t)s * 2 * Wn;
    for (int c = threadIdx.x; c < Wn; c += 256) {
        double S = 0, S2 = 0;
        float mn = 3.402823466e+38f, mx = -3.402823466e+38f;
        bool first = !prior;
        if (prior) {
            S = pa[c];
            S2 = pa[Wn + c];
            mn = (float)pa[2 * Wn + c];
            mx = (float)pa[3 * Wn + c];
        }
        for (int k = k0; k < k1; ++k) {
            const int u = p.spk_list[k];
            const int ch0 = p.utt_chunk0[u], nch = p.utt_chunk0[u + 1] - ch0;
            const double *q = p.partial + (int64_t)ch0 * 4 * Wn;
            double tS = q[c], tS2 = q[Wn + c];
            float tmn = (float)q[2 * Wn + c], tmx = (float)q[3 * Wn + c];
            if (nch > 1) {
                tS = 0, tS2 = 0;
                tmn = 3.402823466e+38f, tmx = -3.402823466e+38f;
                for (int j = 0; j < nch; ++j, q += 4 * Wn) {
                    tS += q[c];
                    tS2 += q[Wn + c];
                    tmn = fminf(tmn, (float)q[2 * Wn + c]);
                    tmx = fmaxf(tmx, (float)q[3 * Wn + c]);
                }
            }
            if (first) {
                S = tS, S2 = tS2, mn = tmn, mx = tmx;
                first = false;
            } else {
                S += tS;
                S2 += tS2;
                mn = fminf(mn, tmn);
                mx = fmaxf(mx, tmx);
            }
        }
        acc[c] = S;
        acc[Wn + c] = S2;
        acc[2 * Wn + c] = (double)mn;
        acc[3 * Wn + c] = (double)mx;
        norm_finish_to(st, Wn, p.norm_type, c, (double)n, S, S2, mn, mx);
    }
}

// grid = tiles of whole rows of one utterance (at most kSpkTileFloats floats); consecutive threads take consecutive floats
// of a row.  The arithmetic is k_norm_apply's float32 expression.
__global__ void __launch_bounds__(256) k_spk_apply(SpkParams p)
{
    __shared__ float s_st[2 * 768];
    const SpkTile t = p.tiles[blockIdx.x];
    const int Wn = p.cols * p.groups;
    const float *st = p.stats + (int64_t)t.spk * 2 * Wn;
    for (int i = threadIdx.x; i < 2 * Wn; i += 256) s_st[i] = st[i];
    __syncthreads();
    float *base = p.data + t.row0 * (int64_t)p.pitch;
    const int total = t.rows * Wn;
    // i / Wn for i < 2^16.  Wn == 1 would wrap the constant to 0: one column takes the shift form (as k_norm_seg)
    const uint32_t magic = Wn > 1 ? 0xffffffffu / (uint32_t)Wn + 1 : 0;
    const bool cmn = p.norm_type == 1;
#pragma unroll 4
    for (int i = threadIdx.x; i < total; i += 256) {
        const int r = Wn > 1 ? (int)__umulhi((uint32_t)i, magic) : i;
        const int c = i - r * Wn;
        float *q = base + (int64_t)r * p.pitch + c;
        const float v = *q;
        *q = cmn ? v - s_st[c] : (v - s_st[c]) * s_st[Wn + c];
    }
}

} // namespace

int spk_tile_rows(int wn) { return wn > 0 && wn <= kSpkTileFloats ? kSpkTileFloats / wn : 1; }

int spk_chunks(int64_t rows) { return (int)((rows + kNormChunkRows - 1) / kNormChunkRows); }

static bool spk_shape_ok(const SpkParams &p) { return p.cols >= 1 && p.cols <= 256 && p.groups >= 1 && p.groups <= 3; }

hipError_t launch_spk_sums(const SpkParams &p, hipStream_t stream)
{
    if (p.n_utt <= 0 || p.max_rows <= 0) return hipSuccess;
    if (!spk_shape_ok(p)) return hipErrorInvalidValue;
    const int chunks = spk_chunks(p.max_rows);
    return for_seg_slices(p.n_utt, [&](int u0, int n) {
        SpkParams q = p;
        q.u0 = u0;
        return launch_kernel((const void *)k_spk_sums, dim3(chunks, n, p.groups), dim3(256), 0, stream, q);
    });
}

hipError_t launch_spk_finish(const SpkParams &p, hipStream_t stream)
{
    if (p.n_spk <= 0) return hipSuccess;
    if (!spk_shape_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_spk_finish, dim3(p.n_spk), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_spk_apply(const SpkParams &p, hipStream_t stream)
{
    if (p.n_tiles <= 0) return hipSuccess;
    if (!spk_shape_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_spk_apply, dim3(p.n_tiles), dim3(256), 0, stream, p);
    return hipGetLastError();
}

} // namespace mfx
