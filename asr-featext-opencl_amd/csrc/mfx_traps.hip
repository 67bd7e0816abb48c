// mfx_traps.hip -- k_traps: TRAPS temporal patterns from stored log mel rows, and its launcher.  See DESIGN.md, "TRAPS".
//
// Per utterance of T frames (M = num_banks, L = traps_len, H = (L - 1) / 2, K = traps_dct_len):
//   u[j]       = x[clamp(t - H + j, 0, T - 1)][m], j < L     the trajectory of band m around frame t
//   y[t][m][k] = sum_j B[k][j] u[j], k < K                   float32, ascending j, one FMA per tap
//   row t      = y[t] band-major: column m * K + k
//
// Layout: grid = (tiles, segments) as k_delta; a block takes R = 64, 32 or 16 consecutive output rows of one utterance
// (the launcher picks the largest whose LDS leaves several blocks per CU).  The tile's rows plus L - 1 clamped context rows
// are staged in LDS one COLUMN per band ([M][RX], RX odd: the lanes' stores fall on different banks), so that the
// trajectory of (t, m) is the RX-strided run col[t .. t + L - 1] and the [R x L] . [L x K] product of a band is Toeplitz
// in its A operand.
//   matrix pipe (default): a wave takes (band, 16 rows, 16 coefficients) at a time, v_mfma_f32_16x16x4_f32 per 4 taps with
//     A[i][k] = col[16 g + i + 4 s + k] read straight from the staged column and B from the operand table in LDS; two
//     such products run interleaved (the instruction's dependent latency is longer than its issue interval).  Taps past L
//     meet zero operands and the column's zero padding.
//   vector ALUs (TrapsParams::valu): a thread takes (row, band), KP = 4 / 16 / 32 accumulators, the basis row of a tap as
//     16-byte broadcast reads.
// Both are the same ascending FMA chain from zero for every output, so they deliver the same bits.
// Finished rows are assembled in LDS as they lie in memory and stored with consecutive lanes on consecutive words, as
// 16-byte words where the pitch, the column count and the pointer allow.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_dev.h"
#include "mfx_launch.h"
#include "mfx_tile_dev.h"

namespace mfx {

namespace {

__host__ __device__ inline int traps_steps(int L) { return (L + 3) >> 2; }
// floats of a staged column: the tile's rows + the taps the padded matrix form reads (>= R + L - 1), odd
__host__ __device__ inline int traps_rx(int R, int L) { return (R + 4 * traps_steps(L)) | 1; }
__host__ __device__ inline int traps_kp(int K) { return K <= 4 ? 4 : K <= 16 ? 16 : 32; }
// floats of the operand table in LDS (a multiple of 4)
__host__ __device__ inline int traps_operand_floats(int L, int K, bool valu)
{
    return valu ? L * traps_kp(K) : ((K + 15) >> 4) * traps_steps(L) * 64;
}

// LDS: s_out [R][M K] | operands | s_x [M][RX]
template <bool VALU, int KP>
__global__ void __launch_bounds__(256) k_traps(TrapsParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Segment sg = p.segs[blockIdx.y];
    const int R = p.tile_rows;
    const int r0 = blockIdx.x * R;
    if (r0 >= sg.n_out) return;
    const int rows = min(R, sg.n_out - r0);
    const int M = p.num_banks, L = p.L, K = p.K, H = (L - 1) >> 1;
    const int cols = M * K;
    const int RX = traps_rx(R, L);
    const int nop = traps_operand_floats(L, K, VALU);
    const int tid = threadIdx.x;
    float *s_out = smem;
    float *s_b = smem + ((R * cols + 3) & ~3);
    float *s_x = s_b + nop;

    for (int i = tid; i < nop; i += 256) s_b[i] = p.operands[i];
    {   // rows r0 - H .. r0 + R + H - 1 of the utterance, clamped to it; zeros behind them
        const int n_ctx = R + L - 1;
        const uint32_t magic = div_magic(M); // floor(i / M) for i < 2^16 (RX * M <= 181 * 256)
        const int n = RX * M;
        for (int i = tid; i < n; i += 256) {
            const int rr = div_small(i, M, magic);
            const int c = i - rr * M;
            float v = 0.f;
            if (rr < n_ctx) {
                const int sr = max(sg.lo, min(sg.hi, r0 + rr - H));
                v = p.src[(sg.src_row0 + sr) * (int64_t)p.src_pitch + c];
            }
            s_x[c * RX + rr] = v;
        }
    }
    __syncthreads();

    if constexpr (VALU) {
        const int lgR = R == 64 ? 6 : R == 32 ? 5 : 4;
        const int n = M << lgR;
        for (int i = tid; i < n; i += 256) {
            const int m = i >> lgR, t = i & (R - 1);
            if (t >= rows) continue;
            float acc[KP];
#pragma unroll
            for (int k = 0; k < KP; ++k) acc[k] = 0.f;
            const float *col = s_x + m * RX + t;
            for (int j = 0; j < L; ++j) {
                const float u = col[j];
                const float4 *b = (const float4 *)(s_b + j * KP);
#pragma unroll
                for (int q = 0; q < KP / 4; ++q) {
                    const float4 w = b[q];
                    acc[4 * q + 0] = __builtin_fmaf(u, w.x, acc[4 * q + 0]);
                    acc[4 * q + 1] = __builtin_fmaf(u, w.y, acc[4 * q + 1]);
                    acc[4 * q + 2] = __builtin_fmaf(u, w.z, acc[4 * q + 2]);
                    acc[4 * q + 3] = __builtin_fmaf(u, w.w, acc[4 * q + 3]);
                }
            }
            float *o = s_out + t * cols + m * K;
#pragma unroll
            for (int k = 0; k < KP; ++k)
                if (k < K) o[k] = acc[k];
        }
    } else {
        const int lane = tid & 63, wave = tid >> 6;
        const int steps = traps_steps(L);
        const int G = (rows + 15) >> 4;      // row groups of 16 that hold output rows
        const int MG = M * G;
        const int nu = MG * ((K + 15) >> 4); // work items: (coefficient tile, row group, band), band fastest
        const int li = lane & 15, lk = lane >> 4;
        for (int u0 = wave * 2; u0 < nu; u0 += 8) {
            int nt[2], g[2], m[2];
            const float *a[2], *b[2];
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const int u = min(u0 + w, nu - 1); // (an odd count: the last item twice, stored once)
                nt[w] = u / MG;
                const int r = u - nt[w] * MG;
                g[w] = r / M;
                m[w] = r - g[w] * M;
                a[w] = s_x + m[w] * RX + 16 * g[w] + li + lk;
                b[w] = s_b + nt[w] * steps * 64 + lane;
            }
            f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
            for (int s = 0; s < steps; ++s) {
                c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][4 * s], b[0][64 * s], c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1][4 * s], b[1][64 * s], c1, 0, 0, 0);
            }
            // D[i][n]: lane holds rows i = 4 (lane >> 4) + r, coefficient n = lane & 15
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                if (w == 1 && u0 + 1 >= nu) break;
                const int k = 16 * nt[w] + li;
                if (k >= K) continue;
                float *o = s_out + (16 * g[w] + 4 * lk) * cols + m[w] * K + k;
                const f32x4 c = w == 0 ? c0 : c1;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (16 * g[w] + 4 * lk + r < rows) o[r * cols] = c[r];
            }
        }
    }
    __syncthreads();

    tile_store_rows(s_out, cols, rows, p.out, sg.out_row0 + r0, p.out_pitch, tid);
}

} // namespace

size_t traps_lds_bytes(const TrapsParams &p, int tile_rows)
{
    const size_t f = (size_t)((tile_rows * p.num_banks * p.K + 3) & ~3) + (size_t)traps_operand_floats(p.L, p.K, p.valu != 0) +
                     (size_t)p.num_banks * traps_rx(tile_rows, p.L);
    return f * sizeof(float);
}

#ifndef MFX_TRAPS_LDS_TARGET
#define MFX_TRAPS_LDS_TARGET kTileLdsTarget
#endif
int traps_tile_rows(const TrapsParams &p)
{
    return tile_rows_for([&](int r) { return traps_lds_bytes(p, r); }, MFX_TRAPS_LDS_TARGET);
}

hipError_t launch_traps(const TrapsParams &p, hipStream_t stream)
{
    if (p.n_segs <= 0 || p.tiles_per_seg_max <= 0) return hipSuccess;
    if (p.num_banks <= 0 || p.K < 1 || p.K > 32 || p.L < 3 || p.L > 101 || !(p.L & 1) || p.K > p.L || p.num_banks * p.K > 256 ||
        p.src_pitch < p.num_banks || p.out_pitch < p.num_banks * p.K)
        return hipErrorInvalidValue;
    const int R = traps_tile_rows(p);
    if (R == 0) return hipErrorInvalidValue;
    const size_t lds = traps_lds_bytes(p, R);
    const int kp = traps_kp(p.K);
    const void *fn = !p.valu   ? (const void *)k_traps<false, 0>
                     : kp == 4 ? (const void *)k_traps<true, 4>
                     : kp == 16 ? (const void *)k_traps<true, 16>
                                : (const void *)k_traps<true, 32>;
    if (hipError_t e = allow_dynamic_lds(fn, lds); e != hipSuccess) return e;
    const int tiles_x = p.tiles_per_seg_max * (64 / R);
    return for_seg_slices(p.n_segs, [&](int s0, int n) {
        TrapsParams q = p;
        q.tile_rows = R;
        q.segs = p.segs + s0;
        q.n_segs = n;
        return launch_kernel(fn, dim3(tiles_x, n), dim3(256), lds, stream, q);
    });
}

} // namespace mfx
