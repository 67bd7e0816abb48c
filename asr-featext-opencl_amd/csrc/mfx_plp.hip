// mfx_plp.hip -- k_plp: PLP cepstra from stored magnitude rows (the PLP counterpart of k_melcep, mfx_tail.hip), and its
// launcher.  See DESIGN.md, "PLP".
//
// Per frame (M = num_banks, p = lpc_order, C = ceps_len, N = M + 2):
//   P[j] = v[j]^2                                   power of the stored magnitude (the MFCC path's |X_j| / W2)
//   E_m  = max(sum_j T[m%2][j] P[j], 1e-30)         the MFCC mel table and summation order, on power
//   A_m  = (e_m E_m)^(1/3), A_0 = A_1, A_{N-1} = A_M equal loudness (e_m per table: the centres move with alpha), cube root
//   r_i  = sum_m idft[i][m] A_m                     inverse DFT of the real even spectrum, i = 0 .. p
//   Levinson-Durbin -> a_1 .. a_p, E^p; c_0 = ln E^p, c_n = -a_n - sum_k (k / n) c_k a_{n-k}
//   row = [w_1 c_1 .. w_C c_C (, c_0)]
//
// Layout: a wave takes 64 consecutive rows.  Phase 1 walks their filterbanks one row at a time on the wave's 64 lanes
// (MelWavePlan, mel64_walk_log without the log) into LDS rows of RP floats (RP odd: lane l's row is bank-disjoint from its
// neighbours'), E_m at word m + 1.  Phase 2 gives each lane one row: cube roots, the autocorrelation, the recursion and
// the cepstrum run in registers (a[], r[] unrolled to PMAX), c_n goes back to the lane's LDS row, and the wave then writes
// the 64 rows out with consecutive lanes on consecutive words.  blockIdx.y = filterbank of a VTLN sweep.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_dev.h"
#include "mfx_launch.h"

#include <algorithm>

namespace mfx {

namespace {

constexpr int kPlpRows = 64; // rows per wave (one per lane in phase 2)

__host__ __device__ inline int plp_pmax(int p) { return p <= 8 ? 8 : p <= 16 ? 16 : 32; }
// floats per basis row in LDS: [N][PS], PS a multiple of 4 > PMAX (16-byte broadcast reads, zeros past p)
__host__ __device__ constexpr int plp_ps(int pmax) { return (pmax + 4) & ~3; }
// floats per lane row: holds E_1 .. E_M at words 1 .. M (word 0 parks idle walk lanes) and later c_1 .. c_C / the output row
__host__ __device__ inline int plp_rp(int nb, int ceps)
{
    int x = std::max(nb + 2, ceps + 1);
    return x | 1;
}

// x^(1/3) for a positive normal x: v_log_f32 / v_exp_f32 (relative error ~1e-6 over the range of e_m E_m)
__device__ __forceinline__ float plp_cbrt(float x) { return __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(x) * (1.0f / 3.0f)); }

template <int PMAX>
__global__ void __launch_bounds__(256) k_plp(PlpParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n_waves = blockDim.x >> 6;
    const int nb = p.num_banks, RS = p.mel64_row_stride, rounds = p.mel64_rounds, MF = p.mag_floats;
    const int N = nb + 2, order = p.lpc_order, C = p.ceps_len;
    constexpr int PS = plp_ps(PMAX);
    const int RP = plp_rp(nb, C);
    const int WR = mel64_rows(nb);
    float *s_mw = smem;                              // [WR][RS]
    int *s_mst = (int *)(s_mw + WR * RS);            // [rounds][64]
    int *s_mfid = s_mst + 64 * rounds;               // [rounds][64]
    int *s_L = s_mfid + 64 * rounds;                 // [8]
    float *s_idft = (float *)(s_L + 8);              // [N][PS]
    float *s_eql = s_idft + N * PS;                  // [nb, x4]
    float *s_lift = s_eql + ((nb + 3) & ~3);         // [C, x4]
    float *s_wave = s_lift + ((C + 3) & ~3) + wave * (MF + kPlpRows * RP);
    float *mag = s_wave, *rows = s_wave + MF;

    const int table = blockIdx.y;
    const float *gw = p.mel64_w + (int64_t)table * 64 * RS;
    const int32_t *gst = p.mel64_start + (int64_t)table * 64 * rounds, *gfid = p.mel64_fid + (int64_t)table * 64 * rounds;
    const float *geql = p.eql + (int64_t)table * nb;
    float *feat = p.feat + (int64_t)table * p.feat_table_stride;
    float *r_out = table == 0 ? p.r_out : nullptr;
    for (int i = tid; i < WR * RS; i += blockDim.x) s_mw[i] = gw[i];
    for (int i = tid; i < 64 * rounds; i += blockDim.x) {
        s_mst[i] = gst[i];
        s_mfid[i] = gfid[i];
    }
    if (tid < 8) s_L[tid] = p.mel64_L[table * 8 + tid];
    for (int i = tid; i < N * PS; i += blockDim.x) { // transposed: one 16-byte broadcast read per band and 4 orders
        const int m = i / PS, k = i - m * PS;
        s_idft[i] = k <= order ? p.idft[k * N + m] : 0.f;
    }
    for (int i = tid; i < nb; i += blockDim.x) s_eql[i] = geql[i];
    for (int i = tid; i < C; i += blockDim.x) s_lift[i] = p.lift[i];
    for (int i = lane; i < MF; i += 64) mag[i] = 0.f; // words past the last bin stay zero (finite) for good
    __syncthreads();

    const int q4 = p.spec_pitch >> 2;
    const int nbins = (p.fft_size >> 1) + 1;
    const int cols = p.cols;
    for (int64_t grp = (int64_t)blockIdx.x * n_waves + wave; grp * kPlpRows < p.n_rows; grp += (int64_t)gridDim.x * n_waves) {
        const int64_t row0 = grp * kPlpRows;
        const int count = (int)(p.n_rows - row0 < kPlpRows ? p.n_rows - row0 : kPlpRows);
        // ---- phase 1: filterbank energies of the power spectrum, one row at a time on the whole wave
        for (int f = 0; f < count; ++f) {
            const float4 *src = (const float4 *)(p.spec + (row0 + f) * p.spec_pitch);
            for (int k = lane; k < q4; k += 64) {
                const float4 v = src[k];
                ((float4 *)mag)[k] = make_float4(v.x * v.x, v.y * v.y, v.z * v.z, v.w * v.w);
            }
            if (nbins + lane < 4 * q4) mag[nbins + lane] = 0.f; // padding words are never written in memory
            wave_sync();
            mel64_walk_log<false>(mag, rows + f * RP + 1, -1, s_mw, s_mst, s_mfid, s_L, rounds, RS, lane, WR);
            wave_sync();
        }
        // ---- phase 2: lane = row
        if (lane < count) {
            float *row = rows + lane * RP;
            float r[PMAX + 1];
#pragma unroll
            for (int i = 0; i <= PMAX; ++i) r[i] = 0.f;
            auto add_band = [&](int m, float am) {
                const float4 *b = (const float4 *)(s_idft + m * PS);
#pragma unroll
                for (int i4 = 0; i4 < PS / 4; ++i4) {
                    const float4 w = b[i4];
                    if (4 * i4 + 0 <= PMAX) r[4 * i4 + 0] = __builtin_fmaf(w.x, am, r[4 * i4 + 0]);
                    if (4 * i4 + 1 <= PMAX) r[4 * i4 + 1] = __builtin_fmaf(w.y, am, r[4 * i4 + 1]);
                    if (4 * i4 + 2 <= PMAX) r[4 * i4 + 2] = __builtin_fmaf(w.z, am, r[4 * i4 + 2]);
                    if (4 * i4 + 3 <= PMAX) r[4 * i4 + 3] = __builtin_fmaf(w.w, am, r[4 * i4 + 3]);
                }
            };
            const float a1 = plp_cbrt(s_eql[0] * row[1]);
            add_band(0, a1); // A_0 = A_1
            add_band(1, a1);
            float am = a1;
            for (int m = 2; m <= nb; ++m) {
                am = plp_cbrt(s_eql[m - 1] * row[m]);
                add_band(m, am);
            }
            add_band(N - 1, am); // A_{N-1} = A_M
            if (r_out) {
                float *ro = r_out + (row0 + lane) * (int64_t)(order + 1);
#pragma unroll
                for (int i = 0; i <= PMAX; ++i)
                    if (i <= order) ro[i] = r[i];
            }
            // Levinson-Durbin, A(z) = 1 + sum a_j z^-j
            float a[PMAX + 1];
#pragma unroll
            for (int j = 0; j <= PMAX; ++j) a[j] = 0.f;
            float E = r[0];
#pragma unroll
            for (int i = 1; i <= PMAX; ++i) {
                if (i <= order) { // (uniform)
                    float acc = r[i];
#pragma unroll
                    for (int j = 1; j < i; ++j) acc = __builtin_fmaf(a[j], r[i - j], acc);
                    const float k = -acc / E;
                    float na[PMAX + 1];
#pragma unroll
                    for (int j = 1; j < i; ++j) na[j] = __builtin_fmaf(k, a[i - j], a[j]);
#pragma unroll
                    for (int j = 1; j < i; ++j) a[j] = na[j];
                    a[i] = k;
                    E *= 1.f - k * k;
                }
            }
            const float c0 = MFX_LOG(E);
            // cepstrum: c_n = -a_n - (1/n) sum_{j=1}^{min(p, n-1)} (n - j) c_{n-j} a_j; c_n at row[n]
            for (int n = 1; n <= C; ++n) {
                float s = 0.f, an = 0.f;
#pragma unroll
                for (int j = 1; j <= PMAX; ++j) {
                    if (j == n) an = a[j];
                    if (j < n && j <= order) s = __builtin_fmaf((float)(n - j) * row[n - j], a[j], s);
                }
                row[n] = -an - s / (float)n;
            }
            // lifted row in place: [w_1 c_1 .. w_C c_C (, c_0)]
            for (int n = 1; n <= C; ++n) row[n - 1] = s_lift[n - 1] * row[n];
            if (p.want_c0) row[C] = c0;
        }
        wave_sync();
        // ---- rows out: consecutive lanes on consecutive words of each row
        for (int i = lane; i < count * cols; i += 64) {
            const int rr = i / cols, cc = i - rr * cols;
            feat[(row0 + rr) * (int64_t)p.feat_pitch + cc] = rows[rr * RP + cc];
        }
        wave_sync();
    }
}

template <int PMAX>
size_t plp_lds_bytes_t(const PlpParams &p, int n_waves)
{
    const size_t nb = (size_t)p.num_banks;
    const size_t f = (size_t)mel64_rows(p.num_banks) * p.mel64_row_stride + (size_t)128 * p.mel64_rounds + 8 +
                     (nb + 2) * plp_ps(PMAX) + ((nb + 3) & ~(size_t)3) + (((size_t)p.ceps_len + 3) & ~(size_t)3) +
                     (size_t)n_waves * ((size_t)p.mag_floats + (size_t)kPlpRows * plp_rp(p.num_banks, p.ceps_len));
    return f * sizeof(float);
}

template <int PMAX>
hipError_t launch_plp_t(const PlpParams &p, hipStream_t stream)
{
    int nw = 4; // waves per block: as many of 4 as the LDS holds
    while (nw > 1 && plp_lds_bytes_t<PMAX>(p, nw) > 160 * 1024) nw >>= 1;
    const size_t lds = plp_lds_bytes_t<PMAX>(p, nw);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const void *fn = (const void *)k_plp<PMAX>;
    if (hipError_t e = allow_dynamic_lds(fn, lds); e != hipSuccess) return e;
    int64_t blocks = ((p.n_rows + kPlpRows - 1) / kPlpRows + nw - 1) / nw;
    int per_cu = blocks_per_cu(fn, 64 * nw, lds, (int)std::min<size_t>(4, (160 * 1024) / lds));
    if (per_cu > 8) per_cu = 8;
    const int cap = num_cus() * (per_cu < 1 ? 1 : per_cu);
    if (blocks > cap) blocks = cap;
    const int tables = p.n_tables > 1 ? p.n_tables : 1;
    if (tables > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_plp<PMAX>, dim3((unsigned)blocks, (unsigned)tables), dim3(64 * nw), lds, stream, p);
    return hipGetLastError();
}

} // namespace

size_t plp_lds_bytes(const PlpParams &p, int n_waves)
{
    switch (plp_pmax(p.lpc_order)) {
    case 8: return plp_lds_bytes_t<8>(p, n_waves);
    case 16: return plp_lds_bytes_t<16>(p, n_waves);
    default: return plp_lds_bytes_t<32>(p, n_waves);
    }
}

hipError_t launch_plp(const PlpParams &p, hipStream_t stream)
{
    if (p.n_rows <= 0) return hipSuccess;
    if (p.mag_floats < p.spec_pitch || (p.spec_pitch & 3) || (p.mag_floats & 3)) return hipErrorInvalidValue;
    if (p.lpc_order < 1 || p.lpc_order > kPlpMaxOrder || p.ceps_len < 1 || p.num_banks < 1) return hipErrorInvalidValue;
    switch (plp_pmax(p.lpc_order)) {
    case 8: return launch_plp_t<8>(p, stream);
    case 16: return launch_plp_t<16>(p, stream);
    default: return launch_plp_t<32>(p, stream);
    }
}

} // namespace mfx
