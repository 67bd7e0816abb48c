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
// (MelPlan, mel64_walk_log without the log) into LDS rows of RP floats (RP odd: lane l's row is bank-disjoint from its
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

// The kernel's text is mfx_plp_body.h: compiled here as k_plp and as its row-run form k_plp_runs.  (As a function template over
// a row-group iterator, the form k_melcep has, k_plp_runs<16> was 1.1 % slower twice over: profiles/r07/README.md.)
#define MFX_PLP_RUNS 0
#include "mfx_plp_body.h"
#undef MFX_PLP_RUNS
#define MFX_PLP_RUNS 1
#include "mfx_plp_body.h"
#undef MFX_PLP_RUNS

template <int PMAX>
size_t plp_lds_bytes_t(const PlpParams &p, int n_waves)
{
    const size_t nb = (size_t)p.num_banks;
    const size_t f = mel64_lds_floats(p.num_banks, p.mel.rounds, p.mel.row_stride) + 8 +
                     (nb + 2) * plp_ps(PMAX) + ((nb + 3) & ~(size_t)3) + (((size_t)p.ceps_len + 3) & ~(size_t)3) +
                     (size_t)n_waves * ((size_t)p.mag_floats + (size_t)kPlpRows * plp_rp(p.num_banks, p.ceps_len));
    return f * sizeof(float);
}

// groups of kPlpRows rows for the busiest of `active` tables (launch_plp: all rows, 1); args: the kernel's arguments
template <int PMAX>
hipError_t launch_plp_t(const void *fn, const PlpParams &p, int64_t groups, int active, hipStream_t stream, void **args)
{
    const int tables = p.n_tables > 1 ? p.n_tables : 1;
    if (tables > kGridYMax) return hipErrorInvalidValue;
    ResidentGrid g;
    if (hipError_t e = resident_grid(fn, [&](int nw) { return plp_lds_bytes_t<PMAX>(p, nw); }, groups, active, g); e != hipSuccess) return e;
    return hipLaunchKernel(fn, dim3(g.blocks, (unsigned)tables), dim3(64 * g.waves), args, g.lds, stream);
}

static bool plp_args_ok(const PlpParams &p)
{
    return spec_rows_ok(p.mag_floats, p.spec_pitch) && p.lpc_order >= 1 && p.lpc_order <= kPlpMaxOrder && p.ceps_len >= 1 && p.num_banks >= 1;
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
    if (!plp_args_ok(p)) return hipErrorInvalidValue;
    const int64_t groups = (p.n_rows + kPlpRows - 1) / kPlpRows;
    PlpParams q = p;
    void *args[] = {&q};
    switch (plp_pmax(p.lpc_order)) {
    case 8: return launch_plp_t<8>((const void *)k_plp<8>, p, groups, 1, stream, args);
    case 16: return launch_plp_t<16>((const void *)k_plp<16>, p, groups, 1, stream, args);
    default: return launch_plp_t<32>((const void *)k_plp<32>, p, groups, 1, stream, args);
    }
}

hipError_t launch_plp_runs(const PlpParams &p, const RowRuns &rr, const int32_t *h_off, const int64_t *h_runs, hipStream_t stream)
{
    int active = 0;
    const int64_t groups = run_groups_in_window(h_off, h_runs, p.n_tables > 1 ? p.n_tables : 1, rr.row0, rr.rows, kPlpRows, active);
    if (groups <= 0) return hipSuccess;
    if (!plp_args_ok(p) || p.r_out) return hipErrorInvalidValue;
    PlpParams q = p;
    RowRuns r = rr;
    void *args[] = {&q, &r};
    switch (plp_pmax(p.lpc_order)) {
    case 8: return launch_plp_t<8>((const void *)k_plp_runs<8>, p, groups, active, stream, args);
    case 16: return launch_plp_t<16>((const void *)k_plp_runs<16>, p, groups, active, stream, args);
    default: return launch_plp_t<32>((const void *)k_plp_runs<32>, p, groups, active, stream, args);
    }
}

} // namespace mfx
