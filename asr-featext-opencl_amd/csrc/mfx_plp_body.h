// mfx_plp_body.h -- the text of k_plp, included twice by mfx_plp.hip: MFX_PLP_RUNS 0 is k_plp itself, 1 is its row-run form
// k_plp_runs -- as k_melcep_runs (mfx_tail.hip) with groups of 64 rows: a wave's 64 rows come from ONE run, phase 2 runs with
// the table's own eql.  Not a header in its own right.
template <int PMAX>
#if MFX_PLP_RUNS
__global__ void __launch_bounds__(256) k_plp_runs(PlpParams p, RowRuns runs)
#else
__global__ void __launch_bounds__(256) k_plp(PlpParams p)
#endif
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n_waves = blockDim.x >> 6;
    const int nb = p.num_banks, RS = p.mel.row_stride, rounds = p.mel.rounds, MF = p.mag_floats;
    const int N = nb + 2, order = p.lpc_order, C = p.ceps_len;
    constexpr int PS = plp_ps(PMAX);
    const int RP = plp_rp(nb, C);
    const int WR = mel64_rows(nb);

    const int table = blockIdx.y;
#if MFX_PLP_RUNS
    int run0, run1; // the table's runs that reach into the window (none: nothing to stage; uniform over the block)
    if (!runs_in_window(runs, table, run0, run1)) return;
#endif
    MelPlanLds plan;
    float *s_idft = stage_mel_plan(smem, p.mel, nb, table, tid, blockDim.x, plan); // [N][PS]
    float *s_eql = s_idft + N * PS;                  // [nb, x4]
    float *s_lift = s_eql + ((nb + 3) & ~3);         // [C, x4]
    float *s_wave = s_lift + ((C + 3) & ~3) + wave * (MF + kPlpRows * RP);
    float *mag = s_wave, *rows = s_wave + MF;
    const float *geql = p.eql + (int64_t)table * nb;
#if MFX_PLP_RUNS
    float *feat = p.feat; // one output, absolute rows
    float *r_out = nullptr;
#else
    float *feat = p.feat + (int64_t)table * p.feat_table_stride;
    float *r_out = table == 0 ? p.r_out : nullptr;
#endif
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
#if MFX_PLP_RUNS
    for (RunGroups<kPlpRows> it(runs, run0, run1, (int64_t)blockIdx.x * n_waves + wave, (int64_t)gridDim.x * n_waves); it.valid();
         it.advance()) {
        const int64_t row0 = it.row0;
        const int count = it.count;
#else
    for (int64_t grp = (int64_t)blockIdx.x * n_waves + wave; grp * kPlpRows < p.n_rows; grp += (int64_t)gridDim.x * n_waves) {
        const int64_t row0 = grp * kPlpRows;
        const int count = (int)(p.n_rows - row0 < kPlpRows ? p.n_rows - row0 : kPlpRows);
#endif
        // ---- phase 1: filterbank energies of the power spectrum, one row at a time on the whole wave
        for (int f = 0; f < count; ++f) {
            const float4 *src = (const float4 *)(p.spec + (row0 + f) * p.spec_pitch);
            for (int k = lane; k < q4; k += 64) {
                const float4 v = src[k];
                ((float4 *)mag)[k] = make_float4(v.x * v.x, v.y * v.y, v.z * v.z, v.w * v.w);
            }
            if (nbins + lane < 4 * q4) mag[nbins + lane] = 0.f; // padding words are never written in memory
            wave_sync();
            mel64_walk_log<false>(mag, rows + f * RP + 1, -1, plan.s_mw, plan.s_mst, plan.s_mfid, plan.s_L, rounds, RS, lane, WR);
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
