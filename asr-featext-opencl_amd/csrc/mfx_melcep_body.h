// mfx_melcep_body.h -- the text of k_melcep, included twice by mfx_tail.hip: MFX_MELCEP_RUNS 0 is k_melcep itself (the
// same tokens as ever: the same ISA), 1 is its row-run form k_melcep_runs.  Not a header in its own right.
//
// k_melcep_runs (per-utterance warp factors of the batch entries): blockIdx.y is still the table, staged in LDS exactly as
// in k_melcep, but instead of all rows [0, n_rows) the block walks that table's row runs (RowRuns), each clipped to the
// slab's window.  The groups of 4 rows of the table's clipped runs are numbered through in run order and dealt to the
// waves of the grid's blockIdx.y plane (RunGroups, mfx_dev.h): a group starts at a clipped run's first row + 4 k and never
// spans two runs, only a run's last group is short.  spec and feat address absolute rows; each row's arithmetic is the
// code below, shared with k_melcep.
#if MFX_MELCEP_RUNS
__global__ void __launch_bounds__(256) k_melcep_runs(MelcepParams p, RowRuns rr)
#else
__global__ void __launch_bounds__(256) k_melcep(MelcepParams p)
#endif
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n_waves = blockDim.x >> 6;
    const int nb = p.num_banks, RS = p.mel64_row_stride, rounds = p.mel64_rounds;
    const int FS = lm_fs4(nb), MF = p.mag_floats;
    const int WR = mel64_rows(nb);                   // weight rows in LDS (lanes that carry a filter)
    float *s_mw = smem;                              // [WR][RS]
    int *s_mst = (int *)(s_mw + WR * RS);            // [rounds][64]
    int *s_mfid = s_mst + 64 * rounds;               // [rounds][64]
    int *s_L = s_mfid + 64 * rounds;                 // [8]
    float *s_wave = (float *)(s_L + 8) + wave * (MF + 4 * FS);
    float *mag = s_wave, *lm = s_wave + MF;

    const int table = blockIdx.y;
#if MFX_MELCEP_RUNS
    int run0, run1; // the table's runs that reach into the window (none: nothing to stage; uniform over the block)
    if (!runs_in_window(rr, table, run0, run1)) return;
#endif
    const float *gw = p.mel64_w + (int64_t)table * 64 * RS;
    const int32_t *gst = p.mel64_start + (int64_t)table * 64 * rounds, *gfid = p.mel64_fid + (int64_t)table * 64 * rounds;
#if MFX_MELCEP_RUNS
    float *feat = p.feat; // one output, absolute rows
#else
    float *feat = p.feat + (int64_t)table * p.feat_table_stride;
#endif
    for (int i = tid; i < WR * RS; i += blockDim.x) s_mw[i] = gw[i];
    for (int i = tid; i < 64 * rounds; i += blockDim.x) {
        s_mst[i] = gst[i];
        s_mfid[i] = gfid[i];
    }
    if (tid < 8) s_L[tid] = p.mel64_L[table * 8 + tid];
    for (int i = lane; i < MF + 4 * FS; i += 64) s_wave[i] = 0.f; // words past the last bin stay zero (finite) for good
    __syncthreads();

    const int dct_ks = p.dct_ksteps, dct_tiles64 = (p.dct_len + 63) >> 6;
    const int dct_bytes = p.dct_b4 ? dct_tiles64 * dct_ks * 1024 : 0;
    const __amdgpu_buffer_rsrc_t dct_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)p.dct_b4, 0, dct_bytes, 0x00020000);
    const int q4 = p.spec_pitch >> 2; // rows are whole 16-byte words (spec_pitch is a multiple of 4, rows 16-byte aligned)
    const int nbins = (p.fft_size >> 1) + 1;
#if MFX_MELCEP_RUNS
    for (RunGroups<4> it(rr, run0, run1, (int64_t)blockIdx.x * n_waves + wave, (int64_t)gridDim.x * n_waves); it.valid(); it.advance()) {
        const int64_t row0 = it.row0;
        const int count = it.count;
#else
    for (int64_t grp = (int64_t)blockIdx.x * n_waves + wave; grp * 4 < p.n_rows; grp += (int64_t)gridDim.x * n_waves) {
        const int64_t row0 = grp * 4;
        const int count = (int)(p.n_rows - row0 < 4 ? p.n_rows - row0 : 4);
#endif
        for (int f = 0; f < count; ++f) {
            const float4 *src = (const float4 *)(p.spec + (row0 + f) * p.spec_pitch);
            for (int k = lane; k < q4; k += 64) ((float4 *)mag)[k] = src[k];
            // the row's padding words (bins > W2/2) are never written in memory: they meet zero weights in the walk and
            // must be finite (0 x NaN is NaN)
            if (nbins + lane < 4 * q4) mag[nbins + lane] = 0.f;
            wave_sync();
            mel64_walk_log(mag, lm + f * FS, FS - 1, s_mw, s_mst, s_mfid, s_L, rounds, RS, lane, WR);
            wave_sync();
        }
        dct4_store<3>(lm, FS, dct_rsrc, dct_bytes, dct_ks, dct_tiles64, p.dct_b4 != nullptr, lane, p.cols, feat, (int64_t)p.feat_pitch,
                   row0, count);
        wave_sync();
    }
}
