// mfx_slide.hip -- the sliding-window CMN / CVN of the batch entries (mfx_batch_set_sliding_norm): apply-cmvn-sliding of a
// Kaldi-style recipe.  The window sums are differences of the online normaliser's prefix chains, so the launch sequence is
//   k_onorm_totals, k_onorm_offsets   (mfx_onorm.hip, unchanged: the offsets O of v and q of every 32-row chunk)
//   k_slide_apply                     per chunk: lead chain up to we - 1, trail chain up to ws - 1, statistics, write
// over the online normaliser's utterance tiling.  include/mfx.h states every sum's order; mfx_onorm_dev.h holds the arithmetic
// (the links of the chains, slide_row) and the tile image, mfx_tables.h the window rule (slide_window), which the host
// restatement shares.  See DESIGN.md section 5, "Sliding-window normalisation".
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_dev.h"
#include "mfx_launch.h"
#include "mfx_onorm_dev.h"

namespace mfx {

namespace {

// One chain of a column thread over the 32 rows of its chunk.  The positions it must reach -- we - 1 (lead) or ws - 1 (trail)
// of row r -- never decrease from one row to the next and advance by at most one (slide_window), so the 32 of them lie in at
// most two consecutive chunks of the utterance, [base, base + 64).  I is rebuilt by the definition's ascending chain from the
// start of the first chunk: `pre` holds its rows up to the position of row 0, `adv` the row at the position of every later
// row (read whether or not the position moved, from an address that always exists, so that no load waits for a decision).
// Position -1 (ws == 0: P[-1] = 0) is the last row of a chunk "-1" whose O and I are 0; its successor is chunk 0.
struct SlideChain {
    int pos;       // the position of the current row
    uint32_t step; // bit r: the position of row r is that of row r - 1 plus one
    double Ov, Oq, Nv, Nq; // O of the current chunk; O of the next one
    double Iv, Iq;
};

// grid = ceil(n_chunks / G), 256 threads, dynamic LDS: the tiles' descriptors and the tiles' own rows [32][G * Wn], which
// become the output rows in place (the online kernel's image: mfx_onorm_dev.h).  The rows of the two chains go straight into
// the column thread's registers, as the online kernel's trail tile does: the lanes of a wave still read whole row pieces.
__global__ void __launch_bounds__(256) k_slide_apply(SlideParams sp)
{
#pragma clang fp contract(off)
    extern __shared__ int64_t s_dyn[]; // row0 [G] | rows [G] | local chunk [G] | T [G] | tiles
    const OnormParams &p = sp.pre;
    const int Wn = p.Wn, G = onorm_tiles(Wn), GW = G * Wn;
    const int tid = threadIdx.x;
    int64_t *s_row0 = s_dyn;
    int32_t *s_rows = (int32_t *)(s_row0 + G), *s_lc = s_rows + G, *s_T = s_lc + G;
    float *tile = (float *)(s_T + G);
    if (tid < G) {
        const int ci = blockIdx.x * G + tid;
        int64_t row0 = 0;
        int rows = 0, lc = 0, T = 0;
        if (ci < p.chunks.count) {
            const UttItem ch = utt_item<kOnormChunk>(p.chunks, p.segs, p.chunks.first + ci);
            row0 = ch.row0 + ch.t0, rows = ch.n, lc = ch.local, T = ch.T;
        }
        s_row0[tid] = row0, s_rows[tid] = rows, s_lc[tid] = lc, s_T[tid] = T;
    }
    __syncthreads();
    const int g = tid / Wn, j = tid - g * Wn;
    const bool mine = g < G && s_rows[g] > 0;
    const int N = sp.window, mw = sp.min_window;
    const bool center = sp.center != 0;

    SlideChain lead{}, trail{};
    float lpre[kOnormChunk], ladv[kOnormChunk], tpre[kOnormChunk], tadv[kOnormChunk];
    int lcnt = 0, tcnt = 0; // rows of `pre` that exist
    if (mine) {
        const int T = s_T[g], rows = s_rows[g], t0 = s_lc[g] * kOnormChunk;
        const float *usrc = p.src + (s_row0[g] - t0) * (int64_t)p.src_pitch + j; // row 0 of the utterance, this column
        const double *uo = p.tot + (int64_t)(p.chunks.first + blockIdx.x * G + g - s_lc[g]) * 2 * Wn + j; // O of its chunk 0
        int ws, we;
        slide_window(T, N, mw, center, t0, ws, we);
        lead.pos = we - 1, trail.pos = ws - 1;
        // (rows past the utterance's end take its last row's window: their positions stand still and nothing stores them)
        int lp = lead.pos, tp = trail.pos;
#pragma unroll
        for (int r = 1; r < kOnormChunk; ++r) {
            slide_window(T, N, mw, center, t0 + min(r, rows - 1), ws, we);
            lead.step |= (uint32_t)(we - 1 != lp) << r, trail.step |= (uint32_t)(ws - 1 != tp) << r;
            lp = we - 1, tp = ws - 1;
            ladv[r] = usrc[(int64_t)lp * p.src_pitch];
            tadv[r] = usrc[(int64_t)max(tp, 0) * p.src_pitch];
        }
        ladv[0] = tadv[0] = 0.f;
        const int lbase = lead.pos & ~(kOnormChunk - 1), tbase = trail.pos < 0 ? -kOnormChunk : trail.pos & ~(kOnormChunk - 1);
        lcnt = lead.pos - lbase + 1, tcnt = trail.pos < 0 ? 0 : trail.pos - tbase + 1;
#pragma unroll
        for (int k = 0; k < kOnormChunk; ++k) {
            lpre[k] = usrc[(int64_t)min(lbase + k, lead.pos) * p.src_pitch];
            tpre[k] = usrc[(int64_t)max(min(tbase + k, trail.pos), 0) * p.src_pitch];
        }
        // (a chunk behind the utterance's last has no O, and no row of this tile reaches it)
        const int per = 2 * Wn;
        const double *lo = uo + (int64_t)(lbase / kOnormChunk) * per, *tn = uo + (int64_t)(tbase / kOnormChunk + 1) * per;
        lead.Ov = lo[0], lead.Oq = lo[Wn];
        if (lbase + kOnormChunk < T) lead.Nv = lo[per], lead.Nq = lo[per + Wn];
        if (trail.pos >= 0) trail.Ov = tn[-per], trail.Oq = tn[Wn - per];
        if (tbase + kOnormChunk < T) trail.Nv = tn[0], trail.Nq = tn[Wn];
    }
    const OnormTileIndex ix(Wn, G);
    onorm_tiles_load(ix, p.src, p.src_pitch, s_row0, s_rows, tile, tid);
    __syncthreads();
    if (mine) {
        // the chains up to the positions of row 0
#pragma unroll
        for (int k = 0; k < kOnormChunk; ++k) {
            if (k < lcnt) lead.Iv = onorm_add(lead.Iv, (double)lpre[k]), lead.Iq = onorm_add(lead.Iq, onorm_sq(lpre[k]));
            if (k < tcnt) trail.Iv = onorm_add(trail.Iv, (double)tpre[k]), trail.Iq = onorm_add(trail.Iq, onorm_sq(tpre[k]));
        }
        // (all 32 rows whatever the tile holds: the staging left zeros behind its last row and nothing stores them)
#pragma unroll
        for (int r = 0; r < kOnormChunk; ++r) {
            if (r > 0 && ((lead.step >> r) & 1)) {
                if ((++lead.pos & (kOnormChunk - 1)) == 0) lead.Ov = lead.Nv, lead.Oq = lead.Nq, lead.Iv = 0.0, lead.Iq = 0.0;
                lead.Iv = onorm_add(lead.Iv, (double)ladv[r]), lead.Iq = onorm_add(lead.Iq, onorm_sq(ladv[r]));
            }
            if (r > 0 && ((trail.step >> r) & 1)) {
                if ((++trail.pos & (kOnormChunk - 1)) == 0) trail.Ov = trail.Nv, trail.Oq = trail.Nq, trail.Iv = 0.0, trail.Iq = 0.0;
                trail.Iv = onorm_add(trail.Iv, (double)tadv[r]), trail.Iq = onorm_add(trail.Iq, onorm_sq(tadv[r]));
            }
            const double Sw = onorm_sub(onorm_add(lead.Ov, lead.Iv), onorm_add(trail.Ov, trail.Iv));
            const double Qw = onorm_sub(onorm_add(lead.Oq, lead.Iq), onorm_add(trail.Oq, trail.Iq));
            tile[r * GW + tid] = slide_row(tile[r * GW + tid], Sw, Qw, lead.pos - trail.pos, sp.norm_vars);
        }
    }
    __syncthreads();
    onorm_tiles_store(ix, p.out, p.out_pitch, s_row0, s_rows, tile, tid);
}

} // namespace

hipError_t launch_slide(const SlideParams &sp, hipStream_t stream)
{
    const OnormParams &p = sp.pre;
    if (p.n_utt <= 0 || p.chunks.count <= 0) return hipSuccess;
    if (p.Wn < 1 || p.Wn > 256 || sp.window < 1 || sp.window > 4096 || sp.min_window < 0 || sp.min_window > sp.window || p.src == p.out ||
        p.src_pitch < p.Wn || p.out_pitch < p.Wn || p.chunks.rows != kOnormChunk) // (the chunk size is the kernels' constant)
        return hipErrorInvalidValue;
    if (hipError_t e = launch_onorm_prefix(p, stream); e != hipSuccess) return e;
    const int G = p.Wn >= 256 ? 1 : 256 / p.Wn;
    const int blocks = (p.chunks.count + G - 1) / G;
    const size_t lds = (size_t)G * 20 + (size_t)kOnormChunk * G * p.Wn * sizeof(float); // descriptors + tiles: <= 37 KB
    hipLaunchKernelGGL(k_slide_apply, dim3(blocks), dim3(256), lds, stream, sp);
    return hipGetLastError();
}

} // namespace mfx
