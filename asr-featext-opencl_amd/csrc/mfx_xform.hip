// mfx_xform.hip -- k_splice_affine: frame splicing + affine transform of finished feature rows, and its launcher.  See
// DESIGN.md, "Splice + affine transform".
//
// Per utterance of T frames (Wd = row width, C = left + right + 1, in_dim = C Wd, x = the utterance's transform):
//   z[t]      = [ y[clamp(t - left, 0, T - 1)] | ... | y[clamp(t + right, 0, T - 1)] ]
//   out[t][r] = b_x[r], then for i = 0 .. in_dim - 1 ascending: fmaf(A_x[r][i], z[t][i], .)       float32, one FMA per tap
//
// Layout: grid = (tiles, segments) as k_traps; a block takes R = 64, 32 or 16 consecutive output rows of one utterance.  The
// tile's rows plus the left + right clamped context rows are staged in LDS back to back at pitch Wd, so that z[t] is the
// contiguous run s_y[t Wd .. t Wd + in_dim): no splice is ever materialised.  The matrix does not fit LDS in general; it
// comes as operands [step of 4 taps][tile of 16 outputs][64 lanes] (build_xform_operands) and is streamed through two LDS
// buffers in chunks of `ksteps` steps, chunk c + 1 travelling through registers while chunk c is consumed.
// Waves: G = R / 16 row groups, wave w owns group w % G and the output tiles (w / G) + j (4 / G), j < TM, and carries all
// their accumulators through every tap -- the chain of an output is never cut.
//   matrix pipe (default): v_mfma_f32_16x16x4_f32 per 4 taps and tile, A[i][k] = s_y[(16 g + i) Wd + 4 s + k]; the A
//     operand of a step is read once and serves all the wave's tiles, whose products are independent and interleave (the
//     instruction's dependent latency, 40 cycles, is longer than its issue interval, 32).  A wave with a single tile
//     (out_dim <= 16 at R = 64) has one chain; the other waves of its SIMD fill the gaps.
//   vector ALUs (XformParams::valu): the same operands, every lane the accumulators the matrix form leaves in it (output
//     lane & 15 of each tile, rows 4 (lane >> 4) + r).
// Both are the same ascending FMA chain from b for every output, so they deliver the same bits.  Taps past in_dim (in_dim
// is padded to a multiple of 4) meet zero matrix columns and a z forced to zero, never another frame's values.
// Finished rows are assembled in LDS as they lie in memory and stored with consecutive lanes on consecutive words, as
// 16-byte words where the pitch, out_dim and the pointer allow.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_dev.h"
#include "mfx_launch.h"
#include "mfx_tile_dev.h"
#include "mfx_xform_dev.h"

namespace mfx {

namespace {

// (xform_tiles / xform_steps / xform_ksteps, the chunk loop and the scatter: mfx_xform_dev.h, shared with k_sess_xform)
// floats of the staged rows: R + left + right rows back to back, then the zeros the last row's padded taps read
__host__ __device__ inline int xform_stage_floats(int R, int width, int ctx) { return (R + ctx) * width + 4; }

// LDS: s_out [R][out_dim] | operand buffers [2][ksteps][tiles][64] | s_y [(R + left + right) Wd + 4]
template <bool VALU, int TM>
__global__ void __launch_bounds__(256) k_splice_affine(XformParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Segment sg = p.segs[blockIdx.y];
    const int R = p.tile_rows;
    const int r0 = blockIdx.x * R;
    if (r0 >= sg.n_out) return;
    const int rows = min(R, sg.n_out - r0);
    const int Wd = p.width, ctx = p.left + p.right, in_dim = (ctx + 1) * Wd, od = p.out_dim;
    const int NT = xform_tiles(od), steps = xform_steps(in_dim), KS = p.ksteps;
    const int chunk4 = KS * NT * 16;  // 16-byte words of a chunk
    const int total4 = steps * NT * 16;
    const int nchunks = (steps + KS - 1) / KS;
    const int x = p.seg_xf ? p.seg_xf[blockIdx.y] : 0;
    const f32x4 *ops4 = (const f32x4 *)(p.operands + (int64_t)x * steps * NT * 64);
    const float *bias = p.bias + (int64_t)x * NT * 16;
    const int tid = threadIdx.x;
    float *s_out = smem;
    float *s_b = smem + ((R * od + 3) & ~3);
    float *s_y = s_b + 2 * chunk4 * 4;

    // chunk 0 on its way while the rows are staged
    f32x4 pf[2] = {};
    xform_prefetch0(ops4, pf, chunk4, total4, tid);
    {   // rows r0 - left .. r0 + R + right - 1 of the utterance, clamped to it; zeros behind them
        const int n = (R + ctx) * Wd;
        const uint32_t magic = div_magic(Wd); // floor(i / Wd) for i < 2^16 (n < 160 KB / 4)
        for (int i = tid; i < n; i += 256) {
            const int rr = div_small(i, Wd, magic);
            const int c = i - rr * Wd;
            const int sr = max(sg.lo, min(sg.hi, r0 + rr - p.left));
            s_y[i] = p.src[(sg.src_row0 + sr) * (int64_t)p.src_pitch + c];
        }
        if (tid < 4) s_y[n + tid] = 0.f;
    }
    xform_commit0(s_b, pf, chunk4, total4, tid);
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const XformWave w = xform_wave<TM>(wave, R >> 4, NT); // row group w.g, output tiles w.slot + j w.slots, j < w.cnt
    const int g = w.g;
    const bool busy = w.cnt > 0 && 16 * g < rows;

    // matrix form: lane (li, lk) feeds row 16 g + li, tap 4 s + lk; vector form: rows 16 g + 4 lk + r, taps in turn
    const float *za = VALU ? s_y + (16 * g + 4 * lk) * Wd : s_y + (16 * g + li) * Wd + lk;
    xform_compute<VALU, TM>(ops4, bias, pf, s_b, chunk4, total4, nchunks, steps, KS, NT, in_dim, Wd, za, busy, w, tid, s_out + 16 * g * od, od,
                            rows - 16 * g);

    tile_store_rows(s_out, od, rows, p.out, sg.out_row0 + r0, p.out_pitch, tid);
}

template <bool VALU>
const void *xform_fn(int tm)
{
    switch (tm) {
    case 1: return (const void *)k_splice_affine<VALU, 1>;
    case 2: return (const void *)k_splice_affine<VALU, 2>;
    case 3: return (const void *)k_splice_affine<VALU, 3>;
    case 4: return (const void *)k_splice_affine<VALU, 4>;
    case 8: return (const void *)k_splice_affine<VALU, 8>;
    default: return (const void *)k_splice_affine<VALU, 16>;
    }
}

} // namespace

bool xform_shape_ok(const XformParams &p)
{
    return p.width >= 1 && p.left >= 0 && p.left <= 32 && p.right >= 0 && p.right <= 32 && p.out_dim >= 1 && p.out_dim <= 256 &&
           (int64_t)(p.left + p.right + 1) * p.width <= 8192;
}

size_t xform_lds_bytes(const XformParams &p, int tile_rows)
{
    const int in_dim = (p.left + p.right + 1) * p.width;
    const size_t f = (size_t)((tile_rows * p.out_dim + 3) & ~3) +
                     (size_t)2 * xform_ksteps(in_dim, p.out_dim) * xform_tiles(p.out_dim) * 64 +
                     (size_t)xform_stage_floats(tile_rows, p.width, p.left + p.right);
    return f * sizeof(float);
}

#ifndef MFX_XFORM_LDS_TARGET
#define MFX_XFORM_LDS_TARGET kTileLdsTarget
#endif
int xform_tile_rows(const XformParams &p)
{
    return xform_shape_ok(p) ? tile_rows_for([&](int r) { return xform_lds_bytes(p, r); }, MFX_XFORM_LDS_TARGET) : 0;
}

hipError_t launch_xform(const XformParams &p, hipStream_t stream)
{
    if (p.n_segs <= 0 || p.tiles_per_seg_max <= 0) return hipSuccess;
    if (!xform_shape_ok(p) || p.src_pitch < p.width || p.out_pitch < p.out_dim || !p.operands || !p.bias) return hipErrorInvalidValue;
    const int R = xform_tile_rows(p);
    if (R == 0) return hipErrorInvalidValue;
    const size_t lds = xform_lds_bytes(p, R);
    const int tm = xform_tm(p.out_dim, R);
    const void *fn = p.valu ? xform_fn<true>(tm) : xform_fn<false>(tm);
    if (hipError_t e = allow_dynamic_lds(fn, lds); e != hipSuccess) return e;
    const int tiles_x = p.tiles_per_seg_max * (64 / R);
    return for_seg_slices(p.n_segs, [&](int s0, int n) {
        XformParams q = p;
        q.tile_rows = R;
        q.ksteps = xform_ksteps((p.left + p.right + 1) * p.width, p.out_dim);
        q.segs = p.segs + s0;
        if (p.seg_xf) q.seg_xf = p.seg_xf + s0;
        q.n_segs = n;
        return launch_kernel(fn, dim3(tiles_x, n), dim3(256), lds, stream, q);
    });
}

} // namespace mfx
