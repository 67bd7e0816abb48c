// mfx_sess_xform.hip -- k_sess_xform: splice + affine transform of the rows one push delivers, for many sessions at once, and
// its launcher.  See DESIGN.md, "Session transform".
//
// The arithmetic is k_splice_affine's (mfx_xform.hip; the chunk loop, the chains and the scatter are the same code,
// mfx_xform_dev.h): out[t][r] = b_x[r], then fmaf(A_x[r][i], z[t][i], .) for i ascending, z[t] the rows t - left .. t + right of
// the session's stream, clamped to the window the push may read.  What differs is the tiling.  A push is many sessions with
// about ten rows each, so a block does not take 64 consecutive rows of one series: it takes up to G = 4, 2 or 1 ROW GROUPS
// (SessXfGroup: at most 16 output rows of one session, with their own source row, clamp window and output row), all of ONE
// transform (SessXfBlock), stages each group's 16 + left + right clamped rows in LDS at pitch Wd, and streams the operand chunks
// of that transform through the two LDS buffers exactly once while all its waves consume them.  Wave w owns group w % G and the
// output tiles (w / G) + j (4 / G), j < TM, as in k_splice_affine at R = 16 G rows.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_dev.h"
#include "mfx_launch.h"
#include "mfx_tile_dev.h"
#include "mfx_xform_dev.h"

namespace mfx {

namespace {

// floats of one group's staged rows: 16 + left + right rows back to back, then the zeros the last row's padded taps read
__host__ __device__ inline int sess_xform_stage_floats(int width, int ctx) { return (16 + ctx) * width + 4; }

// LDS: s_out [16 G][out_dim] | operand buffers [2][ksteps][tiles][64] | s_y [G][(16 + left + right) Wd + 4]
template <bool VALU, int TM>
__global__ void __launch_bounds__(256) k_sess_xform(SessXformParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const SessXfBlock blk = p.blocks[blockIdx.x];
    const int R = p.tile_rows, G = R >> 4;
    const int ng = min(blk.ng, G);
    const int Wd = p.width, ctx = p.left + p.right, in_dim = (ctx + 1) * Wd, od = p.out_dim;
    const int NT = xform_tiles(od), steps = xform_steps(in_dim), KS = p.ksteps;
    const int chunk4 = KS * NT * 16; // 16-byte words of a chunk
    const int total4 = steps * NT * 16;
    const int nchunks = (steps + KS - 1) / KS;
    const f32x4 *ops4 = (const f32x4 *)(p.operands + (int64_t)blk.xf * steps * NT * 64);
    const float *bias = p.bias + (int64_t)blk.xf * NT * 16;
    const int tid = threadIdx.x;
    const int stage = sess_xform_stage_floats(Wd, ctx);
    float *s_out = smem;
    float *s_b = smem + ((R * od + 3) & ~3);
    float *s_y = s_b + 2 * chunk4 * 4;

    // chunk 0 on its way while the groups' rows are staged
    f32x4 pf[2] = {};
    xform_prefetch0(ops4, pf, chunk4, total4, tid);
    {
        const int n = (16 + ctx) * Wd;
        const uint32_t magic = div_magic(Wd); // floor(i / Wd) for i < 2^16 (n < 160 KB / 4)
        for (int q = 0; q < ng; ++q) { // rows r0 - left .. r0 + 15 + right of the group's series, clamped to its window
            const SessXfGroup gr = p.groups[blk.g0 + q];
            float *sy = s_y + q * stage;
            for (int i = tid; i < n; i += 256) {
                const int rr = div_small(i, Wd, magic);
                const int c = i - rr * Wd;
                const int sr = max(gr.lo, min(gr.hi, gr.r0 + rr - p.left));
                sy[i] = p.src[(gr.src_row0 + sr) * (int64_t)p.src_pitch + c];
            }
            if (tid < 4) sy[n + tid] = 0.f;
        }
    }
    xform_commit0(s_b, pf, chunk4, total4, tid);
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const XformWave w = xform_wave<TM>(wave, G, NT);
    const bool busy = w.cnt > 0 && w.g < ng;

    const float *sy = s_y + w.g * stage;
    const float *za = VALU ? sy + 4 * lk * Wd : sy + li * Wd + lk;
    xform_compute<VALU, TM>(ops4, bias, pf, s_b, chunk4, total4, nchunks, steps, KS, NT, in_dim, Wd, za, busy, w, tid, s_out + 16 * w.g * od, od,
                            busy ? p.groups[blk.g0 + w.g].rows : 0);

    for (int q = 0; q < ng; ++q) {
        const SessXfGroup gr = p.groups[blk.g0 + q];
        tile_store_rows(s_out + 16 * q * od, od, min(gr.rows, 16), p.out, gr.out_row0, p.out_pitch, tid);
    }
}

template <bool VALU>
const void *sess_xform_fn(int tm)
{
    switch (tm) {
    case 1: return (const void *)k_sess_xform<VALU, 1>;
    case 2: return (const void *)k_sess_xform<VALU, 2>;
    case 3: return (const void *)k_sess_xform<VALU, 3>;
    case 4: return (const void *)k_sess_xform<VALU, 4>;
    case 8: return (const void *)k_sess_xform<VALU, 8>;
    default: return (const void *)k_sess_xform<VALU, 16>;
    }
}

bool sess_xform_shape_ok(const SessXformParams &p)
{
    return p.width >= 1 && p.left >= 0 && p.left <= 32 && p.right >= 0 && p.right <= 32 && p.out_dim >= 1 && p.out_dim <= 256 &&
           (int64_t)(p.left + p.right + 1) * p.width <= 8192;
}

} // namespace

size_t sess_xform_lds_bytes(const SessXformParams &p, int tile_rows)
{
    const int in_dim = (p.left + p.right + 1) * p.width;
    const size_t f = (size_t)((tile_rows * p.out_dim + 3) & ~3) +
                     (size_t)2 * xform_ksteps(in_dim, p.out_dim) * xform_tiles(p.out_dim) * 64 +
                     (size_t)(tile_rows >> 4) * sess_xform_stage_floats(p.width, p.left + p.right);
    return f * sizeof(float);
}

int sess_xform_tile_rows(const SessXformParams &p)
{
    return sess_xform_shape_ok(p) ? tile_rows_for([&](int r) { return sess_xform_lds_bytes(p, r); }, kTileLdsTarget) : 0;
}

hipError_t launch_sess_xform(const SessXformParams &p, hipStream_t stream)
{
    if (p.n_blocks <= 0) return hipSuccess;
    if (!sess_xform_shape_ok(p) || p.src_pitch < p.width || p.out_pitch < p.out_dim || !p.operands || !p.bias || !p.groups || !p.blocks)
        return hipErrorInvalidValue;
    const int R = sess_xform_tile_rows(p);
    if (R == 0 || (p.tile_rows != 0 && p.tile_rows != R)) return hipErrorInvalidValue; // (the work list was packed for another G)
    const size_t lds = sess_xform_lds_bytes(p, R);
    const int tm = xform_tm(p.out_dim, R);
    const void *fn = p.valu ? sess_xform_fn<true>(tm) : sess_xform_fn<false>(tm);
    if (hipError_t e = allow_dynamic_lds(fn, lds); e != hipSuccess) return e;
    SessXformParams q = p;
    q.tile_rows = R;
    q.ksteps = xform_ksteps((p.left + p.right + 1) * p.width, p.out_dim);
    return launch_kernel(fn, dim3(p.n_blocks), dim3(256), lds, stream, q);
}

} // namespace mfx
