// mfx_sess_resample.hip -- k_sess_resample: sample-rate conversion in front of a push of the session entries (int16 -> int16),
// and its launcher.  See DESIGN.md section 5, "Session sample-rate conversion".
//
// Output sample j of a STREAM is k_resample's, unchanged (mfx_resample.hip; the chain is convert_tile of
// mfx_resample_dev.h): n = (j M) div L, phi = (j M) mod L, the ascending fmaf sum over x[n - Wh + 1 + k], rintf, clamp.  What
// differs is where x comes from.  A piece converts outputs [j_old, j_new) of its stream from stream samples [c0, n_new): the
// samples [c0, n_old) lie in the session's PREVIOUS carry slot, the samples [n_old, n_new) in the caller's array; samples
// before 0 are zero, samples at or after n_new are zero and are reached only by a final push (an open stream converts only the
// outputs whose last tap has arrived: the planner's delivery rule).
//
// Layout: grid = tiles, 256 threads; a tile is at most tile_out consecutive outputs of ONE piece, the first at j_old, so one
// launch serves any mix of rates.  A block
//   0. (the piece's first tile) writes the new carry, stream samples [c1, n_new), to the session's CURRENT carry slot as whole
//      32-bit words -- previous and current slot are different slots of the ping-pong pair, so no block of the launch reads
//      what another writes;
//   1. stages the rate's table in LDS when ResRate::in_lds says so, as k_resample does;
//   2. stages the tile's input span with halo in LDS as floats, eight samples per channel per work item: a group inside the
//      caller's part is read as whole 32-bit words at the array's own alignment (mono: the span starts one sample early where
//      the piece sits on an odd element), a group inside the carried part as whole words of the slot (four from its 16-byte
//      base's even elements, or the five that hold the group where the carry's parity differs from the array's: mono only), and
//      2-byte loads serve only the groups that hold the seam or an end;
//   3. runs convert_tile on it: the one FMA chain, so the bits are those of k_resample whatever the cut;
//   4. stores the int16 results as whole words into the scratch, where every piece starts on an even sample and is padded with
//      a zero to an even length.
// Pass-through pieces of a push that converts (rate = -1) copy their new samples to the scratch, word by word.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_launch.h"
#include "mfx_resample_dev.h"

#include <algorithm>

namespace mfx {

namespace {

// stream sample n of channel c, c0 <= n < n_new
template <int CH>
__device__ __forceinline__ int16_t stream_sample(const SessResampleParams &p, const SessResTile &t, int64_t n, int c)
{
    return n < t.n_old ? p.carry[t.carry_src + (n - t.c0) * CH + c] : p.pcm[(t.in_off + (n - t.n_old)) * CH + c];
}

// the carry a push leaves: stream samples [c1, n_new) -> the current slot, two elements per 32-bit word
template <int CH>
__device__ __forceinline__ void move_carry(const SessResampleParams &p, const SessResTile &t)
{
    const int elems = (int)(t.n_new - t.c1) * CH, words = (elems + 1) >> 1;
    uint32_t *dst = (uint32_t *)(p.carry + t.carry_dst);
    for (int i = threadIdx.x; i < words; i += 256) {
        const int e = 2 * i;
        uint32_t v = (uint16_t)stream_sample<CH>(p, t, t.c1 + e / CH, e % CH);
        if (e + 1 < elems) v |= (uint32_t)(uint16_t)stream_sample<CH>(p, t, t.c1 + (e + 1) / CH, (e + 1) % CH) << 16;
        dst[i] = v;
    }
}

// a pass-through piece: new samples [j0 - j_old, ...) of it, word by word (two words and a 2-byte shift when the source is on
// an odd element)
template <int CH>
__device__ __forceinline__ void copy_piece(const SessResampleParams &p, const SessResTile &t)
{
    const int64_t left = t.j_new - t.j0;
    const int n = (int)(left < kResCopyTile ? left : kResCopyTile);
    const int elems = n * CH, words = (elems + 1) >> 1;
    const int64_t es = (t.in_off + (t.j0 - t.j_old)) * CH;
    uint32_t *dst = (uint32_t *)(p.out + (t.out_off + (t.j0 - t.j_old)) * CH);
    const uint32_t *src = (const uint32_t *)p.pcm;
    for (int i = threadIdx.x; i < words; i += 256) {
        const int64_t e = es + 2 * (int64_t)i;
        const bool hi = 2 * i + 1 < elems;
        uint32_t v;
        if ((e & 1) == 0) {
            v = src[e >> 1];
            if (!hi) v &= 0xffffu;
        } else {
            v = src[(e - 1) >> 1] >> 16;
            if (hi) v |= src[(e + 1) >> 1] << 16;
        }
        dst[i] = v;
    }
}

template <int CH>
__device__ __forceinline__ void words_to_floats(const uint32_t *w, float (&v)[CH][8])
{
    if (CH == 1) {
        const uint32_t a = w[0], b = w[1], c = w[2], d = w[3];
        v[0][0] = lo16(a), v[0][1] = hi16(a), v[0][2] = lo16(b), v[0][3] = hi16(b);
        v[0][4] = lo16(c), v[0][5] = hi16(c), v[0][6] = lo16(d), v[0][7] = hi16(d);
    } else {
        uint32_t a[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) a[q] = w[q];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[0][q] = lo16(a[q]), v[CH - 1][q] = hi16(a[q]);
    }
}

// LDS: table [taps_floats] | input span [CH][x_floats] | output staging, int16 [out_elems]
template <int CH>
__global__ void __launch_bounds__(256) k_sess_resample(SessResampleParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const SessResTile t = p.tiles[blockIdx.x];
    if (t.move) move_carry<CH>(p, t);
    if (t.rate < 0) {
        copy_piece<CH>(p, t);
        return;
    }
    const ResRate r = p.rates[t.rate];
    const int64_t left = t.j_new - t.j0;
    const int nout = (int)(left < r.tile_out ? left : r.tile_out);
    if (nout <= 0) return; // (a piece that only moves its carry)
    const int tid = threadIdx.x;
    float *s_taps = smem;
    float *s_x = smem + p.taps_floats;
    const int xf = p.x_floats;
    int16_t *s_out = (int16_t *)(s_x + CH * xf);

    const int64_t n_first = (t.j0 * (int64_t)r.M) / r.L;
    const int64_t span0 = n_first - r.Wh + 1;
    // mono: position 0 of the span sits on an even element of the caller's array
    const int64_t base_n = CH == 1 ? span0 - ((t.in_off + span0 - t.n_old) & 1) : span0;
    const int64_t n_end = ((t.j0 + nout - 1) * (int64_t)r.M) / r.L + r.Wh; // last sample any chain of the tile reads
    const int groups = (int)((n_end - base_n + 8) >> 3);                  // of 8 samples per channel (host: 8 groups <= x_floats)

    if (r.in_lds) {
        const float *g = p.taps + r.taps_off;
        const int n = r.L * r.P, P = r.P;
        for (int i = tid; i < n; i += 256) {
            const int ph = (int)((uint32_t)i / (uint32_t)P);
            s_taps[i + ph] = g[i]; // ph * (P + 1) + (i - ph * P)
        }
    }
    {   // output staging cleared: the half word behind an odd count is stored as zero
        uint32_t *o = (uint32_t *)s_out;
        const int words = (min(r.tile_out, p.out_elems / CH) * CH + 1) >> 1;
        for (int i = tid; i < words; i += 256) o[i] = 0;
    }
    for (int g = tid; g < groups; g += 256) {
        const int64_t n0 = base_n + 8 * (int64_t)g;
        float v[CH][8];
        const int64_t ce = t.carry_src + (n0 - t.c0) * CH; // the group's first element, were it carried
        if (n0 >= t.n_old && n0 + 8 <= t.n_new) {
            words_to_floats<CH>((const uint32_t *)(p.pcm + (t.in_off + (n0 - t.n_old)) * CH), v); // an even element: a whole word
        } else if (n0 >= t.c0 && n0 + 8 <= t.n_old && (ce & 1) == 0) {
            words_to_floats<CH>((const uint32_t *)(p.carry + ce), v);
        } else if (CH == 1 && n0 >= t.c0 && n0 + 8 <= t.n_old) {
            // carried samples on an odd element (the carry's parity differs from the array's): the five words that hold them; the
            // last one ends one element behind the group, inside the slot (a slot is longer than any carry)
            const uint32_t *w = (const uint32_t *)(p.carry + (ce - 1));
            const uint32_t a = w[0], b = w[1], c = w[2], d = w[3], e = w[4];
            v[0][0] = hi16(a), v[0][1] = lo16(b), v[0][2] = hi16(b), v[0][3] = lo16(c);
            v[0][4] = hi16(c), v[0][5] = lo16(d), v[0][6] = hi16(d), v[0][7] = lo16(e);
        } else { // a group that holds the seam or an end of the stream
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int64_t n = n0 + q;
                const bool in = n >= t.c0 && n < t.n_new;
#pragma unroll
                for (int c = 0; c < CH; ++c) v[c][q] = in ? (float)stream_sample<CH>(p, t, n, c) : 0.f;
            }
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            rs_f4 *d = (rs_f4 *)(s_x + c * xf + 8 * g);
            d[0] = rs_f4{v[c][0], v[c][1], v[c][2], v[c][3]};
            d[1] = rs_f4{v[c][4], v[c][5], v[c][6], v[c][7]};
        }
    }
    __syncthreads();

    ResTile bt{};
    bt.j0 = t.j0;
    if (r.in_lds)
        convert_tile<CH, true>(r, bt, s_taps, r.P + 1, s_x, xf, s_out, nout, base_n);
    else
        convert_tile<CH, false>(r, bt, p.taps + r.taps_off, r.P, s_x, xf, s_out, nout, base_n);
    __syncthreads();

    const int words = (nout * CH + 1) >> 1;
    const int64_t eo = (t.out_off + (t.j0 - t.j_old)) * CH; // even
    const uint32_t *so = (const uint32_t *)s_out;
    uint32_t *dst = (uint32_t *)(p.out + eo);
    int done = 0;
    if (((eo & 7) | ((uintptr_t)p.out & 15)) == 0) {
        const int quads = words >> 2;
        for (int i = tid; i < quads; i += 256) ((uint4 *)dst)[i] = ((const uint4 *)so)[i];
        done = quads << 2;
    }
    for (int i = done + tid; i < words; i += 256) dst[i] = so[i];
}

} // namespace

hipError_t launch_sess_resample(const SessResampleParams &p, hipStream_t stream)
{
    if (p.n_tiles <= 0) return hipSuccess;
    if (!p.out || !p.carry || !p.tiles || !p.rates || !p.taps || (p.channels != 1 && p.channels != 2) || (p.x_floats & 7) ||
        (p.taps_floats & 3) || (p.out_elems & 1))
        return hipErrorInvalidValue;
    ResampleParams q{};
    q.channels = p.channels, q.taps_floats = p.taps_floats, q.x_floats = p.x_floats, q.out_elems = p.out_elems;
    const size_t lds = resample_lds_bytes(q);
    if (lds > kLdsMax) return hipErrorInvalidValue;
    const void *fn = p.channels == 2 ? (const void *)k_sess_resample<2> : (const void *)k_sess_resample<1>;
    if (hipError_t e = allow_dynamic_lds(fn, lds); e != hipSuccess) return e;
    SessResampleParams a = p;
    if (hipError_t e = launch_kernel(fn, dim3((unsigned)p.n_tiles), dim3(256), lds, stream, a); e != hipSuccess) return e;
    return hipGetLastError();
}

} // namespace mfx
