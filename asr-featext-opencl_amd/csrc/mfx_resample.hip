// mfx_resample.hip -- k_resample: per-utterance sample-rate conversion of the batch entries' PCM (int16 -> int16), and its
// launcher.  See DESIGN.md, "Sample-rate conversion".
//
// Output sample j of an utterance converted by L / M with the table h [L][P], P = 2 Wh:
//   n = (j M) div L, phi = (j M) mod L                                           (int64)
//   acc = 0; for k = 0 .. P - 1 ascending: acc = fmaf(h[phi][k], (float)x[n - Wh + 1 + k], acc)     x outside the utterance = 0
//   y[j] = clamp(rintf(acc), -32768, 32767)
//
// Layout: grid = tiles, 256 threads; a tile is at most tile_out consecutive output samples of ONE utterance (ResTile), so one
// launch serves any mix of rates.  A block
//   1. stages the rate's table in LDS at row stride P + 1 (odd: the lanes' phases fall on different banks) when it fits
//      (ResRate::in_lds), else leaves it to the caches;
//   2. reads the tile's input span with halo from HBM ONCE -- eight samples per channel per work item, as whole 32-bit words
//      at the source's own alignment (an utterance on an odd sample starts its span one sample early, so that every word is
//      aligned; the extra sample is outside the utterance and staged as zero), 2-byte loads only in the groups that hold an
//      end of the utterance -- converts it to float and writes it to LDS as 16-byte words, one plane per channel; samples
//      outside [0, n_in) of the utterance are ZERO, never a neighbour's;
//   3. deals the outputs to work items: item w owns outputs w + r items, r < R, of the tile.  items is a multiple of L, so
//      the R outputs share the phase: a tap is read once and serves R (x 2 with stereo) FMAs, (R C + 1) / (R C) LDS reads per
//      FMA.  Consecutive lanes own consecutive outputs, so their x addresses advance by M / L on average: the same word or
//      the next when interpolating, stride M when decimating by an integer (free of bank conflicts for odd M, two-way for
//      2:1).  L = 1 has the one phase: every lane reads the same tap (a broadcast).  Every output's chain is the whole
//      ascending sum in one thread: nothing is cut or reordered, so the bits do not depend on the tiling;
//   4. assembles the int16 results in LDS and stores them as whole 32-bit words (16-byte words where the destination
//      allows); the half word behind an odd utterance length is written as zero (the scratch pads every utterance to an even
//      length).
// Tiles of utterances already at the output rate (rate = -1) copy their samples, word by word.
// The chain itself (convert_tile) is in mfx_resample_dev.h, shared with k_sess_resample.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_launch.h"
#include "mfx_resample_dev.h"

#include <algorithm>

namespace mfx {

namespace {

// a same-rate utterance: samples [j0, j0 + n) of it, word by word (two words and a 2-byte shift when the source is on an
// odd element)
template <int CH>
__device__ __forceinline__ void copy_tile(const ResampleParams &p, const ResTile &t)
{
    const int64_t left = t.n_out - t.j0;
    const int n = (int)(left < kResCopyTile ? left : kResCopyTile);
    const int elems = n * CH, words = (elems + 1) >> 1;
    const int64_t es = (t.in_off + t.j0) * CH;
    uint32_t *dst = (uint32_t *)(p.out + (t.out_off + t.j0) * CH);
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

// LDS: table [taps_floats] | input span [CH][x_floats] | output staging, int16 [out_elems]
template <int CH>
__global__ void __launch_bounds__(256) k_resample(ResampleParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const ResTile t = p.tiles[blockIdx.x];
    if (t.rate < 0) {
        copy_tile<CH>(p, t);
        return;
    }
    const ResRate r = p.rates[t.rate];
    const int tid = threadIdx.x;
    float *s_taps = smem;
    float *s_x = smem + p.taps_floats;
    const int xf = p.x_floats;
    int16_t *s_out = (int16_t *)(s_x + CH * xf);

    const int64_t left = t.n_out - t.j0;
    const int nout = (int)(left < r.tile_out ? left : r.tile_out);
    const int64_t n_first = (t.j0 * (int64_t)r.M) / r.L;
    const int64_t span0 = n_first - r.Wh + 1;
    // mono: position 0 of the span sits on an even element of the caller's array
    const int64_t base_n = CH == 1 ? span0 - ((t.in_off + span0) & 1) : span0;
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
        if (n0 >= 0 && n0 + 8 <= t.n_in) {
            const uint32_t *w = (const uint32_t *)(p.pcm + (t.in_off + n0) * CH); // an even element: a whole word
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
        } else { // a group that holds an end of the utterance: what lies outside is zero
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int64_t n = n0 + q;
                const bool in = n >= 0 && n < t.n_in;
#pragma unroll
                for (int c = 0; c < CH; ++c) v[c][q] = in ? (float)p.pcm[(t.in_off + n) * CH + c] : 0.f;
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

    if (r.in_lds)
        convert_tile<CH, true>(r, t, s_taps, r.P + 1, s_x, xf, s_out, nout, base_n);
    else
        convert_tile<CH, false>(r, t, p.taps + r.taps_off, r.P, s_x, xf, s_out, nout, base_n);
    __syncthreads();

    const int words = (nout * CH + 1) >> 1;
    const int64_t eo = (t.out_off + t.j0) * CH; // even
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

// outputs whose input span fits `budget` floats per channel
int64_t fit_outputs(const ResRate &r, int64_t budget)
{
    const int64_t s = budget - r.P - 32;
    return s <= 0 ? 0 : s * r.L / r.M;
}

} // namespace

// Tile geometry.  Target: 2048 outputs per tile with the input span inside 32 KB of LDS (all channels); a ratio or a filter
// too long for that takes up to 64 KB, and fewer outputs (the limits of mfx_batch_plan_rates leave at least 4).  R same-phase
// outputs per work item: 4 where four periods of L fit the tile, else 2, else 1 (every phase then occurs at most once in a tile:
// nothing to share).  The table goes to LDS when its padded form is at most 64 KB.
void resample_geometry(int channels, ResRate &r)
{
    const int ch = channels == 2 ? 2 : 1;
    int64_t to = std::min<int64_t>(2048, fit_outputs(r, 8192 / ch));
    if (to < 64) to = std::min<int64_t>(2048, fit_outputs(r, 16384 / ch));
    to = std::max<int64_t>(to & ~(int64_t)1, 2);
    if (2 * (int64_t)r.L > to) {
        r.R = 1;
        r.items = (int32_t)to;
    } else {
        r.R = 4 * (int64_t)r.L <= to ? 4 : 2;
        r.items = r.L * (int32_t)(to / ((int64_t)r.R * r.L));
    }
    r.tile_out = r.R * r.items;
    r.in_lds = (int64_t)r.L * (r.P + 1) <= 16384 ? 1 : 0;
}

// floats per channel of a full tile's span: (tile_out - 1) M / L + 1 input positions + P - 1 of halo + 1 for the parity
// step of a mono source, rounded up to whole groups of 8
int resample_span_floats(const ResRate &r)
{
    const int64_t span = ((int64_t)(r.tile_out - 1) * r.M) / r.L + r.P + 3;
    return (int)(((span + 7) & ~(int64_t)7) + 8);
}

size_t resample_lds_bytes(const ResampleParams &p)
{
    return ((size_t)p.taps_floats + (size_t)(p.channels == 2 ? 2 : 1) * p.x_floats) * sizeof(float) + (size_t)p.out_elems * sizeof(int16_t);
}

hipError_t launch_resample(const ResampleParams &p, hipStream_t stream)
{
    if (p.n_tiles <= 0) return hipSuccess;
    if (!p.pcm || !p.out || !p.tiles || (p.channels != 1 && p.channels != 2) || (p.x_floats & 7) || (p.taps_floats & 3) ||
        (p.out_elems & 1))
        return hipErrorInvalidValue;
    const size_t lds = resample_lds_bytes(p);
    if (lds > kLdsMax) return hipErrorInvalidValue;
    const void *fn = p.channels == 2 ? (const void *)k_resample<2> : (const void *)k_resample<1>;
    if (hipError_t e = allow_dynamic_lds(fn, lds); e != hipSuccess) return e;
    ResampleParams q = p;
    void *args[] = {&q};
    if (hipError_t e = hipLaunchKernel(fn, dim3((unsigned)p.n_tiles), dim3(256), args, lds, stream); e != hipSuccess) return e;
    return hipGetLastError();
}

} // namespace mfx
