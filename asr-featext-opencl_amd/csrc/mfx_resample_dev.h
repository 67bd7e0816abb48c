// mfx_resample_dev.h -- the tile body of the two sample-rate converters (int16 -> int16): k_resample (mfx_resample.hip: tiles of
// whole utterances of a batch) and k_sess_resample (mfx_sess_resample.hip: tiles of the pieces of a push, their input the
// session's carried tail and the caller's array).  See DESIGN.md, "Sample-rate conversion" and "Session sample-rate conversion".
//
// Output sample j of an utterance (a stream) converted by L / M with the table h [L][P], P = 2 Wh:
//   n = (j M) div L, phi = (j M) mod L                                           (int64)
//   acc = 0; for k = 0 .. P - 1 ascending: acc = fmaf(h[phi][k], (float)x[n - Wh + 1 + k], acc)     x outside the samples = 0
//   y[j] = clamp(rintf(acc), -32768, 32767)
//
// Layout: grid = tiles, 256 threads; a tile is at most tile_out consecutive output samples of ONE utterance (piece), so one
// launch serves any mix of rates.  LDS: table [taps_floats] | input span [CH][x_floats] | output staging, int16 [out_elems]
// (ResLds: the maxima over the launch's rates).  resample_tile, the body of both kernels,
//   1. stages the rate's table in LDS at row stride P + 1 (odd: the lanes' phases fall on different banks) when it fits
//      (ResRate::in_lds), else leaves it to the caches;
//   2. stages the tile's input span with halo in LDS as floats, one plane per channel, position base_n of the utterance (stream)
//      at index 0: eight samples per channel per work item, written as 16-byte words.  WHERE a group's eight samples come from
//      is the kernel's own business (its `load_group`); both read whole 32-bit words at the source's own alignment -- a mono
//      source on an odd element starts its span one sample early (ResSpan's parity term), so that every word is aligned -- and
//      2-byte loads only in the groups that hold an end or a seam; samples outside the source are ZERO, never a neighbour's;
//   3. deals the outputs to work items: item w owns outputs w + r items, r < R, of the tile.  items is a multiple of L, so
//      the R outputs share the phase: a tap is read once and serves R (x 2 with stereo) FMAs, (R C + 1) / (R C) LDS reads per
//      FMA.  Consecutive lanes own consecutive outputs, so their x addresses advance by M / L on average: the same word or
//      the next when interpolating, stride M when decimating by an integer (free of bank conflicts for odd M, two-way for
//      2:1).  L = 1 has the one phase: every lane reads the same tap (a broadcast).  Every output's chain is the whole
//      ascending sum in one thread: nothing is cut or reordered, so the bits do not depend on the tiling, the cut or the kernel;
//   4. assembles the int16 results in LDS and stores them as whole 32-bit words (16-byte words where the destination
//      allows); the half word behind an odd count is written as zero (the scratch pads every utterance and piece to an even
//      length).
// Tiles at the output rate (rate = -1) copy their samples, word by word (copy_words).
#pragma once
#include <hip/hip_runtime.h>

#include "mfx_kernels.h"
#include "mfx_launch.h"

#include <type_traits>

namespace mfx {
namespace {

typedef float rs_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float lo16(uint32_t w) { return (float)(int16_t)(w & 0xffffu); }
__device__ __forceinline__ float hi16(uint32_t w) { return (float)((int32_t)w >> 16); }

__device__ __forceinline__ int16_t to_pcm(float acc)
{
    return (int16_t)(int)fminf(fmaxf(rintf(acc), -32768.f), 32767.f);
}

// the outputs of a tile dealt to work items, every output's whole ascending FMA chain in one thread
template <int CH, int R, bool LDS_TAPS>
__device__ __forceinline__ void convert_items(const ResRate &r, int64_t j0, const float *taps, int tap_stride, const float *s_x, int xf,
                                              int16_t *s_out, int nout, int64_t base_n)
{
    // (LDS_TAPS: the table pointer keeps its LDS address space through the call, so the tap reads are ds_read, not flat loads)
    using TapPtr = typename std::conditional<LDS_TAPS, const __attribute__((address_space(3))) float *, const float *>::type;
    const int NI = r.items, P = r.P;
    const int step = (int)(((int64_t)NI * r.M) / r.L); // input samples between the same-phase outputs of an item (exact for R > 1)
    for (int w = threadIdx.x; w < NI && w < nout; w += 256) {
        const int64_t jm = (j0 + w) * (int64_t)r.M;
        const int64_t n = jm / r.L;
        const int phi = (int)(jm - n * r.L);
        const TapPtr h = (TapPtr)taps + phi * tap_stride;
        const int xb0 = (int)(n - r.Wh + 1 - base_n);
        const float *xp[R];
        float acc[CH][R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            xp[q] = s_x + (w + q * NI < nout ? xb0 + q * step : 0);
#pragma unroll
            for (int c = 0; c < CH; ++c) acc[c][q] = 0.f;
        }
#pragma unroll 4
        for (int k = 0; k < P; ++k) {
            const float hk = h[k];
#pragma unroll
            for (int q = 0; q < R; ++q)
#pragma unroll
                for (int c = 0; c < CH; ++c) acc[c][q] = __builtin_fmaf(hk, xp[q][c * xf + k], acc[c][q]);
        }
#pragma unroll
        for (int q = 0; q < R; ++q)
            if (w + q * NI < nout)
#pragma unroll
                for (int c = 0; c < CH; ++c) s_out[(w + q * NI) * CH + c] = to_pcm(acc[c][q]);
    }
}

// convert_items at the rate's R
template <int CH, bool LDS_TAPS>
__device__ __forceinline__ void convert_tile(const ResRate &r, int64_t j0, const float *taps, int tap_stride, const float *s_x, int xf,
                                             int16_t *s_out, int nout, int64_t base_n)
{
    if (r.R == 4)
        convert_items<CH, 4, LDS_TAPS>(r, j0, taps, tap_stride, s_x, xf, s_out, nout, base_n);
    else if (r.R == 2)
        convert_items<CH, 2, LDS_TAPS>(r, j0, taps, tap_stride, s_x, xf, s_out, nout, base_n);
    else
        convert_items<CH, 1, LDS_TAPS>(r, j0, taps, tap_stride, s_x, xf, s_out, nout, base_n);
}

// the input span of outputs [j0, j0 + nout): it starts at sample base_n and has `groups` groups of 8 samples per channel (host:
// 8 groups <= x_floats).  parity: the element of the source array that sample 0 sits on (mono: position 0 of the span sits on an
// even element)
template <int CH>
struct ResSpan {
    int64_t base_n;
    int groups;
    __device__ __forceinline__ ResSpan(const ResRate &r, int64_t j0, int nout, int64_t parity)
    {
        const int64_t span0 = (j0 * (int64_t)r.M) / r.L - r.Wh + 1;
        base_n = CH == 1 ? span0 - ((parity + span0) & 1) : span0;
        const int64_t n_end = ((j0 + nout - 1) * (int64_t)r.M) / r.L + r.Wh; // last sample any chain of the tile reads
        groups = (int)((n_end - base_n + 8) >> 3);
    }
};

// eight samples per channel from whole words at an even element: 4 words of a mono source, 8 of an interleaved stereo one
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

// group g of the span into the channel planes, two 16-byte words each
template <int CH>
__device__ __forceinline__ void put_group(float *s_x, int xf, int g, const float (&v)[CH][8])
{
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        rs_f4 *d = (rs_f4 *)(s_x + c * xf + 8 * g);
        d[0] = rs_f4{v[c][0], v[c][1], v[c][2], v[c][3]};
        d[1] = rs_f4{v[c][4], v[c][5], v[c][6], v[c][7]};
    }
}

// One converting tile: outputs [j0, j0 + nout) of the rate r -> `words` = (nout CH + 1) / 2 words at element eo (even) of out.
// load_group(n0, v): samples [n0, n0 + 8) of every channel as floats, zero outside the source.
template <int CH, class LoadGroup>
__device__ __forceinline__ void resample_tile(const ResRate &r, const ResLds &lds, const float *taps, float *smem, int64_t j0, int nout,
                                              int64_t parity, int16_t *out, int64_t eo, LoadGroup load_group)
{
    const int tid = threadIdx.x;
    float *s_taps = smem;
    float *s_x = smem + lds.taps_floats;
    const int xf = lds.x_floats;
    int16_t *s_out = (int16_t *)(s_x + CH * xf);
    const ResSpan<CH> sp(r, j0, nout, parity);

    if (r.in_lds) {
        const float *g = taps + r.taps_off;
        const int n = r.L * r.P, P = r.P;
        for (int i = tid; i < n; i += 256) {
            const int ph = (int)((uint32_t)i / (uint32_t)P);
            s_taps[i + ph] = g[i]; // ph * (P + 1) + (i - ph * P)
        }
    }
    {   // output staging cleared: the half word behind an odd count is stored as zero
        uint32_t *o = (uint32_t *)s_out;
        const int words = (min(r.tile_out, lds.out_elems / CH) * CH + 1) >> 1;
        for (int i = tid; i < words; i += 256) o[i] = 0;
    }
    for (int g = tid; g < sp.groups; g += 256) {
        float v[CH][8];
        load_group(sp.base_n + 8 * (int64_t)g, v);
        put_group<CH>(s_x, xf, g, v);
    }
    __syncthreads();

    if (r.in_lds)
        convert_tile<CH, true>(r, j0, s_taps, r.P + 1, s_x, xf, s_out, nout, sp.base_n);
    else
        convert_tile<CH, false>(r, j0, taps + r.taps_off, r.P, s_x, xf, s_out, nout, sp.base_n);
    __syncthreads();

    const int words = (nout * CH + 1) >> 1;
    const uint32_t *so = (const uint32_t *)s_out;
    uint32_t *dst = (uint32_t *)(out + eo);
    int done = 0;
    if (((eo & 7) | ((uintptr_t)out & 15)) == 0) {
        const int quads = words >> 2;
        for (int i = tid; i < quads; i += 256) ((uint4 *)dst)[i] = ((const uint4 *)so)[i];
        done = quads << 2;
    }
    for (int i = done + tid; i < words; i += 256) dst[i] = so[i];
}

// A tile at the output rate: at most kResCopyTile of the `left` samples per channel from element es of src (any parity) to
// element eo (even) of out, word by word (two words and a 2-byte shift when the source is on an odd element)
template <int CH>
__device__ __forceinline__ void copy_words(const int16_t *pcm, int64_t es, int16_t *out, int64_t eo, int64_t left)
{
    const int n = (int)(left < kResCopyTile ? left : kResCopyTile);
    const int elems = n * CH, words = (elems + 1) >> 1;
    uint32_t *dst = (uint32_t *)(out + eo);
    const uint32_t *src = (const uint32_t *)pcm;
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

// The launch of either kernel: the shape checks on what both parameter structs share, the LDS sum, the launch.  The pointer
// checks are the caller's.
template <class Params>
inline hipError_t launch_resample_tiles(const void *mono, const void *stereo, const Params &p, hipStream_t stream)
{
    if ((p.channels != 1 && p.channels != 2) || (p.lds.x_floats & 7) || (p.lds.taps_floats & 3) || (p.lds.out_elems & 1))
        return hipErrorInvalidValue;
    const size_t lds = resample_lds_bytes(p.channels, p.lds);
    if (lds > kLdsMax) return hipErrorInvalidValue;
    const void *fn = p.channels == 2 ? stereo : mono;
    if (hipError_t e = allow_dynamic_lds(fn, lds); e != hipSuccess) return e;
    Params q = p;
    if (hipError_t e = launch_kernel(fn, dim3((unsigned)p.n_tiles), dim3(256), lds, stream, q); e != hipSuccess) return e;
    return hipGetLastError();
}

} // namespace
} // namespace mfx
