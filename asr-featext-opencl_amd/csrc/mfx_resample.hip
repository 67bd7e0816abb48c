// mfx_resample.hip -- k_resample: per-utterance sample-rate conversion of the batch entries' PCM (int16 -> int16), and its
// launcher.  See DESIGN.md, "Sample-rate conversion".  The definition, the layout and the tile body are in mfx_resample_dev.h,
// shared with k_sess_resample; this file says where a tile's fields and a group's eight samples come from: the utterance in
// the caller's array, or zero outside [0, n_in) of it.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_resample_dev.h"

namespace mfx {

namespace {

template <int CH>
__global__ void __launch_bounds__(256) k_resample(ResampleParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const ResTile t = p.tiles[blockIdx.x];
    const int64_t left = t.n_out - t.j0, eo = (t.out_off + t.j0) * CH; // (eo: even)
    if (t.rate < 0) {
        copy_words<CH>(p.pcm, (t.in_off + t.j0) * CH, p.out, eo, left);
        return;
    }
    const ResRate r = p.rates[t.rate];
    const int nout = (int)(left < r.tile_out ? left : r.tile_out);
    resample_tile<CH>(r, p.lds, p.taps, smem, t.j0, nout, t.in_off, p.out, eo, [&](int64_t n0, float (&v)[CH][8]) {
        if (n0 >= 0 && n0 + 8 <= t.n_in) {
            words_to_floats<CH>((const uint32_t *)(p.pcm + (t.in_off + n0) * CH), v); // an even element: a whole word
        } else { // a group that holds an end of the utterance: what lies outside is zero
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int64_t n = n0 + q;
                const bool in = n >= 0 && n < t.n_in;
#pragma unroll
                for (int c = 0; c < CH; ++c) v[c][q] = in ? (float)p.pcm[(t.in_off + n) * CH + c] : 0.f;
            }
        }
    });
}

} // namespace

hipError_t launch_resample(const ResampleParams &p, hipStream_t stream)
{
    if (p.n_tiles <= 0) return hipSuccess;
    // (rates and taps are the plan's own uploads and are not judged here; launch_sess_resample judges its two)
    if (!p.pcm || !p.out || !p.tiles) return hipErrorInvalidValue;
    return launch_resample_tiles((const void *)k_resample<1>, (const void *)k_resample<2>, p, stream);
}

} // namespace mfx
