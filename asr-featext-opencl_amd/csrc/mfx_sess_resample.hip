// mfx_sess_resample.hip -- k_sess_resample: sample-rate conversion in front of a push of the session entries (int16 -> int16),
// and its launcher.  See DESIGN.md section 5, "Session sample-rate conversion".
//
// Output sample j of a STREAM is k_resample's, unchanged: the definition, the layout and the tile body are in
// mfx_resample_dev.h.  What differs is where x comes from.  A piece converts outputs [j_old, j_new) of its stream from stream
// samples [c0, n_new): the samples [c0, n_old) lie in the session's PREVIOUS carry slot, the samples [n_old, n_new) in the
// caller's array; samples before 0 are zero, samples at or after n_new are zero and are reached only by a final push (an open
// stream converts only the outputs whose last tap has arrived: the planner's delivery rule).  A tile is at most tile_out
// consecutive outputs of ONE piece, the first at j_old.  A block
//   0. (the piece's first tile) writes the new carry, stream samples [c1, n_new), to the session's CURRENT carry slot as whole
//      32-bit words -- previous and current slot are different slots of the ping-pong pair, so no block of the launch reads
//      what another writes;
//   1. runs resample_tile, its groups of eight loaded thus: a group inside the caller's part as whole 32-bit words at the
//      array's own alignment, a group inside the carried part as whole words of the slot (four from its 16-byte base's even
//      elements, or the five that hold the group where the carry's parity differs from the array's: mono only), and 2-byte loads
//      only in the groups that hold the seam or an end.
// Pass-through pieces of a push that converts (rate = -1) copy their new samples to the scratch.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_resample_dev.h"

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

template <int CH>
__global__ void __launch_bounds__(256) k_sess_resample(SessResampleParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const SessResTile t = p.tiles[blockIdx.x];
    if (t.move) move_carry<CH>(p, t);
    const int64_t left = t.j_new - t.j0, eo = (t.out_off + (t.j0 - t.j_old)) * CH; // (eo: even)
    if (t.rate < 0) {
        copy_words<CH>(p.pcm, (t.in_off + (t.j0 - t.j_old)) * CH, p.out, eo, left);
        return;
    }
    const ResRate r = p.rates[t.rate];
    const int nout = (int)(left < r.tile_out ? left : r.tile_out);
    if (nout <= 0) return; // (a piece that only moves its carry)
    resample_tile<CH>(r, p.lds, p.taps, smem, t.j0, nout, t.in_off - t.n_old, p.out, eo, [&](int64_t n0, float (&v)[CH][8]) {
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
    });
}

} // namespace

hipError_t launch_sess_resample(const SessResampleParams &p, hipStream_t stream)
{
    if (p.n_tiles <= 0) return hipSuccess;
    if (!p.out || !p.carry || !p.tiles || !p.rates || !p.taps) return hipErrorInvalidValue; // (pcm may be null: no piece brings samples)
    return launch_resample_tiles((const void *)k_sess_resample<1>, (const void *)k_sess_resample<2>, p, stream);
}

} // namespace mfx
