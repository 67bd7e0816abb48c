// mfx_sessions.hip -- k_sess_gather, the carry kernel of the session entries (mfx_sessions_host.cpp), and its launcher.
// See DESIGN.md section 5, "Session entries".
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_launch.h"

#include <algorithm>

namespace mfx {

namespace {

// 8 consecutive int16 elements base[o .. o + 7] as one 16-byte word.  `base` is 4-byte aligned, `limit` the element count
// behind it.  wide: 32-bit words at the source's 4-byte alignment -- four when o is even (one global_load_dwordx4 in
// the gfx950 build), five (dwordx4 + dword) and a 2-byte funnel shift (v_alignbyte_b32) per word when it is odd; the last word may reach one element past `limit` (the whole-word read of the last sample that the front ends
// do as well, inside the allocation).  Otherwise eight 2-byte loads.
__device__ __forceinline__ uint4 load8(const int16_t *base, int64_t o, int64_t limit, bool wide)
{
    uint4 v;
    if (wide && o + 8 + (o & 1) <= ((limit + 1) & ~(int64_t)1)) {
        const uint32_t *w = (const uint32_t *)(base + (o & ~(int64_t)1));
        const uint32_t a = w[0], b = w[1], c = w[2], d = w[3];
        if (o & 1) {
            const uint32_t e = w[4];
            v.x = __builtin_amdgcn_alignbyte(b, a, 2);
            v.y = __builtin_amdgcn_alignbyte(c, b, 2);
            v.z = __builtin_amdgcn_alignbyte(d, c, 2);
            v.w = __builtin_amdgcn_alignbyte(e, d, 2);
        } else {
            v = make_uint4(a, b, c, d);
        }
        return v;
    }
    const uint16_t *s = (const uint16_t *)base + o;
    v.x = (uint32_t)s[0] | ((uint32_t)s[1] << 16);
    v.y = (uint32_t)s[2] | ((uint32_t)s[3] << 16);
    v.z = (uint32_t)s[4] | ((uint32_t)s[5] << 16);
    v.w = (uint32_t)s[6] | ((uint32_t)s[7] << 16);
    return v;
}

// grid = (pieces, descriptors), 256 threads.  A work item is one 16-byte word of the destination: first the words of the
// slot's PCM part (carried tail, then the new samples, zeros up to the end of the last word), then the carried static
// rows, then (session transform) the carried rows y, float by float.  Every store of the first two parts is an aligned 16-byte
// word, except static rows whose pitch is no multiple of 4 floats.
__global__ void __launch_bounds__(256) k_sess_gather(SessGatherParams p)
{
    const SessDesc d = p.descs[blockIdx.y];
    const int n_pcm = d.carry_n + d.new_n;
    const int pcm_words = (n_pcm + 7) >> 3;
    const bool vec_rows = ((p.stat_pitch | d.src_pitch) & 3) == 0;
    const int per_row = vec_rows ? (p.cols + 3) >> 2 : p.cols;
    const int stat_items = pcm_words + d.n_rows * per_row;
    const int total = stat_items + d.y_rows * p.y_width; // (the carried rows y are contiguous in both slots: single floats)
    const bool wide = p.narrow == 0;
    // (per_row > 0: floor(j / per_row) as a multiply-high, j < 2^16 rows x columns of one slot)
    const uint32_t magic = per_row > 1 ? 0xffffffffu / (uint32_t)per_row + 1 : 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        if (i < pcm_words) {
            const int e0 = i << 3;
            uint4 v;
            if (e0 + 8 <= d.carry_n) {
                v = load8(p.slot_pcm, d.carry_src + e0, p.slot_elems, wide);
            } else if (e0 >= d.carry_n && e0 + 8 <= n_pcm) {
                v = load8(p.pcm, d.new_src + (e0 - d.carry_n), p.pcm_elems, wide);
            } else { // the word that holds the seam, or the end
                uint32_t h[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int e = e0 + k;
                    uint32_t x = 0;
                    if (e < d.carry_n)
                        x = (uint16_t)p.slot_pcm[d.carry_src + e];
                    else if (e < n_pcm)
                        x = (uint16_t)p.pcm[d.new_src + (e - d.carry_n)];
                    h[k] = x;
                }
                v = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
            }
            *(uint4 *)(p.slot_pcm + d.pcm_dst + e0) = v;
        } else if (i >= stat_items) {
            const int j = i - stat_items;
            p.slot_y[d.y_dst * p.y_width + j] = p.slot_y[d.y_src * p.y_width + j];
        } else {
            const int j = i - pcm_words;
            const int r = per_row > 1 ? (int)__umulhi((uint32_t)j, magic) : j, c = j - r * per_row;
            const float *src = p.slot_stat + (d.row_src + r) * (int64_t)d.src_pitch;
            float *dst = p.slot_stat + (d.row_dst + r) * (int64_t)p.stat_pitch;
            if (vec_rows)
                ((float4 *)dst)[c] = ((const float4 *)src)[c];
            else
                dst[c] = src[c];
        }
    }
}

} // namespace

int sess_gather_items(const SessDesc &d, int stat_pitch, int cols, int y_width)
{
    const bool vec_rows = ((stat_pitch | d.src_pitch) & 3) == 0;
    return ((d.carry_n + d.new_n + 7) >> 3) + d.n_rows * (vec_rows ? (cols + 3) >> 2 : cols) + d.y_rows * y_width;
}

hipError_t launch_sess_gather(const SessGatherParams &p, hipStream_t stream)
{
    if (p.n_descs <= 0 || p.items_max <= 0) return hipSuccess;
    if (p.cols <= 0 || p.stat_pitch < p.cols) return hipErrorInvalidValue;
    // a push is a few hundred words per session: up to 8 blocks of 256 words each
    const int pieces = std::min(8, (p.items_max + 255) / 256);
    return for_seg_slices(p.n_descs, [&](int s0, int n) {
        SessGatherParams q = p;
        q.descs = p.descs + s0;
        q.n_descs = n;
        return launch_kernel((const void *)k_sess_gather, dim3(pieces, n), dim3(256), 0, stream, q);
    });
}

} // namespace mfx
