// mfx_tensor.hip -- dense padded tensor output of the batch entries (mfx_batch_set_tensor), and its launcher.  See DESIGN.md
// section 5, "Tensor output".
//
// The finished float32 rows [total_rows][Wo] of a run become the caller's tensor in one read and one write:
//   element (u, t, c) = cvt(rows[row0_u + t][c]) for t < len_u = min(L_u, Tp), else cvt(pad_value)
//   TIME_MAJOR    at (u Tp + t) Wo + c        CHANNEL_MAJOR    at (u Wo + c) Tp + t        (64-bit indices)
// A regular grid, no work list: block (u, i) owns rows t in [i R, min((i + 1) R, Tp)) of utterance u, R = kTensorTileRows, real
// rows and pad rows alike, so every element of the tensor has exactly one writer and is written on every run.
//
//   k_tensor_pack_tm  the tile's n Wo source floats are contiguous and so are its destination elements: a straight stream.
//                     The destination is only element-aligned: at most 3 scalar elements lead up to the first address that is a
//                     multiple of four elements, whole quads follow (16-byte stores of float32, 8-byte stores of the 16-bit
//                     types), at most 3 scalar elements end the tile.  A quad's source is one 16-byte load where the source is
//                     aligned with the destination, else four loads.  No LDS.
//   k_tensor_pack_cm  the tile's real rows are staged into an LDS image at the odd pitch Wo | 1 dwords (consecutive lanes write
//                     consecutive dwords), then every wave writes, for one column c at a time, consecutive t: a lane reads
//                     image[t][c] -- t P + c with P odd: the 32 lanes of a group on 32 banks -- and the wave writes one run of
//                     n elements.  The 16-bit types pack two t per lane (the two reads are then 2-way on a bank, far below
//                     what HBM asks of the LDS).  A column's base is 2-byte aligned only -- Tp odd, or d_out itself -- so a
//                     run whose first element is on an odd half-word starts with a single element, and one whose last pair is
//                     cut ends with one.
// The conversions are the compiler's (__float2half_rn, __float2bfloat16: v_cvt_f16_f32 and v_cvt_pk_bf16_f32 on gfx950); float32
// elements move as 32-bit words and never meet arithmetic.  Nothing here is atomic and no result depends on timing.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "mfx_dev.h"
#include "mfx_launch.h"

namespace mfx {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// an element type: its storage and the conversion from the bits of a float32
template <int DT>
struct Elem;
template <>
struct Elem<kDtypeF32> {
    typedef uint32_t type;
    static __device__ __forceinline__ uint32_t cvt(uint32_t b) { return b; }
};
template <>
struct Elem<kDtypeF16> {
    typedef uint16_t type;
    static __device__ __forceinline__ uint16_t cvt(uint32_t b) { return __half_as_ushort(__float2half_rn(__uint_as_float(b))); }
};
template <>
struct Elem<kDtypeBf16> {
    typedef uint16_t type;
    static __device__ __forceinline__ uint16_t cvt(uint32_t b) { return __bfloat16_as_ushort(__float2bfloat16(__uint_as_float(b))); }
};

// what block (u, i) owns
struct TensorTile {
    int u;
    int t0, n;       // rows [t0, t0 + n) of the utterance's Tp
    int real;        // the first `real` of them hold rows of the run, the rest the pad value
    const uint32_t *src; // row t0 of the utterance (not read when real == 0)
};

__device__ __forceinline__ TensorTile tensor_tile(const TensorParams &p)
{
    constexpr int R = kTensorTileRows;
    const unsigned tiles = (unsigned)(p.Tp + R - 1) / R;
    const unsigned du = blockIdx.x / tiles;
    const int i = (int)(blockIdx.x - du * tiles);
    TensorTile tl;
    tl.u = p.u0 + (int)du;
    const TensorUtt ut = p.utt[tl.u];
    const int L = p.voiced ? p.voiced[tl.u] : ut.T;
    const int len = min(max(L, 0), p.Tp);
    if (i == 0 && threadIdx.x == 0) p.len[tl.u] = len;
    tl.t0 = i * R;
    tl.n = min(R, p.Tp - tl.t0);
    tl.real = min(max(len - tl.t0, 0), tl.n);
    tl.src = (const uint32_t *)p.rows + (ut.row0 + tl.t0) * (int64_t)p.Wo;
    return tl;
}

template <int DT>
__global__ void __launch_bounds__(256) k_tensor_pack_tm(TensorParams p)
{
    typedef typename Elem<DT>::type E;
    const TensorTile tl = tensor_tile(p);
    const int tid = threadIdx.x;
    const int count = tl.n * p.Wo, real = tl.real * p.Wo; // elements of the tile, and those of them that come from rows
    const uint32_t *src = tl.src;
    E *dst = (E *)p.out + ((int64_t)tl.u * p.Tp + tl.t0) * p.Wo;
    const uint32_t padb = __float_as_uint(p.pad_value);
    const E pade = Elem<DT>::cvt(padb);
    // elements in front of the first address that is a multiple of four elements
    const int head = min((int)((4u - (unsigned)(((uintptr_t)dst / sizeof(E)) & 3)) & 3), count);
    const int quads = (count - head) >> 2;
    const bool src16 = (((uintptr_t)(src + head)) & 15) == 0;
    if (tid < head) dst[tid] = tid < real ? Elem<DT>::cvt(src[tid]) : pade;
    for (int q = tid; q < quads; q += 256) {
        const int j = head + 4 * q;
        u32x4 w;
        if (j + 4 <= real) {
            if (src16)
                w = *(const u32x4 *)(src + j);
            else
                w = u32x4{src[j], src[j + 1], src[j + 2], src[j + 3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = j + k < real ? src[j + k] : padb;
        }
        if constexpr (sizeof(E) == 4) {
            *(u32x4 *)(dst + j) = w;
        } else {
            u32x2 o;
            o[0] = (uint32_t)Elem<DT>::cvt(w[0]) | ((uint32_t)Elem<DT>::cvt(w[1]) << 16);
            o[1] = (uint32_t)Elem<DT>::cvt(w[2]) | ((uint32_t)Elem<DT>::cvt(w[3]) << 16);
            *(u32x2 *)(dst + j) = o;
        }
    }
    const int j = head + 4 * quads + tid; // at most 3 elements behind the last quad
    if (j < count) dst[j] = j < real ? Elem<DT>::cvt(src[j]) : pade;
}

template <int DT>
__global__ void __launch_bounds__(256) k_tensor_pack_cm(TensorParams p)
{
    typedef typename Elem<DT>::type E;
    extern __shared__ uint32_t s_img[]; // [kTensorTileRows][Wo | 1]
    const TensorTile tl = tensor_tile(p);
    const int tid = threadIdx.x;
    const int Wo = p.Wo, P = Wo | 1;
    const int real = tl.real * Wo;
    const uint32_t *src = tl.src;
    const uint32_t padb = __float_as_uint(p.pad_value);
    const E pade = Elem<DT>::cvt(padb);
    // i / Wo for i < 2^16 (the image holds at most 160 KB / 4 = 40960 floats)
    const uint32_t magic = Wo > 1 ? 0xffffffffu / (uint32_t)Wo + 1 : 0;
    auto stage = [&](int i, uint32_t v) {
        const int r = Wo > 1 ? (int)__umulhi((uint32_t)i, magic) : i;
        s_img[r * P + (i - r * Wo)] = v;
    };
    const int quads = (((uintptr_t)src & 15) == 0) ? real >> 2 : 0;
    for (int q = tid; q < quads; q += 256) {
        const u32x4 w = ((const u32x4 *)src)[q];
#pragma unroll
        for (int k = 0; k < 4; ++k) stage(4 * q + k, w[k]);
    }
    for (int i = 4 * quads + tid; i < real; i += 256) stage(i, src[i]);
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    const int n = tl.n, nr = tl.real;
    for (int c = wave; c < Wo; c += 4) {
        E *col = (E *)p.out + ((int64_t)tl.u * Wo + c) * p.Tp + tl.t0;
        if constexpr (sizeof(E) == 4) {
            for (int t = lane; t < n; t += 64) col[t] = t < nr ? s_img[t * P + c] : padb;
        } else {
            // a run that starts on an odd half-word: its first element alone, pairs from the second on
            const int h = (int)(((uintptr_t)col >> 1) & 1); // (n >= 1: the grid has no empty tile)
            if (h && lane == 0) col[0] = 0 < nr ? Elem<DT>::cvt(s_img[c]) : pade;
            for (int k = lane; h + 2 * k < n; k += 64) {
                const int t = h + 2 * k;
                const E a = t < nr ? Elem<DT>::cvt(s_img[t * P + c]) : pade;
                if (t + 1 < n) {
                    const E b = t + 1 < nr ? Elem<DT>::cvt(s_img[(t + 1) * P + c]) : pade;
                    *(uint32_t *)(col + t) = (uint32_t)a | ((uint32_t)b << 16);
                } else {
                    col[t] = a; // (the run's last pair is cut)
                }
            }
        }
    }
}

const void *tensor_kernel(int layout, int dtype)
{
    if (layout == kTensorTimeMajor)
        return dtype == kDtypeF32   ? (const void *)k_tensor_pack_tm<kDtypeF32>
               : dtype == kDtypeF16 ? (const void *)k_tensor_pack_tm<kDtypeF16>
                                    : (const void *)k_tensor_pack_tm<kDtypeBf16>;
    return dtype == kDtypeF32   ? (const void *)k_tensor_pack_cm<kDtypeF32>
           : dtype == kDtypeF16 ? (const void *)k_tensor_pack_cm<kDtypeF16>
                                : (const void *)k_tensor_pack_cm<kDtypeBf16>;
}

} // namespace

bool tensor_params_ok(const TensorParams &p)
{
    if (p.Tp < 0 || p.Tp > kTensorPadMax || p.Wo < 1 || p.u0 < 0 || p.u1 < p.u0) return false;
    if ((p.layout != kTensorTimeMajor && p.layout != kTensorChannelMajor) || p.dtype < kDtypeF32 || p.dtype > kDtypeBf16) return false;
    if (p.layout == kTensorChannelMajor && tensor_lds_bytes(p.Wo) > kLdsMax) return false;
    if ((int64_t)p.Wo * kTensorTileRows > 0x7fffffff / 2) return false; // (a tile's element count is an int)
    const int64_t tiles = (p.Tp + kTensorTileRows - 1) / kTensorTileRows;
    return (int64_t)(p.u1 - p.u0) * tiles <= 0x7fffffff;
}

hipError_t launch_tensor_pack(const TensorParams &p, hipStream_t stream)
{
    if (!tensor_params_ok(p)) return hipErrorInvalidValue;
    if (p.u1 == p.u0 || p.Tp == 0) return hipSuccess; // (no element to write; len_u = 0 is what the setter left)
    if (!p.rows || !p.out || !p.utt || !p.len) return hipErrorInvalidValue;
    if (((uintptr_t)p.rows & 3) != 0 || ((uintptr_t)p.out & (uintptr_t)(tensor_elem_bytes(p.dtype) - 1)) != 0) return hipErrorInvalidValue;
    const unsigned tiles = (unsigned)((p.Tp + kTensorTileRows - 1) / kTensorTileRows);
    const void *fn = tensor_kernel(p.layout, p.dtype);
    size_t lds = 0;
    if (p.layout == kTensorChannelMajor) {
        lds = tensor_lds_bytes(p.Wo);
        if (hipError_t e = allow_dynamic_lds(fn, lds); e != hipSuccess) return e;
    }
    TensorParams q = p;
    return launch_kernel(fn, dim3((unsigned)(p.u1 - p.u0) * tiles), dim3(256), lds, stream, q);
}

} // namespace mfx
