// mfx_kaldi_opts.hip -- k_kaldi_front_opts: k_kaldi_front (mfx_kaldi.hip) for kaldi_flags of mfx_create_kaldi != 0 -- snip_edges = false,
// the frame's log-energy, the HTK column order (include/mfx.h, method 7, "Options").  Its own translation unit and kernel, so that
// a handle without options runs the code, the registers and the blocks per CU it always had.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include "mfx_dev.h"
#include "mfx_launch.h"
#include "mfx_tile_dev.h"
#include "mfx_kaldi_dev.h"

namespace mfx {

namespace {

__global__ void __launch_bounds__(256) k_kaldi_front_opts(KaldiParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    kaldi_front<true>(p, smem);
}

} // namespace

hipError_t launch_kaldi_opts(const KaldiParams &p, size_t lds, hipStream_t stream)
{
    const void *fn = (const void *)k_kaldi_front_opts;
    if (hipError_t e = allow_dynamic_lds(fn, lds); e != hipSuccess) return e;
    KaldiParams q = p;
    return launch_kernel(fn, dim3(p.n_chunks), dim3(256), lds, stream, q);
}

} // namespace mfx
