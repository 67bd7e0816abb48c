// mfx_pitchfeat.hip -- Kaldi's pitch features from the pitch track of the batch entries (mfx_batch_set_pitch_feats), their
// paste into the rows of a run, and the two launchers.  See DESIGN.md section 5, "Pitch features"; the definition
// k_pitch_feats follows operation for operation is in include/mfx.h.
//
//   k_pitch_feats  one block of 256 threads per tile of at most 256 consecutive rows of one utterance (an utterance tiling,
//                  UttTiling of mfx_kernels.h, at kPitchFeatRows).  The block evaluates w (the probability of voicing that weighs the sliding mean) and
//                  p = ln(rate / lag) once for its rows and a halo of max(left, D) rows before and max(right, D) rows behind
//                  them, cut at the utterance, into LDS as doubles.  Then one row per thread: the window's two sums, ascending,
//                  from LDS -- consecutive lanes read consecutive 8-byte words, every row sums its own window from its first
//                  row on, so that no value depends on the tiling -- the regression over p, the POV value, and F floats out.
//   k_pitch_paste  one output float per thread over the rows of the run: [ narrow row (Wd) | feats (F) ] into rows of Wd + F
//                  floats, at any 4-byte alignment of the destination.
// Nothing here is atomic, no result depends on timing or on the other utterances of the batch.
#include "mfx_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>

#include "mfx_dev.h"
#include "mfx_launch.h"

// every double operation below is rounded on its own
#pragma clang fp contract(off)

namespace mfx {

namespace {

constexpr int kFeatSpan = kPitchFeatRows + 2048; // the tile's rows (= threads per block) and the largest halo on both sides

// grid = tiles of the utterance range
__global__ void __launch_bounds__(kPitchFeatRows) k_pitch_feats(PitchFeatParams q)
{
    __shared__ double s_w[kFeatSpan], s_p[kFeatSpan];
    const int tid = threadIdx.x;
    const UttItem tl = utt_item<kPitchFeatRows>(q.tiles, q.segs, q.tiles.first + blockIdx.x);
    const int T = tl.T, t0 = tl.t0, nr = tl.n;
    const int D = q.D;
    const int lo0 = max(0, t0 - max(q.left, D)), hi0 = min(T - 1, t0 + nr - 1 + max(q.right, D));
    const float *track = q.pitch + 2 * tl.row0;
    const double rate = (double)q.sample_rate;

    // ---- w and p of the tile's rows and their halo, once
    for (int i = tid; i <= hi0 - lo0; i += kPitchFeatRows) {
        const float lag = track[2 * (int64_t)(lo0 + i)], rho = track[2 * (int64_t)(lo0 + i) + 1];
        const double n = fmin(1.0, fmax(-1.0, (double)rho));
        const double a = fabs(n);
        const double a1 = a - 1.0;
        const double x1 = 7.5 * a1, x2 = -10.0 * a, x3 = 20.0 * a1;
        const double e1 = 5.4 * exp(x1), e2 = 4.8 * a, e3 = 2.0 * exp(x2), e4 = 4.2 * exp(x3);
        double r = -5.2 + e1;
        r = r + e2;
        r = r - e3;
        r = r + e4;
        const double en = exp(-r);
        const double dn = 1.0 + en;
        s_w[i] = 1.0 / dn;
        const double ratio = rate / (double)lag;
        s_p[i] = log(ratio);
    }
    __syncthreads();
    if (tid >= nr) return; // (nothing below synchronises)

    const int t = t0 + tid;
    const double pt = s_p[t - lo0];
    float *out = q.feats + (tl.row0 + t) * (int64_t)q.F;
    if (q.columns & kPfPov) {
        const double n = fmin(1.0, fmax(-1.0, (double)track[2 * (int64_t)t + 1]));
        const double b = 1.0001 - n;
        const double y = pow(b, 0.15) - 1.0;
        const double v = (double)q.pov_scale * y;
        *out++ = (float)(v + (double)q.pov_offset);
    }
    if (q.columns & kPfNorm) {
        const int lo = max(0, t - q.left) - lo0, hi = min(T - 1, t + q.right) - lo0;
        double sw = 0.0, sp = 0.0;
        for (int i = lo; i <= hi; ++i) {
            const double w = s_w[i];
            const double wp = w * s_p[i];
            sw = sw + w;
            sp = sp + wp;
        }
        const double mean = sp / sw;
        const double d = pt - mean;
        *out++ = (float)((double)q.pitch_scale * d);
    }
    if (q.columns & kPfDelta) {
        double num = 0.0;
        for (int l = 1; l <= D; ++l) {
            const double d = s_p[min(T - 1, t + l) - lo0] - s_p[max(0, t - l) - lo0];
            const double ld = (double)l * d;
            num = num + ld;
        }
        const double v = (double)q.delta_scale * num;
        *out++ = (float)(v / q.delta_den);
    }
    if (q.columns & kPfRaw) *out++ = (float)pt;
}

// grid-stride over the (row, column) pairs of the run's rows [row0, row0 + rows)
__global__ void __launch_bounds__(256) k_pitch_paste(PitchPasteParams q)
{
    const int Wy = q.Wd + q.F;
    const int64_t n = q.rows * Wy;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = q.row0 + i / Wy;
        const int c = (int)(i % Wy);
        q.out[r * Wy + c] = c < q.Wd ? q.narrow[r * q.Wd + c] : q.feats[r * q.F + (c - q.Wd)];
    }
}

} // namespace

bool pitch_feat_params_ok(const PitchFeatParams &q)
{
    if (q.columns < 1 || q.columns > 15 || q.F != __builtin_popcount((unsigned)q.columns)) return false;
    return q.left >= 0 && q.left <= 1024 && q.right >= 0 && q.right <= 1024 && q.D >= 1 && q.D <= 16 && q.delta_den > 0.0;
}

hipError_t launch_pitch_feats(const PitchFeatParams &q, hipStream_t stream)
{
    if (q.tiles.count <= 0) return hipSuccess; // (no utterance of the range has a frame)
    if (!pitch_feat_params_ok(q) || !q.pitch || !q.feats || q.tiles.rows != kPitchFeatRows) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pitch_feats, dim3(q.tiles.count), dim3(kPitchFeatRows), 0, stream, q);
    return hipGetLastError();
}

hipError_t launch_pitch_paste(const PitchPasteParams &q, hipStream_t stream)
{
    if (q.rows <= 0) return hipSuccess;
    if (q.Wd < 1 || q.F < 1 || q.F > 4 || !q.narrow || !q.feats || !q.out) return hipErrorInvalidValue;
    const int64_t blocks = (q.rows * (q.Wd + q.F) + 1023) / 1024; // (four values per thread where the run is large)
    hipLaunchKernelGGL(k_pitch_paste, dim3((unsigned)std::min<int64_t>(blocks, 1 << 20)), dim3(256), 0, stream, q);
    return hipGetLastError();
}

} // namespace mfx
