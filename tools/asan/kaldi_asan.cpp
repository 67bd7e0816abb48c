// kaldi_asan.cpp -- the host arithmetic of the Kaldi front end (mfx_tables.cpp: build_kaldi_mel, build_kaldi_spans,
// build_kaldi_dct, build_kaldi_operands) under AddressSanitizer + UBSan, CPU only (`make asan` in asr-featext-opencl_amd/csrc
// builds and runs it).  The two tables go into buffers of exactly their size; a restatement of k_kaldi_front's transform -- the
// same stages, the same index arithmetic lane for lane with lanes beyond the butterflies idle, in place in a buffer of exactly
// N / 2 points with twiddle and split tables of exactly N / 2 -- is run on a windowed, pre-emphasised frame and held against a
// direct DFT in double at all three lengths.
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../asr-featext-opencl_amd/csrc/mfx_tables.h"

namespace {

typedef std::complex<float> cf;

// one radix-4 Stockham stage as a wave of 64 lanes runs it: lane l < M / 4 owns butterfly l; all reads, then all writes
void stage4(std::vector<cf> &buf, const std::vector<cf> &tw, int M, int LEN)
{
    const int ST = M / LEN, N1 = LEN / 4, NBF = M / 4;
    std::vector<cf> v((size_t)64 * 4);
    for (int lane = 0; lane < 64; ++lane) {
        if (lane >= NBF) continue;
        const int pp = lane / ST, q = lane % ST;
        for (int r = 0; r < 4; ++r) v[(size_t)lane * 4 + r] = buf.at(q + ST * (pp + r * N1));
    }
    const cf mi(0.f, -1.f);
    for (int lane = 0; lane < 64; ++lane) {
        if (lane >= NBF) continue;
        const int pp = lane / ST, q = lane % ST;
        const cf *a = &v[(size_t)lane * 4];
        const cf b0 = a[0] + a[2], b1 = a[0] - a[2], b2 = a[1] + a[3], b3 = a[1] - a[3];
        const cf o0 = b0 + b2, o2 = b0 - b2, o1 = b1 + mi * b3, o3 = b1 - mi * b3;
        const int y = q + ST * (4 * pp);
        buf.at(y) = o0;
        if (LEN == 4) {
            buf.at(y + ST) = o1, buf.at(y + 2 * ST) = o2, buf.at(y + 3 * ST) = o3;
        } else {
            buf.at(y + ST) = o1 * tw.at(pp * ST);
            buf.at(y + 2 * ST) = o2 * tw.at(2 * pp * ST);
            buf.at(y + 3 * ST) = o3 * tw.at(3 * pp * ST);
        }
    }
}

void stage2_last(std::vector<cf> &buf, int M)
{
    const int ST = M / 2;
    std::vector<cf> v((size_t)64 * 2);
    for (int lane = 0; lane < 64 && lane < ST; ++lane) v[(size_t)lane * 2] = buf.at(lane), v[(size_t)lane * 2 + 1] = buf.at(lane + ST);
    for (int lane = 0; lane < 64 && lane < ST; ++lane) {
        const cf a = v[(size_t)lane * 2], c = v[(size_t)lane * 2 + 1];
        buf.at(lane) = a + c, buf.at(lane + ST) = a - c;
    }
}

// power spectrum, bins k < N / 2, of one frame z [N] as the kernel forms it from the operands
void frame_power(int N, const std::vector<float> &ops, const float *z, std::vector<float> &P)
{
    const int M = N / 2;
    std::vector<cf> buf(M), tw(M), cs(M);
    for (int k = 0; k < M; ++k) tw[k] = cf(ops.at(N + 2 * k), ops.at(N + 2 * k + 1));
    for (int k = 0; k < M; ++k) cs[k] = cf(ops.at(2 * N + 2 * k), ops.at(2 * N + 2 * k + 1));
    for (int n = 0; n < M; ++n) buf[n] = cf(z[2 * n], z[2 * n + 1]);
    int len = M;
    for (; len >= 4; len /= 4) stage4(buf, tw, M, len);
    if (len == 2) stage2_last(buf, M);
    P.assign(M, 0.f);
    for (int k = 0; k < M; ++k) {
        const cf zk = buf.at(k), zm = buf.at((M - k) & (M - 1));
        const cf s(zk.real() + zm.real(), zk.imag() - zm.imag()), d(zk.real() - zm.real(), zk.imag() + zm.imag());
        const cf X = 0.5f * (s + cs.at(k) * d);
        P[k] = X.imag() * X.imag() + X.real() * X.real();
    }
}

uint32_t rnd(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

} // namespace

int main()
{
    const double two_pi = 6.283185307179586476925286766559;
    uint32_t seed = 2025;
    int frames = 0, tables = 0;

    // the two table builders into exactly sized buffers, over the limits of the method
    for (int N : {128, 256, 512})
        for (int M : {1, 23, 80, 128})
            for (float low : {0.f, 20.f}) {
                const float sr = N == 512 ? 16000.f : N == 256 ? 8000.f : 4000.f;
                double high = 0.0;
                if (!mfx::kaldi_freqs_ok(sr, low, -100.f, &high) || high != (double)sr / 2 - 100.0) return 1;
                const int K = N / 2;
                std::vector<float> w((size_t)M * K), spans;
                std::vector<int32_t> beg(M), len(M), meta;
                mfx::build_kaldi_mel(M, N, sr, low, high, w.data(), beg.data(), len.data());
                mfx::build_kaldi_spans(M, N, sr, low, high, spans, meta);
                if (meta.size() != (size_t)3 * M || spans.empty()) return 2;
                for (int m = 0; m < M; ++m) {
                    if (beg[m] < 0 || len[m] < 0 || beg[m] + len[m] > K) return 2;
                    if (meta[m] != beg[m] || meta[M + m] != len[m] || meta[2 * M + m] < 0 || (size_t)meta[2 * M + m] + len[m] > spans.size()) return 2;
                    for (int j = 0; j < len[m]; ++j)
                        if (spans.at(meta[2 * M + m] + j) != w[(size_t)m * K + beg[m] + j]) return 2;
                    for (int k = 0; k < K; ++k)
                        if (!(w[(size_t)m * K + k] >= 0.f && w[(size_t)m * K + k] <= 1.f)) return 2;
                }
                for (int C : {1, M}) {
                    if (C > M) continue;
                    for (float Q : {0.f, 22.f}) {
                        std::vector<float> G((size_t)C * M);
                        mfx::build_kaldi_dct(M, C, Q, G.data());
                        if (std::fabs(G[0] - std::sqrt(1.0 / M)) > 1e-7) return 3;
                        ++tables;
                    }
                }
            }
    if (mfx::kaldi_freqs_ok(16000.f, 20.f, 8001.f) || mfx::kaldi_freqs_ok(16000.f, -1.f, 0.f) || mfx::kaldi_freqs_ok(16000.f, 4000.f, -4000.f) ||
        mfx::kaldi_freqs_ok(16000.f, 20.f, NAN))
        return 4;
    static_assert(mfx::kaldi_shape_ok(65, 1, 1, 0) && mfx::kaldi_shape_ok(512, 512, 128, 128) && !mfx::kaldi_shape_ok(64, 1, 1, 0) &&
                      !mfx::kaldi_shape_ok(513, 1, 1, 0) && !mfx::kaldi_shape_ok(400, 401, 1, 0) && !mfx::kaldi_shape_ok(400, 160, 129, 0) &&
                      !mfx::kaldi_shape_ok(400, 160, 23, 24),
                  "the limits of a shape");
    static_assert(mfx::kaldi_fft_size(65) == 128 && mfx::kaldi_fft_size(128) == 128 && mfx::kaldi_fft_size(129) == 256 &&
                      mfx::kaldi_fft_size(256) == 256 && mfx::kaldi_fft_size(257) == 512 && mfx::kaldi_fft_size(512) == 512,
                  "the next power of two");

    // the transform against a direct DFT in double, at the shortest and the longest window of every length
    for (int W : {65, 128, 129, 200, 256, 257, 400, 512}) {
        const int N = mfx::kaldi_fft_size(W), M = N / 2;
        std::vector<float> window(W), ops;
        for (int j = 0; j < W; ++j) window[j] = (float)(j + 1) / (float)W; // (the ramp: a reversed tap order shows)
        mfx::build_kaldi_operands(W, N, window.data(), ops);
        if (ops.size() != (size_t)3 * N) return 5;
        for (int j = 0; j < N; ++j)
            if (ops[j] != (j < W ? window[j] : 0.f)) return 5;
        for (int k = 0; k < M; ++k) {
            if (std::fabs(ops[N + 2 * k] - std::cos(two_pi * k / M)) > 1e-7 || std::fabs(ops[N + 2 * k + 1] + std::sin(two_pi * k / M)) > 1e-7) return 5;
            if (std::fabs(ops[2 * N + 2 * k] + std::sin(two_pi * k / N)) > 1e-7 || std::fabs(ops[2 * N + 2 * k + 1] + std::cos(two_pi * k / N)) > 1e-7) return 5;
        }
        for (int trial = 0; trial < 3; ++trial) {
            std::vector<float> x(W), z(N, 0.f), P;
            int64_t s = 0;
            for (int j = 0; j < W; ++j) {
                x[j] = trial == 0 ? (j == 5 ? 32767.f : 0.f) : (float)((int)(rnd(seed) >> 16) - 32768);
                s += (int64_t)x[j];
            }
            const float mean = (float)s / (float)W, c = 0.97f;
            for (int j = 0; j < W; ++j) {
                const float d = x[j] - mean, dp = (j == 0 ? x[0] : x[j - 1]) - mean;
                z[j] = std::fmaf(-c, dp, d) * ops[j];
            }
            frame_power(N, ops, z.data(), P);
            double scale = 0.0, worst = 0.0;
            std::vector<double> want(M);
            for (int k = 0; k < M; ++k) {
                double re = 0.0, im = 0.0;
                for (int j = 0; j < N; ++j) {
                    const double a = two_pi * (double)(((int64_t)k * j) % N) / N;
                    re += z[j] * std::cos(a), im -= z[j] * std::sin(a);
                }
                want[k] = re * re + im * im;
                scale = std::max(scale, want[k]);
            }
            for (int k = 0; k < M; ++k) worst = std::max(worst, std::fabs(P[k] - want[k]));
            if (!(worst <= 2e-5 * scale)) {
                std::printf("kaldi_asan: W %d N %d trial %d: power off by %g of %g\n", W, N, trial, worst, scale);
                return 6;
            }
            ++frames;
        }
    }
    std::printf("kaldi_asan: %d frames, %d tables clean\n", frames, tables);
    return 0;
}
