// stft_fft_asan.cpp -- the host arithmetic of the FFT form of the STFT log-mel front end (mfx_tables.cpp: build_stft_fft_tables,
// build_stft_fft_operands, build_slaney_mel and stft_frame_count at N = 1024 / 2048) under AddressSanitizer + UBSan, CPU only
// (`make asan` in asr-featext-opencl_amd/csrc builds and runs it).  The tables go into buffers of exactly their size; a
// restatement of k_stft_fft_mel's transform -- the same stages, the same index arithmetic lane for lane, in place in a buffer
// of exactly M points with a twiddle table of exactly M -- is run on them and held against a direct DFT in double; the frame
// rule's reflected index stays inside the utterance for every tap of every frame of short utterances.
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../asr-featext-opencl_amd/csrc/mfx_tables.h"

namespace {

typedef std::complex<float> cf;

// one radix-4 Stockham stage as a wave of 64 lanes runs it: all reads, then all writes
void stage4(std::vector<cf> &buf, const std::vector<cf> &tw, int M, int LEN)
{
    const int ST = M / LEN, N1 = LEN / 4, NB = M / 256;
    std::vector<cf> v((size_t)64 * NB * 4);
    for (int lane = 0; lane < 64; ++lane)
        for (int b = 0; b < NB; ++b) {
            const int idx = lane + 64 * b, pp = idx / ST, q = idx % ST;
            for (int r = 0; r < 4; ++r) v[((size_t)lane * NB + b) * 4 + r] = buf.at(q + ST * (pp + r * N1));
        }
    const cf mi(0.f, -1.f);
    for (int lane = 0; lane < 64; ++lane)
        for (int b = 0; b < NB; ++b) {
            const int idx = lane + 64 * b, pp = idx / ST, q = idx % ST;
            const cf *a = &v[((size_t)lane * NB + b) * 4];
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
    const int ST = M / 2, NB = M / 128;
    std::vector<cf> v((size_t)64 * NB * 2);
    for (int lane = 0; lane < 64; ++lane)
        for (int b = 0; b < NB; ++b) {
            const int q = lane + 64 * b;
            v[((size_t)lane * NB + b) * 2] = buf.at(q), v[((size_t)lane * NB + b) * 2 + 1] = buf.at(q + ST);
        }
    for (int lane = 0; lane < 64; ++lane)
        for (int b = 0; b < NB; ++b) {
            const int q = lane + 64 * b;
            const cf a = v[((size_t)lane * NB + b) * 2], c = v[((size_t)lane * NB + b) * 2 + 1];
            buf.at(q) = a + c, buf.at(q + ST) = a - c;
        }
}

// power spectrum of one windowed frame z [N] as the kernel forms it
void frame_power(int N, const std::vector<float> &ops, const float *z, std::vector<float> &P)
{
    const int M = N / 2;
    std::vector<cf> buf(M), tw(M), cs(M + 1);
    for (int k = 0; k < M; ++k) tw[k] = cf(ops.at(N + 2 * k), ops.at(N + 2 * k + 1));
    for (int k = 0; k <= M; ++k) cs[k] = cf(ops.at(2 * N + 2 * k), ops.at(2 * N + 2 * k + 1));
    for (int n = 0; n < M; ++n) buf[n] = cf(z[2 * n], z[2 * n + 1]);
    int len = M;
    for (; len >= 4; len /= 4) stage4(buf, tw, M, len);
    if (len == 2) stage2_last(buf, M);
    P.assign(M + 1, 0.f);
    for (int k = 0; k <= M; ++k) {
        const cf zk = buf.at(k & (M - 1)), zm = buf.at((M - k) & (M - 1));
        const cf s(zk.real() + zm.real(), zk.imag() - zm.imag()), d(zk.real() - zm.real(), zk.imag() + zm.imag());
        const cf X = 0.5f * (s + cs[k] * d);
        P[k] = X.imag() * X.imag() + X.real() * X.real();
    }
}

uint32_t rnd(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

} // namespace

int main()
{
    const double two_pi = 6.283185307179586476925286766559;
    uint32_t seed = 2024;
    int frames = 0;
    for (int N : {1024, 2048}) {
        const int M = N / 2;
        std::vector<float> twid((size_t)2 * M), split((size_t)2 * (M + 1));
        mfx::build_stft_fft_tables(N, twid.data(), split.data());
        for (int k = 0; k < M; ++k)
            if (std::fabs(twid[2 * k] - std::cos(two_pi * k / M)) > 1e-7 || std::fabs(twid[2 * k + 1] + std::sin(two_pi * k / M)) > 1e-7) return 1;
        for (int k = 0; k <= M; ++k)
            if (std::fabs(split[2 * k] + std::sin(two_pi * k / N)) > 1e-7 || std::fabs(split[2 * k + 1] + std::cos(two_pi * k / N)) > 1e-7) return 1;
        std::vector<float> window(N), ops;
        for (int j = 0; j < N; ++j) window[j] = (float)(j + 1) / (float)N; // (the ramp: a reversed tap order shows)
        mfx::build_stft_fft_operands(N, window.data(), ops);
        if (ops.size() != (size_t)3 * N + 2) return 2;
        for (int j = 0; j < N; ++j)
            if (ops[j] != window[j] || ops[N + j] != twid[j]) return 2;
        for (int j = 0; j < 2 * (M + 1); ++j)
            if (ops[2 * N + j] != split[j]) return 2;

        for (int trial = 0; trial < 3; ++trial) { // the transform against a direct DFT in double
            std::vector<float> z(N), P;
            for (int j = 0; j < N; ++j) {
                const float x = trial == 0 ? (j == 5 ? 1.f : 0.f) : (float)((int)(rnd(seed) >> 16) - 32768) / 32768.f;
                z[j] = x * window[j];
            }
            frame_power(N, ops, z.data(), P);
            double scale = 0.0, worst = 0.0;
            std::vector<double> want(M + 1);
            for (int k = 0; k <= M; ++k) {
                double re = 0.0, im = 0.0;
                for (int j = 0; j < N; ++j) {
                    const double a = two_pi * (double)(((int64_t)k * j) % N) / N;
                    re += z[j] * std::cos(a), im -= z[j] * std::sin(a);
                }
                want[k] = re * re + im * im;
                scale = std::max(scale, want[k]);
            }
            for (int k = 0; k <= M; ++k) worst = std::max(worst, std::fabs(P[k] - want[k]));
            if (!(worst <= 2e-5 * scale)) {
                std::printf("stft_fft_asan: N %d trial %d: power off by %g of %g\n", N, trial, worst, scale);
                return 3;
            }
            ++frames;
        }

        for (int S : {1, 160, 441, N / 4, N}) // every tap of every frame stays inside the utterance
            for (int64_t n : {(int64_t)0, (int64_t)N / 2, (int64_t)N / 2 + 1, (int64_t)N / 2 + 2, (int64_t)N, (int64_t)3 * N + 7}) {
                const int64_t T = mfx::stft_frame_count(n, N, S);
                if (T != (n <= N / 2 ? 0 : n / S)) return 4;
                for (int64_t t = 0; t < T; ++t)
                    for (int j : {0, N / 2, N - 1}) {
                        int64_t i = t * S + j - N / 2;
                        if (i < 0) i = -i;
                        if (i >= n) i = 2 * (n - 1) - i;
                        if (i < 0 || i >= n) return 4;
                    }
            }

        for (int nb : {1, 80, 128}) { // the Slaney table at these lengths: spans inside the bins
            const int K1 = N / 2 + 1;
            std::vector<float> w((size_t)nb * K1);
            std::vector<int32_t> beg(nb), len(nb);
            mfx::build_slaney_mel(nb, N, 22050.f, 0.f, 11025.f, w.data(), beg.data(), len.data());
            for (int m = 0; m < nb; ++m)
                if (beg[m] < 0 || len[m] < 0 || beg[m] + len[m] > K1) return 5;
        }
    }
    std::printf("stft_fft_asan: %d frames, tables clean\n", frames);
    return 0;
}
