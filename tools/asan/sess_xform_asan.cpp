// sess_xform_asan.cpp -- the session transform's host arithmetic (mfx_tables.cpp: session_xform_step, pack_sess_xform_groups)
// under AddressSanitizer + UBSan, CPU only (`make asan` in asr-featext-opencl_amd/csrc builds and runs it).  Push sequences
// through the planner's two steps: the delivered rows add up to the stream's frames, the carried rows stay inside left +
// right, every row an output reads lies in the push's slot; the packer's groups cover every delivered row once and no block
// mixes transforms.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../asr-featext-opencl_amd/csrc/mfx_tables.h"

int main()
{
    int nq = 0;
    const int W = 400, S = 160;
    for (int left : {0, 1, 4, 32})
        for (int right : {0, 1, 4, 32})
            for (int D : {0, 2, 6, 20}) {
                const int64_t pushes[] = {0, 1, S - 1, S, W - 1, W, 3000, 0, 7, 2 * W + 3, 16000, 1, 0};
                const int count = (int)(sizeof(pushes) / sizeof(pushes[0]));
                int64_t n = 0, E = 0, Ey = 0, Ex = 0, total = 0, rows = 0;
                for (int k = 0; k < count; ++k) {
                    const bool fin = k + 1 == count;
                    mfx::SessionStep st;
                    mfx::SessionXformStep xs;
                    total += pushes[k];
                    const int64_t Ex_old = Ex;
                    const int32_t n_y = mfx::session_step(W, S, D, n, E, pushes[k], fin, st);
                    rows += mfx::session_xform_step(left, right, Ey, Ex, n_y, fin, xs);
                    if (xs.n_out < 0 || xs.carry_rows < 0 || xs.carry_rows > left + right || Ey != E || Ex > Ey) return 1;
                    if (xs.lo != -xs.src_row0 || (Ex_old > left && xs.src_row0 != left)) return 1;
                    const int slot_rows = xs.carry_rows + n_y;
                    for (int r = 0; r < xs.n_out; ++r)
                        for (int c = 0; c <= left + right; ++c) {
                            int o = r - left + c;
                            o = o < xs.lo ? xs.lo : o > xs.hi ? xs.hi : o;
                            if (xs.src_row0 + o < 0 || xs.src_row0 + o >= slot_rows) return 1;
                        }
                }
                const int64_t T = mfx::frame_count(total, W, S);
                if (rows != (T > 0 ? T : 0) || Ey != 0 || Ex != 0) return 1;
                ++nq;
            }
    int np = 0;
    for (int G : {1, 2, 4})
        for (int n : {0, 1, 5, 13, 1000}) {
            std::vector<int32_t> n_out(n), xf(n);
            std::vector<mfx::SessXfCut> gp;
            std::vector<mfx::SessXfPack> bl;
            for (int i = 0; i < n; ++i) n_out[i] = (i * 7) % 41 == 3 ? 0 : (i * 13) % 50, xf[i] = (i * 5) % 3;
            mfx::pack_sess_xform_groups(n_out.data(), xf.data(), n, G, gp, bl);
            std::vector<int32_t> seen(n, 0);
            for (const mfx::SessXfCut &g : gp) {
                if (g.rows < 1 || g.rows > 16 || g.r0 + g.rows > n_out[g.piece]) return 1;
                seen[g.piece] += g.rows;
            }
            for (int i = 0; i < n; ++i)
                if (seen[i] != n_out[i]) return 1;
            size_t next = 0;
            for (const mfx::SessXfPack &k : bl) {
                if ((size_t)k.g0 != next || k.ng < 1 || k.ng > G) return 1;
                for (int g = k.g0; g < k.g0 + k.ng; ++g)
                    if (xf[gp[g].piece] != k.xf) return 1;
                next += k.ng;
            }
            if (next != gp.size()) return 1;
            ++np;
        }
    std::printf("sess_xform_asan: %d push sequences, %d work lists clean\n", nq, np);
    return 0;
}
