// Sanitizer run of the host restatement of mfx_batch_set_tensor (csrc/mfx_tables.cpp: tensor_pack_host, tensor_bytes and the two
// integer conversions) under -fsanitize=address,undefined.  Rows and tensor live in heap buffers of exactly the size the
// definition gives them, so a read past the rows or a write past tensor_bytes is caught: odd Tp, Wo = 1, len = 0, len > Tp, Tp = 0,
// the empty batch, both layouts, all three element types.  Every element must be written (the tensor is prefilled with a pattern
// no conversion of the inputs gives) and must be the index rule's value.  Built by `make -C csrc asan`.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../asr-featext-opencl_amd/csrc/mfx_tables.h"

static uint32_t bits_of(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}

static uint32_t cvt(float v, int dtype)
{
    return dtype == mfx::kDtypeF32 ? bits_of(v) : dtype == mfx::kDtypeF16 ? mfx::f32_to_f16_bits(bits_of(v)) : mfx::f32_to_bf16_bits(bits_of(v));
}

int main()
{
    int n = 0;
    struct Case {
        int64_t Tp;
        int Wo;
        std::vector<int32_t> len;
    };
    const Case cases[] = {{5, 1, {0, 3, 9}}, {7, 39, {7, 8}}, {0, 4, {3}}, {1, 1, {0}}, {129, 3, {128, 129, 130, 0, 1}}, {3, 2, {}}, {64, 80, {65}}};
    for (const Case &c : cases) {
        const int64_t B = (int64_t)c.len.size();
        std::vector<int64_t> row0((size_t)B);
        int64_t total = 0;
        for (int64_t u = 0; u < B; ++u) row0[(size_t)u] = total, total += c.len[(size_t)u];
        // (exactly sized: data() of an empty vector may be null, which the restatement must cope with when nothing is read)
        std::vector<float> rows((size_t)(total * c.Wo));
        for (size_t i = 0; i < rows.size(); ++i) rows[i] = 0.37f * (float)((int64_t)i % 1001 - 500);
        for (int layout : {mfx::kTensorTimeMajor, mfx::kTensorChannelMajor})
            for (int dtype : {mfx::kDtypeF32, mfx::kDtypeF16, mfx::kDtypeBf16}) {
                const int64_t bytes = mfx::tensor_bytes(B, c.Wo, c.Tp, dtype);
                const int es = mfx::tensor_elem_bytes(dtype);
                if (bytes != B * c.Tp * c.Wo * es) return 1;
                std::vector<unsigned char> out((size_t)bytes, 0xa5);
                const float pad = -3.25f;
                if (!mfx::tensor_pack_host(rows.data(), row0.data(), c.len.data(), B, c.Wo, c.Tp, layout, dtype, pad, out.data())) return 1;
                for (int64_t u = 0; u < B; ++u)
                    for (int64_t t = 0; t < c.Tp; ++t)
                        for (int64_t w = 0; w < c.Wo; ++w) {
                            const float v = t < c.len[(size_t)u] ? rows[(size_t)((row0[(size_t)u] + t) * c.Wo + w)] : pad;
                            const int64_t idx = layout == mfx::kTensorTimeMajor ? (u * c.Tp + t) * c.Wo + w : (u * c.Wo + w) * c.Tp + t;
                            uint32_t got = 0;
                            std::memcpy(&got, out.data() + idx * es, (size_t)es);
                            if (got != cvt(v, dtype)) return 1;
                        }
                ++n;
            }
    }
    // the conversions at their edges
    if (mfx::f32_to_f16_bits(bits_of(65504.f)) != 0x7bff || mfx::f32_to_f16_bits(bits_of(65520.f)) != 0x7c00) return 1;
    if (mfx::f32_to_f16_bits(bits_of(65520.f) - 1) != 0x7bff || mfx::f32_to_f16_bits(0x33000000u) != 0 || mfx::f32_to_f16_bits(0x33000001u) != 1) return 1;
    if (mfx::f32_to_f16_bits(0x80000000u) != 0x8000 || mfx::f32_to_f16_bits(0x7f800001u) != 0x7e00 || mfx::f32_to_f16_bits(0xffffffffu) != 0xffff) return 1;
    if (mfx::f32_to_bf16_bits(0x3f808000u) != 0x3f80 || mfx::f32_to_bf16_bits(0x3f818000u) != 0x3f82 || mfx::f32_to_bf16_bits(0x7f7fffffu) != 0x7f80) return 1;
    if (mfx::f32_to_bf16_bits(0x7f800001u) != 0x7fc0 || mfx::f32_to_bf16_bits(0x80000000u) != 0x8000 || mfx::f32_to_bf16_bits(0x00008001u) != 0x0001) return 1;
    // outside the limits: refused, nothing written
    unsigned char guard[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    const int64_t r0 = 0;
    const int32_t l0 = 1;
    const float row = 1.f;
    if (mfx::tensor_pack_host(&row, &r0, &l0, 1, 0, 1, 0, 0, 0.f, guard) || mfx::tensor_pack_host(&row, &r0, &l0, 1, 1, 1, 2, 0, 0.f, guard) ||
        mfx::tensor_pack_host(&row, &r0, &l0, 1, 1, 1, 0, 3, 0.f, guard) || mfx::tensor_pack_host(&row, &r0, &l0, 1, 1, (1 << 24) + 1, 0, 0, 0.f, guard))
        return 1;
    if (guard[0] != 1 || guard[7] != 8) return 1;
    if (mfx::tensor_bytes((int64_t)1 << 40, 1023, 1 << 24, 0) != -1) return 1;
    std::printf("tensor_asan: %d tensor clean\n", n);
    return 0;
}
