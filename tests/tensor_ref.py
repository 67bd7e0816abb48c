"""Reference of the dense padded tensor output (mfx_batch_set_tensor, include/mfx.h), in numpy with torch on the CPU as the
conversion oracle.  Never the code under test.

Input: the float32 rows of a run WITHOUT the attachment, out_rows and the lengths L_u.  Output: the tensor built by the index
rule -- element (u, t, c) = cvt(rows[out_rows[u] + t][c]) for t < min(L_u, Tp), else cvt(pad) -- as [B][Tp][Wo] (TIME_MAJOR) or
[B][Wo][Tp] (CHANNEL_MAJOR); float32, float16, or the uint16 bits of bfloat16."""
import numpy as np
import torch

TIME_MAJOR, CHANNEL_MAJOR = 0, 1
F32, F16, BF16 = 0, 1, 2
NP_DTYPE = {F32: np.float32, F16: np.float16, BF16: np.uint16}
BITS_DTYPE = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}


def convert(x, dtype):
    """float32 array -> the element type, by torch's CPU conversion (round to nearest even)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == F32:
        return x.copy()
    t = torch.from_numpy(x)
    if dtype == F16:
        return t.to(torch.float16).numpy()
    return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def tensor_ref(rows, out_rows, lengths, Tp, layout, dtype, pad):
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    Wo = rows.shape[1]
    B = len(out_rows)
    dense = np.empty((B, Tp, Wo), np.float32)
    dense.view(np.uint32)[...] = np.float32(pad).view(np.uint32)
    for u in range(B):
        n = int(min(int(lengths[u]), Tp))
        if n > 0:
            dense[u, :n] = rows[int(out_rows[u]):int(out_rows[u]) + n]
    out = convert(dense, dtype)
    if layout == CHANNEL_MAJOR:
        out = np.ascontiguousarray(out.transpose(0, 2, 1))
    return out


def same_bits(got, want, dtype):
    """Bit for bit, but that a NaN is compared as a NaN (its payload is not pinned for the 16-bit types)."""
    g = np.ascontiguousarray(got).view(BITS_DTYPE[dtype]).reshape(-1)
    w = np.ascontiguousarray(want).view(BITS_DTYPE[dtype]).reshape(-1)
    if g.shape != w.shape:
        return False
    if dtype == F32:
        return bool(np.array_equal(g, w))
    exp, man = (0x7c00, 0x03ff) if dtype == F16 else (0x7f80, 0x007f)
    g_nan = ((g & exp) == exp) & ((g & man) != 0)
    w_nan = ((w & exp) == exp) & ((w & man) != 0)
    return bool(np.array_equal(g_nan, w_nan) and np.array_equal(g[~g_nan], w[~w_nan]))


def edge_values():
    """The float32 inputs of the conversion checks, as uint32 bit patterns:
    (a) every 16-bit upper half crossed with the lower halves {0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff} (bfloat16's
        ties and their neighbours, every exponent, NaNs and infinities included);
    (b) every float16 value as float32, every midpoint of two neighbours, and the float32 just below and just above it;
    (c) the float16 overflow edge: 65504, the float32 below 65520, 65520 (and just above);
    (d) the float16 subnormal edges: 2^-24 and 2^-25 with neighbours, the largest subnormal, the smallest normal;
    (e) +-0 and +-inf."""
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    a = np.concatenate([hi | lo for lo in (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff)])
    h = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    h = h[np.isfinite(h)]
    f = h.astype(np.float32)  # exact
    pos = np.sort(f[f >= 0])
    mid = ((pos[:-1].astype(np.float64) + pos[1:].astype(np.float64)) * 0.5).astype(np.float32)  # exact in float32
    mb = mid.view(np.uint32)
    mids = np.concatenate([mb, mb - 1, mb + 1])
    b = np.concatenate([f.view(np.uint32), mids, mids | 0x80000000])
    c = np.array([np.float32(65504.0).view(np.uint32), np.float32(65520.0).view(np.uint32) - 1, np.float32(65520.0).view(np.uint32),
                  np.float32(65520.0).view(np.uint32) + 1], np.uint32)
    c = np.concatenate([c, c | 0x80000000])
    sub = []
    for e in (-24, -25, -26, -14, -15):
        v = np.float32(2.0 ** e).view(np.uint32)
        sub += [v - 1, v, v + 1]
    sub += [np.float32(2.0 ** -14 - 2.0 ** -24).view(np.uint32), np.float32(2.0 ** -14 - 2.0 ** -25).view(np.uint32),
            np.float32(1.5 * 2.0 ** -24).view(np.uint32), np.float32(2.5 * 2.0 ** -24).view(np.uint32)]
    d = np.array(sub, np.uint32)
    d = np.concatenate([d, d | 0x80000000])
    e = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000], np.uint32)
    return np.concatenate([a, b, c, d, e]).astype(np.uint32)
