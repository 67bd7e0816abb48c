"""Float64 restatement of the tail stages (delta / delta-delta, CMN / CVN / MINMAX) with float32 rounding bounds.

Plain numpy: no GPU, no oracle.  An output row is [static | d | dd]; the static part is a copy, the rest is a function
of the static columns of the same utterance, so rows can be checked against a restatement of THEIR OWN statics and the
tolerance comes from float32 rounding alone -- no front-end noise enters it.

Notation: u = 2^-24 (unit roundoff of float32), gamma(k) = k u / (1 - k u).

Denormals: the kernels are built with hipcc's defaults for gfx950, which keep float32 denormals (no flush-to-zero; FMA
and add handle them at full rate on gfx9), so no flush term is needed.  Gradual underflow still replaces the RELATIVE
rounding error by an absolute one of at most half the denormal spacing, 2^-150, per rounding, and delta_quot's remainder
step is exact only away from that range (mfx_delta_dev.h); ETA below is that term, one 2^-149 per operation of the chain.
It is ~1e-44 and never decides a comparison of real data.
"""
import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -149


def gamma(k):
    return k * U / (1.0 - k * U)


def _regress(xp, lo, n, l):
    """sum_{j=1..l} j (xp[i + lo + j] - xp[i + lo - j]) for i < n, its sum of absolute terms, and 2 sum j^2."""
    num = np.zeros((n,) + xp.shape[1:])
    absnum = np.zeros_like(num)
    for j in range(1, l + 1):
        d = xp[lo + j:lo + j + n] - xp[lo - j:lo - j + n]
        num += j * d
        absnum += j * np.abs(d)
    return num, absnum, 2.0 * sum(j * j for j in range(1, l + 1))


def delta_ref(statics, dyn, l1, l2):
    """statics [T][cols] (float64 of the rows' own static columns) -> (d, dd, b_d, b_dd), each [T][cols]; dd and b_dd are
    None unless dyn == 2.

    The STATICS are clamped at the utterance ends, x[clamp(t, 0, T - 1)] for t = -D .. T - 1 + D with D = l1 (+ l2); the
    delta of the l2 virtual rows on either side is computed from them and is NOT clamped (mfcccpu.cpp:234-263).
    Bounds: one rounding per difference, one per multiply-add of the chain (the first-entered term meets all l + 1 of
    them and its own difference: gamma(l + 2) covers every term), one for the quotient (u |result|); the delta-delta
    adds what the bounds of the deltas it reads allow.  These bounds are the tolerance: no factor on top."""
    x = np.asarray(statics, np.float64)
    T = x.shape[0]
    assert dyn in (1, 2) and l1 > 0 and (dyn == 1 or l2 > 0)
    l2p = l2 if dyn == 2 else 0
    D = l1 + l2p
    if T == 0:
        z = np.zeros_like(x)
        return z, (z if dyn == 2 else None), z, (z if dyn == 2 else None)
    xp = x[np.clip(np.arange(-D, T + D), 0, T - 1)]
    n1 = T + 2 * l2p                                   # delta of t = -l2' .. T - 1 + l2'; x[t] = xp[t + D] = xp[i + l1]
    num, absnum, den1 = _regress(xp, l1, n1, l1)
    d = num / den1
    b_d = gamma(l1 + 2) * absnum / den1 + U * np.abs(d) + (l1 + 3) * ETA
    if dyn == 1:
        return d, None, b_d, None
    num2, absnum2, den2 = _regress(d, l2, T, l2)
    dd = num2 / den2
    prop = np.zeros_like(dd)
    for j in range(1, l2 + 1):
        prop += j * (b_d[l2 + j:l2 + j + T] + b_d[l2 - j:l2 - j + T])
    b_dd = prop / den2 + gamma(l2 + 2) * absnum2 / den2 + U * np.abs(dd) + (l2 + 3) * ETA
    return d[l2:l2 + T], dd, b_d[l2:l2 + T], b_dd


def assert_tail_consistent(rows, cols, dyn, l1, l2, what=""):
    """Every row and every column of the delta groups of `rows` [T][cols (1 + dyn)] against delta_ref of the rows' own
    static columns.  Fails with the worst err / bound, its row and its column; returns {"d": worst, "dd": worst}."""
    rows = np.asarray(rows)
    assert rows.ndim == 2 and rows.shape[1] == cols * (1 + dyn), "%s: %s is not [T][%d x %d]" % (what, rows.shape, 1 + dyn, cols)
    worst = {}
    if dyn == 0:
        return worst
    assert np.isfinite(rows).all(), "%s: non-finite values" % what
    r = rows.astype(np.float64)
    d, dd, b_d, b_dd = delta_ref(r[:, :cols], dyn, l1, l2)
    for g, (name, ref, bound) in enumerate((("d", d, b_d), ("dd", dd, b_dd))[:dyn], 1):
        got = r[:, g * cols:(g + 1) * cols]
        if got.size == 0:
            worst[name] = 0.0
            continue
        ratio = np.abs(got - ref) / bound
        t, c = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        worst[name] = float(ratio[t, c])
        assert ratio[t, c] <= 1.0, "%s: %s group: err / bound = %.3g at row %d of %d, column %d of %d (got %.9g, want %.9g, bound %.3g)" % (
            what, name, ratio[t, c], t, rows.shape[0], c, cols, got[t, c], ref[t, c], bound[t, c])
    return worst


def norm_stats_ref(x, kind, stat_rows):
    """normalizercpu.cpp:22-89 as k_norm_stats states it, over the first stat_rows rows of x [T][cols] (float32 rows of
    ONE column group): (mean, mult, b_mean, b_mult) in float64, to be compared with the handle's float32 statistics.

    S = sum v in double; S2 = sum of double(float32(v) * float32(v)) -- the product is rounded to float32 first, as the
    kernel and the reference do; mean = S / n; CVN mult = sqrt((n - 1) / (S2 - S (S / n))); MINMAX mult = 1 / max(|min -
    mean32|, |max - mean32|) with mean32 the float32 mean; CMN mult = 1.
    Bounds: mean -- its float32 rounding u |mean| and the double summation n 2^-53 sum|v| / n; CVN -- u |mult| and
    1/2 |mult| n 2^-53 S2 / (S2 - S^2 / n) (the summation error of S2 against the cancelled difference); MINMAX -- two
    float32 roundings (the subtraction, the reciprocal).  Degenerate statistics (n = 1 under CVN: 0 / 0, or 0 over the
    rounding error of one float32 square) come out as the kernel's own doubles give them: non-finite or zero."""
    x32 = np.asarray(x, np.float32)[:stat_rows]
    n = x32.shape[0]
    assert n == stat_rows and n > 0
    v = x32.astype(np.float64)
    S = v.sum(0)
    S2 = (x32 * x32).astype(np.float64).sum(0)
    mean = S / n
    eps = 2.0 ** -53
    b_mean = U * np.abs(mean) + n * eps * np.abs(v).sum(0) / n
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == 1:
            mult, b_mult = np.ones_like(mean), np.zeros_like(mean)
        elif kind == 2:
            var = S2 - S * (S / n)
            mult = np.sqrt((n - 1) / var)
            b_mult = U * np.abs(mult) + 0.5 * np.abs(mult) * n * eps * S2 / var
        else:
            m32 = mean.astype(np.float32).astype(np.float64)
            mult = 1.0 / np.maximum(np.abs(v.min(0) - m32), np.abs(v.max(0) - m32))
            b_mult = gamma(2) * np.abs(mult)
    return mean, mult, b_mean, b_mult


def norm_apply_f32(x32, mean32, mult32, kind):
    """fl(fl(x - mean) mult) in float32 (fl(x - mean) for CMN): the kernel's (v - st[c]) * st[cols + c] is a difference
    times a factor, which no compiler contracts into one FMA, so the GPU rows are expected to be the SAME BITS."""
    x32 = np.asarray(x32, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        y = x32 - np.asarray(mean32, np.float32)
        if kind != 1:
            y = y * np.asarray(mult32, np.float32)
    assert y.dtype == np.float32
    return y


def same_bits(a, b):
    """Equal float32 bit patterns, NaN matching NaN of any payload."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def assert_norm_consistent(y, x, st, kind, nad, cols, stat_rows, what=""):
    """One utterance of a normalising handle against its norm = NONE twin.  y, x: [T][G cols] rows of the handle and of
    the twin; st [Gs][2][cols]: the handle's own statistics (mean, multiplier), Gs = G after the deltas (nad) else 1.
    Statistics within norm_stats_ref's bounds of the twin's rows; rows the same bits as norm_apply_f32 of the twin's rows
    with the handle's statistics.  Columns whose statistics are non-finite must be so on both sides and are the only ones
    left out.  Returns (worst mean err / bound, worst multiplier err / bound, columns kept [Gs][cols])."""
    y, x, st = np.asarray(y, np.float32), np.asarray(x, np.float32), np.asarray(st, np.float32)
    G = x.shape[1] // cols
    Gs = G if nad else 1
    assert y.shape == x.shape and st.shape == (Gs, 2, cols), (what, y.shape, x.shape, st.shape)
    w_mean = w_mult = 0.0
    keep = np.zeros((Gs, cols), bool)
    for g in range(Gs):
        xg, yg = x[:, g * cols:(g + 1) * cols], y[:, g * cols:(g + 1) * cols]
        mean, mult, b_mean, b_mult = norm_stats_ref(xg, kind, stat_rows)
        ok = np.isfinite(mean) & np.isfinite(mult) & np.isfinite(b_mult)
        got_ok = np.isfinite(st[g, 0]) & np.isfinite(st[g, 1])
        assert np.array_equal(ok, got_ok), "%s group %d: degenerate statistics differ: columns %s" % (what, g, np.nonzero(ok != got_ok)[0])
        keep[g] = ok
        for name, got, ref, b in (("mean", st[g, 0], mean, b_mean), ("multiplier", st[g, 1], mult, b_mult)):
            if kind == 1 and name == "multiplier":
                continue                                # (CMN: the slot is not used by the apply)
            err = np.abs(got.astype(np.float64)[ok] - ref[ok])
            if err.size == 0:
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(err == 0, 0.0, err / b[ok])
            c = int(np.argmax(ratio))
            assert ratio[c] <= 1.0, "%s group %d: %s err / bound = %.3g at column %d (got %.9g, want %.17g)" % (
                what, g, name, ratio[c], np.nonzero(ok)[0][c], got[ok][c], ref[ok][c])
            if name == "mean":
                w_mean = max(w_mean, float(ratio[c]))
            else:
                w_mult = max(w_mult, float(ratio[c]))
        want = norm_apply_f32(xg, st[g, 0], st[g, 1], kind)
        if not same_bits(yg[:, ok], want[:, ok]):
            eq = (np.ascontiguousarray(yg).view(np.uint32) == want.view(np.uint32)) | (np.isnan(yg) & np.isnan(want))
            bad = np.argwhere(~eq & ok[None, :])
            t, c = bad[0]
            raise AssertionError("%s group %d: %d normalised values differ in bits, first at row %d column %d: got %.9g, want %.9g" % (
                what, g, len(bad), t, c, yg[t, c], want[t, c]))
    return w_mean, w_mult, keep
