"""Per-speaker normalisation (mfx_batch_set_speakers) restated on top of tests/tail_ref.py.  Plain numpy: no GPU, no oracle.

A speaker's statistics are those of ONE segment holding the rows of all its utterances: the rows of the norm = NONE twin are
concatenated in ascending utterance order (a prior enters as the rows of the earlier batches, in front) and handed to
tail_ref.norm_stats_ref.  That function's bounds hold for any order of the double additions, so they are the tolerance with
no factor on top, however the kernels chunk and pool.  The rows themselves are checked bit for bit against
tail_ref.norm_apply_f32 of the twin's rows with the handle's OWN statistics.
"""
import numpy as np

from tail_ref import norm_apply_f32, norm_stats_ref, same_bits


def host_lists_ref(utt_spk, frames, n_spk):
    """The CSR lists of mfx_host_speaker_lists, restated: (off [n_spk + 1], list)."""
    per = [[] for _ in range(n_spk)]
    for u, (s, t) in enumerate(zip(utt_spk, frames)):
        if t > 0:
            per[int(s)].append(u)
    off = np.zeros(n_spk + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in per])
    return off, np.array([u for p in per for u in p], np.int32)


def merge_ref(parts):
    """sharding.merge_speaker_acc restated with numpy reductions over the rank axis."""
    count = np.sum([np.asarray(c, np.int64) for c, _ in parts], axis=0)
    acc = np.stack([np.asarray(a, np.float64) for _, a in parts])
    out = np.empty_like(acc[0])
    out[:, 0], out[:, 1] = acc[:, :, 0].sum(0), acc[:, :, 1].sum(0)
    out[:, 2], out[:, 3] = acc[:, :, 2].min(0), acc[:, :, 3].max(0)
    return count, out


def assert_speaker_consistent(ys, xs, st, kind, cols, prior=(), what=""):
    """One speaker of a handle with a speaker list against the norm = NONE twin.  ys, xs: the handle's and the twin's rows of
    the speaker's utterances of this batch, ascending ([T_u][width] each; utterances without rows may be among them);
    st [2][Wn]: the handle's statistics of the speaker (mean, multiplier), Wn = G cols normalised columns; prior: the twin's
    rows of the speaker's utterances of earlier batches.  Statistics within norm_stats_ref's bounds of the pooled rows;
    normalised columns the same bits as norm_apply_f32 of the twin's rows with st.  Columns whose statistics are not finite
    must be so on both sides and are the only ones left out.  Returns (worst mean err / bound, worst multiplier err / bound,
    columns kept [G][cols])."""
    st = np.asarray(st, np.float32)
    Wn = st.shape[1]
    assert st.shape == (2, Wn) and Wn % cols == 0, (what, st.shape, cols)
    G = Wn // cols
    pooled = np.concatenate([np.asarray(x, np.float32)[:, :Wn] for x in list(prior) + list(xs)], axis=0)
    n = pooled.shape[0]
    assert n > 0, "%s: a speaker without rows has no reference" % what
    w_mean = w_mult = 0.0
    keep = np.zeros((G, cols), bool)
    for g in range(G):
        sl = slice(g * cols, (g + 1) * cols)
        mean, mult, b_mean, b_mult = norm_stats_ref(pooled[:, sl], kind, n)
        ok = np.isfinite(mean) & np.isfinite(mult) & np.isfinite(b_mult)
        got_ok = np.isfinite(st[0, sl]) & np.isfinite(st[1, sl])
        assert np.array_equal(ok, got_ok), "%s group %d: degenerate statistics differ: columns %s" % (what, g, np.nonzero(ok != got_ok)[0])
        keep[g] = ok
        for name, got, ref, b in (("mean", st[0, sl], mean, b_mean), ("multiplier", st[1, sl], mult, b_mult)):
            if kind == 1 and name == "multiplier":
                continue                                # (CMN: the slot is not used by the apply)
            err = np.abs(got.astype(np.float64)[ok] - ref[ok])
            if err.size == 0:
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(err == 0, 0.0, err / b[ok])
            c = int(np.argmax(ratio))
            assert ratio[c] <= 1.0, "%s group %d: %s err / bound = %.3g at column %d (got %.9g, want %.17g, %d pooled rows)" % (
                what, g, name, ratio[c], np.nonzero(ok)[0][c], got[ok][c], ref[ok][c], n)
            if name == "mean":
                w_mean = max(w_mean, float(ratio[c]))
            else:
                w_mult = max(w_mult, float(ratio[c]))
        for i, (y, x) in enumerate(zip(ys, xs)):
            y, x = np.asarray(y, np.float32), np.asarray(x, np.float32)
            assert y.shape == x.shape, (what, i, y.shape, x.shape)
            want = norm_apply_f32(x[:, sl], st[0, sl], st[1, sl], kind)
            assert same_bits(y[:, sl][:, ok], want[:, ok]), "%s group %d: rows of the speaker's utterance %d (%d rows) differ in bits" % (
                what, g, i, y.shape[0])
    return w_mean, w_mult, keep
