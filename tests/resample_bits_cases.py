"""Cases of tests/test_resample_bits_gpu.py, shared with tests/golden/make_resample_bits_parent.py (which recorded the converted
samples of commit 7d4edbf, the last one before k_resample and k_sess_resample got their one tile body): the smallest inputs at
which each path of the two kernels is taken.  Every case names the geometry it is there for (`want`), and `geometry(pkg, case)`
asks the library for it on the CPU.

A batch case is the ragged batch of tests/test_resample_gpu.py (its builder, `ragged`) for ONE rate pair, full-scale noise
throughout: lengths 0, 1, 2, Wh - 1, Wh, 2 Wh + 1 and around one and two tiles, every other utterance on an odd input offset,
three pass-through utterances; the samples are the whole scratch (mfx_debug_read kind 8, laid out by mfx_batch_resample_layout).

A session case is one stream of 2 edge + 3 samples (edge: the shortest input that fills a tile) through one session, read
through mfx_sessions_converted_read, cut
  a   one push, behind a first sample pushed alone;
  b   pieces of 1, Wh - 1, Wh, 9, then 8 k + 1 (k = 1, 2, 4, ...) and the rest, every piece at an odd element of the array;
  c   the cuts of b, the pieces alternating between even and odd elements: on mono the carry's parity then differs from the
      array's, the five-word form of the group loader;
each ended by a final push of length 0.  The first piece of every cut is too short to convert anything: its tile only moves the
carry.  `paths(pkg, case)` restates the group loader's conditions on the host, and NEED says which of them each cut is there for.
The three cuts of a stream deliver the same samples, so the fixture holds them once per stream (`stored`).  A mixed case pushes a
converting session beside a pass-through session whose piece has an odd length and sits at an odd offset."""
import numpy as np

import sess_resample_drive as RD
import test_resample_gpu as TR

SR = RD.SR


def _want(L, M, P, R, in_lds, tile_out):
    return dict(L=L, M=M, P=P, R=R, in_lds=in_lds, tile_out=tile_out)


# (in_hz, out_hz, channels) -> geometry at the default zeros and rolloff
TABLE = {
    (48000, 16000, 1): _want(1, 3, 38, 4, True, 2048),          # L = 1: every lane reads the same tap (a broadcast)
    (48000, 16000, 2): _want(1, 3, 38, 4, True, 1340),          # stereo halves the tile
    (8000, 16000, 1): _want(2, 1, 14, 4, True, 2048),           # interpolation: lanes share words
    (8000, 16000, 2): _want(2, 1, 14, 4, True, 2048),
    (44100, 16000, 1): _want(160, 441, 34, 4, True, 1920),      # items a multiple of L, not a power of two
    (44100, 16000, 2): _want(160, 441, 34, 4, True, 1280),
    (11025, 16000, 1): _want(640, 441, 14, 2, True, 1280),      # R = 2
    (12345, 16000, 1): _want(3200, 2469, 14, 1, False, 2048),   # R = 1, taps through the caches
    (12345, 16000, 2): _want(3200, 2469, 14, 1, False, 2048),
    (44142, 44100, 1): _want(1050, 1051, 14, 1, True, 2048),    # R = 1 with a staged table: 75 424 bytes of LDS, over 64 KB
    (200000, 44100, 1): _want(441, 2000, 56, 4, False, 1764),   # R > 1 with an unstaged table
    (200000, 44100, 2): _want(441, 2000, 56, 2, False, 882),    # stereo drops to R = 2
}
SESSION_RATES = (48000, 8000, 44100, 12345)
MIXED_RATE = 44100
# the paths of k_sess_resample's group loader each cut must take (paths())
NEED = {"a": {"caller", "end", "move_only"}, "b": {"caller", "carry", "seam", "end", "move_only"},
        "c": {"caller", "carry", "seam", "end", "move_only"}}

CASES = {}
for (r_in, r_out, ch), w in TABLE.items():
    CASES["batch_%d_%d_ch%d" % (r_in, r_out, ch)] = dict(kind="batch", r_in=r_in, r_out=r_out, ch=ch, want=w,
                                                         stored="batch_%d_%d_ch%d" % (r_in, r_out, ch))
for r_in in SESSION_RATES:
    for ch in (1, 2):
        for cut in "abc":
            CASES["sess_%d_ch%d_%s" % (r_in, ch, cut)] = dict(kind="session", r_in=r_in, r_out=SR, ch=ch, cut=cut,
                                                              want=TABLE[(r_in, SR, ch)], stored="sess_%d_ch%d" % (r_in, ch))
for ch in (1, 2):
    CASES["sess_mixed_ch%d" % ch] = dict(kind="mixed", r_in=MIXED_RATE, r_out=SR, ch=ch, want=TABLE[(MIXED_RATE, SR, ch)],
                                         stored="sess_mixed_ch%d" % ch)


def geometry(pkg, c):
    """The case's geometry: L, M, P and tile_out as the library answers them, R and the table's place restated from
    resample_geometry (the restated tile_out is held to the library's)."""
    ch = c["ch"]
    h, L, M, P = pkg.mfcc.host_resample_taps(c["r_in"], c["r_out"])
    tile = pkg.mfcc.host_resample_tile(c["r_in"], c["r_out"], channels=ch)

    def fit(budget):
        return max(budget - P - 32, 0) * L // M
    to = min(2048, fit(8192 // ch))
    if to < 64:
        to = min(2048, fit(16384 // ch))
    to = max(to & ~1, 2)
    if 2 * L > to:
        R, items = 1, to
    else:
        R = 4 if 4 * L <= to else 2
        items = L * (to // (R * L))
    assert R * items == tile, (c, R, items, tile)
    return _want(L, M, P, R, L * (P + 1) <= 16384, tile)


def lds_bytes(c):
    """Dynamic LDS of a launch that serves the case's rate alone: table | span per channel | output staging."""
    w, ch = c["want"], c["ch"]
    taps = (w["L"] * (w["P"] + 1) + 3) & ~3 if w["in_lds"] else 0
    span = (w["tile_out"] - 1) * w["M"] // w["L"] + w["P"] + 3
    return 4 * (taps + ch * (((span + 7) & ~7) + 8)) + 2 * w["tile_out"] * ch


# ---- session cases ---------------------------------------------------------------------------------------------------------

def stream_length(c):
    w = c["want"]
    return 2 * -(-w["tile_out"] * w["M"] // w["L"]) + 3


def pushes(c):
    """[(length, final, parity of the array element the piece starts on)] of a session case."""
    n, Wh = stream_length(c), c["want"]["P"] // 2
    if c["cut"] == "a":
        return [(1, False, 0), (n - 1, False, 0), (0, True, 0)]
    lens, k = [1, Wh - 1, Wh, 9], 1
    while sum(lens) + 8 * k + 1 < n:
        lens.append(8 * k + 1)
        k *= 2
    lens.append(n - sum(lens))
    assert sum(lens) == n and min(lens) > 0
    return [(m, False, 1 if c["cut"] == "b" else i & 1) for i, m in enumerate(lens)] + [(0, True, 1)]


def piece_paths(pkg, c, state, length, fin, in_off):
    """What k_sess_resample does for one piece of a session at `state` = (N, J), restated from its group loader:
      move_only  nothing converted, a carry to move
      caller     a group of eight read as whole words of the caller's array
      carry      ... of the carry slot, from an even element
      carry5     ... from an odd element: the five words that hold it (mono)
      seam       a group across the end of the carry, sample by sample
      end        a group across the start or the end of the stream's samples at hand, sample by sample
    Returns (the set, the state after the piece)."""
    w, ch = c["want"], c["ch"]
    L, M, Wh, tile = w["L"], w["M"], w["P"] // 2, w["tile_out"]
    st = pkg.mfcc.host_session_resample_step(c["r_in"], c["r_out"], state, length, fin)
    n_old, n_new, j_old = state[0], state[0] + length, state[1]
    c0, j_new = n_old - st["carry_in"], j_old + st["n_out"]
    out = set()
    if st["n_out"] == 0 and st["carry_out"] > 0:
        out.add("move_only")
    for j0 in range(j_old, j_new, tile):
        nout = min(tile, j_new - j0)
        span0 = j0 * M // L - Wh + 1
        base = span0 - ((in_off + span0 - n_old) & 1) if ch == 1 else span0
        n_end = (j0 + nout - 1) * M // L + Wh
        n0 = base + 8 * np.arange((n_end - base + 8) >> 3)
        caller = (n0 >= n_old) & (n0 + 8 <= n_new)
        carried = (n0 >= c0) & (n0 + 8 <= n_old)
        odd = (((n0 - c0) * ch) & 1) == 1                # (a slot starts on a multiple of 8 elements)
        seam = ~caller & ~carried & (n0 < n_old) & (n0 + 8 > n_old) & (n0 + 8 > c0) & (n_old > c0)
        for name, mask in (("caller", caller), ("carry", carried & ~odd), ("carry5", carried & odd), ("seam", seam),
                           ("end", ~caller & ~carried & ~seam)):
            if mask.any():
                out.add(name)
    return out, st["state"]


def paths(pkg, c):
    """The union of piece_paths over a session case's pushes (the random gap in front of a piece does not matter: only the
    parity of its offset does)."""
    out, state = set(), (0, 0)
    for length, fin, par in pushes(c):
        p, state = piece_paths(pkg, c, state, length, fin, par)
        out |= p
    return out


def needed(c):
    """The paths a session case is there for.  The five-word form needs a carried group that starts on an odd element: the
    span starts at c0 or one sample before it, so the group is the second one, samples [c0 + 7, c0 + 15), and the carry must hold
    15 samples.  An open stream carries 2 Wh - 1 = P - 1 samples or a few more, so only a rate with P >= 16 can take it (48000 and
    44100 Hz do; 8000 and 12345 Hz, P = 14, carry 13 and never reach it, however they are cut)."""
    five = c["cut"] == "c" and c["ch"] == 1 and c["want"]["P"] >= 16
    return NEED[c["cut"]] | ({"carry5"} if five else set())


def _push(m, ch, pieces):
    """One push: pieces [(session, samples [n][ch], final, parity)], each behind a gap of +-32767 that puts it on an element
    of that parity.  Returns the converted samples per piece."""
    parts, pos, ids, offs, lens, fins = [], 0, [], [], [], []
    for sid, x, fin, par in pieces:
        k = 2 + ((pos + par) & 1)
        parts.append(np.where(np.arange(k * ch) % 2 == 0, 32767, -32767).astype(np.int16).reshape(k, ch))
        pos += k
        assert pos & 1 == par
        ids.append(sid), offs.append(pos), lens.append(len(x)), fins.append(int(fin))
        parts.append(x)
        pos += len(x)
    parts.append(np.full((2 + pos % 2, ch), -32767, np.int16))
    m.sessions_plan(ids, offs, lens, fins)
    m.sessions_run_host(np.concatenate(parts, 0).reshape(-1))
    return m.sessions_converted_read(len(ids))


def _run_session(pkg, c):
    ch, n = c["ch"], stream_length(c)
    x = RD.stream(0, n, c["r_in"], c["r_in"] % 97, ch)
    m = RD.make(pkg, channels=ch)
    try:
        m.sessions_set_rates([c["r_in"]])
        m.sessions_create(1, n)
        got, o = [], 0
        for length, fin, par in pushes(c):
            got.append(_push(m, ch, [(0, x[o:o + length], fin, par)])[0])
            o += length
    finally:
        m.close()
    assert o == n
    return np.concatenate(got, 0)


def _run_mixed(pkg, c):
    ch = c["ch"]
    x = RD.stream(0, 3001, c["r_in"], 7, ch)
    p = RD.stream(0, 4097, SR, 8, ch)                        # the pass-through piece: odd length, odd offset, two copy tiles
    m = RD.make(pkg, channels=ch)
    try:
        m.sessions_set_rates([c["r_in"], SR])
        m.sessions_create(2, 4097)
        m.sessions_select_rate(1, 1)
        a = _push(m, ch, [(0, x, False, 0), (1, p, False, 1)])
        b = _push(m, ch, [(1, p[:0], True, 1), (0, x[:0], True, 0)])
    finally:
        m.close()
    assert np.array_equal(a[1], p) and len(b[0]) == 0     # (the copy is held to its source: the fixture need not repeat it)
    return np.concatenate([a[0], b[1]], 0)


def _run_batch(pkg, c):
    d = TR.ragged(pkg, [c["r_in"]], c["r_out"], channels=c["ch"], kinds=1)
    m = TR.make(pkg, sr=c["r_out"], channels=c["ch"])
    try:
        m.batch_plan_rates(d["offs"], d["lens"], d["rates"])
        m.batch_run_host(d["pcm"])
        y = m.debug_read(8)
        off, ln, total = m.batch_resample_layout()
    finally:
        m.close()
    hoff, hln, htotal = pkg.mfcc.host_resample_layout(d["lens"], d["rates"], c["r_out"])
    assert off.tolist() == hoff.tolist() and ln.tolist() == hln.tolist() and total == htotal and y.size == total * c["ch"]
    y = y.reshape(-1, c["ch"]).copy()
    for u, (x, r) in enumerate(zip(d["utts"], d["rates"])):
        if r == c["r_out"]:                                 # a copy is held to its source and blanked: the fixture need not repeat it
            assert ln[u] == len(x) and np.array_equal(y[off[u]:off[u] + ln[u]], x.reshape(-1, c["ch"])), (u, len(x))
            y[off[u]:off[u] + ln[u]] = 0
    return y


def run_case(pkg, name):
    """The case's converted samples, int16 [samples][channels]."""
    c = CASES[name]
    y = {"batch": _run_batch, "session": _run_session, "mixed": _run_mixed}[c["kind"]](pkg, c)
    return np.ascontiguousarray(y, np.int16)
