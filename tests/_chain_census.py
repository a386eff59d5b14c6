"""A plain model of the chain fill (k_chain_segments, k_chain_small, k_chain_big of mappy-rs_amd/csrc/mm355_kernels.hip) and a census of
where its inputs go: which segment classes k_chain_segments meets, and for every anchor of a long segment which branches of
chain_big_segment it takes (ring or HBM reads, the max_iter clamp, the 64-anchor jump of st, the break and the n_skip carried from one
64-lane batch to the next, the max_ii rescan and rescue), and what the 8192-slot ring of t[] marks answers.

Plain Python / numpy over the oracle (orc.anchors for the sorted anchors, orc.chain_fill to be compared with); the product is not
imported.  fill() restates lchain.c::mg_lchain_dp's fill loop with comput_sc and mg_log2's bit trick in float32, one rounding per
operation.  It walks the window of an anchor in the kernel's batches of 64 (j = i-1 .. i-64, then the next 64, ...): the scores of a batch
are worked out with numpy, and only the j that comput_sc accepts are walked in Python, in the sequential order of the reference.  With
`ring=None` the t[] marks are the literal array (f, p, v and t then equal orc.chain_fill); with a Ring they are the kernel's circular
table of (anchor index mod 2^tag_bits) marks, and every answer of the table is compared with the literal array kept beside it.

Its use: tests/test_chain_census_host.py asserts, on the CPU, that the inputs of tests/test_gpu_chain_edges.py reach the branches they are
there for, so that the GPU tests cannot quietly stop reaching them."""
import collections

import numpy as np

if __name__ == "__main__":      # run as a script (the census table, at the end): the repository root is not on the path yet
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHAIN_SMALL = 32               # CHAIN_SMALL: segments of up to this many anchors go to one lane of k_chain_small
WAVE = 64                      # WAVE: a strip of k_chain_segments, a batch of chain_big_segment's scan
CH_NEAR = 128                  # CH_NEAR = CH_RING - 2 * WAVE: j is read from the LDS rings when i - j <= CH_NEAR
CH_XNEAR = 896                 # CH_XNEAR = CH_XRING - 2 * WAVE: the same for the ring of reference coordinates
SEG_STEP = 512                 # one look-ahead step of k_chain_segments (eight loads of WAVE anchors)
SEG_CHUNK = 4096               # SEG_CHUNK: anchors per block of k_chain_segments
TW_SIZE = 8192                 # TW_SIZE: slots of the mark ring tw[]
TW_TAG_BITS = 15               # the mark is (i & 0x7fff) | 0x8000
TW_TAG_SPAN = 32768            # 1 << TW_TAG_BITS: anchors after which a mark value comes round again
MAX_CHAIN_ITER = 8000          # the stage refuses a max_chain_iter above this (the window must fit the mark ring)

f32 = np.float32
# clear: the table is cleared again whenever (i & tag mask) == 0.  batch_writes: every lane of a 64-lane batch writes its mark before any lane
# reads one, the lanes behind a break included (what the wave does); False = the marks are written one by one as the sequential scan
# goes, and none behind a break (the order of the reference loop)
Ring = collections.namedtuple("Ring", "slots tag_bits clear batch_writes")
KERNEL_RING = Ring(TW_SIZE, TW_TAG_BITS, False, True)        # tw[] as it was: cleared once per segment
CLEARED_RING = Ring(TW_SIZE, TW_TAG_BITS, True, True)        # cleared again whenever (i & 0x7fff) == 0
WIDE_RING = Ring(TW_SIZE, 31, False, True)                   # the alternative: a tag as wide as the anchor index
SEQUENTIAL_RING = Ring(TW_SIZE, TW_TAG_BITS, False, False)   # the 15-bit table written in the reference loop's order


def max_dist(mo, qlen):
    """(max_dist_x, max_dist_y) of mg_lchain_dp as mm_map_frag calls it, after the `< bw` lift (chain_dist of the kernels)"""
    mdx = mo.max_gap_ref if mo.max_gap_ref > 0 else (max(mo.max_frag_len - qlen, mo.max_gap) if mo.max_frag_len > 0 else mo.max_gap)
    return max(mdx, mo.bw), max(mo.max_gap, mo.bw)


def segment_starts(x, mdx):
    """the rule of k_chain_segments: an anchor starts a segment when its strand | contig differs from its left neighbour's or its
    reference position lies more than max_dist_x (after the bw lift) beyond it.  x: the sorted a[].x; returns a bool array"""
    start = np.ones(len(x), bool)
    start[1:] = ((x[1:] >> np.uint64(32)) != (x[:-1] >> np.uint64(32))) | (x[1:] > x[:-1] + np.uint64(mdx))
    return start


def segment_census(x, mdx):
    """counts of the segment classes of one read (see SEGMENT_KEYS) and the (begin, end) of every segment"""
    n = len(x)
    c = collections.Counter()
    if n == 0:
        return c, np.zeros((0, 2), np.int64)
    b = np.flatnonzero(segment_starts(x, mdx))
    e = np.append(b[1:], n)
    ln = e - b
    c["seg_1"] = int((ln == 1).sum())
    c["seg_2_31"] = int(((ln >= 2) & (ln < CHAIN_SMALL)).sum())
    c["seg_32"] = int((ln == CHAIN_SMALL).sum())
    c["seg_33"] = int((ln == CHAIN_SMALL + 1).sum())
    c["seg_longer"] = int((ln > CHAIN_SMALL + 1).sum())
    c["start_lane_63"] = int(((b & (WAVE - 1)) == WAVE - 1).sum())
    strip = b // WAVE
    last = np.append(strip[1:] != strip[:-1], True)                  # the last start of its strip: the wave looks ahead for its end
    nxt = (strip + 1) * WAVE                                         # where the look-ahead begins
    c["last_end_same_strip"] = int((last & (e < nxt)).sum())         # (only the read's last segment: its end is n)
    c["last_end_next_64"] = int((last & (e >= nxt) & (e < nxt + WAVE) & (e < n)).sum())
    c["last_end_beyond_512"] = int((last & (e >= nxt + SEG_STEP)).sum())
    c["last_end_beyond_chunk"] = int((last & (e > (b // SEG_CHUNK + 1) * SEG_CHUNK)).sum())
    c["last_end_read_end"] = int((last & (e == n) & (e >= nxt)).sum())   # the look-ahead runs off the read
    c["read_multi_chunk"] = int(n > SEG_CHUNK)
    return c, np.stack([b, e], 1)


SEGMENT_KEYS = ("seg_1", "seg_2_31", "seg_32", "seg_33", "seg_longer", "start_lane_63", "last_end_next_64", "last_end_beyond_512",
                "last_end_beyond_chunk", "last_end_read_end", "read_multi_chunk")
WINDOW_KEYS = ("win_le_128", "win_129_896", "win_gt_896", "st_jump_64", "iter_clamp")
SCAN_KEYS = ("batches_1", "batches_2", "batches_3up", "break_first_batch", "break_later_batch", "break_lane_0", "break_lane_63",
             "skip_carried", "reflect", "tie_in_batch", "far_batch")
MAXII_KEYS = ("rescan", "rescan_tie", "rescue_wins", "maxii_gt_128", "maxii_gt_896", "v_far")
RING_KEYS = ("idx_ge_32768",)
ALL_KEYS = SEGMENT_KEYS + WINDOW_KEYS + SCAN_KEYS + MAXII_KEYS + RING_KEYS


def _mg_log2(x):
    """mmpriv.h::mg_log2 on a float32 array (x >= 2), every operation rounded to float32"""
    z = x.view(np.uint32)
    log_2 = (((z >> np.uint32(23)) & np.uint32(255)).astype(np.int64) - 128).astype(f32)
    z = (z & np.uint32(~(255 << 23) & 0xffffffff)) + np.uint32(127 << 23)
    zf = z.view(f32)
    return log_2 + (((f32(-0.34484843) * zf + f32(2.02466578)) * zf) - f32(0.67487759))


def fill(a, qlen, mo, k, ring=None, census=None):
    """mg_lchain_dp's fill loop on the sorted anchors a [n, 2] (uint64) of one read of qlen bases under MapOpt mo at k-mer length k.
    ring: None = the literal t[]; a Ring = the marks of the long segments come from the circular table (short segments keep the
    literal marks: k_chain_small has full-width ones).  census: a Counter that takes the counts of WINDOW / SCAN / MAXII / RING_KEYS
    over the anchors of long segments.  Returns dict(f, p, v, t, false_marks): t is the literal array either way, false_marks the
    number of answers of the table that differ from it (at the j where the answer is used)."""
    n = len(a)
    X, Y = np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])
    assert not ((Y >> np.uint64(48)) & np.uint64(0xff)).any()          # one segment per read: sidi == sidj throughout
    mdx, mdy = max_dist(mo, qlen)
    bw, max_skip, max_iter = int(mo.bw), int(mo.max_chain_skip), int(mo.max_chain_iter)
    pen_gap = f32(np.float64(mo.chain_gap_scale) * 0.01 * k)
    pen_skip = f32(np.float64(mo.chain_skip_scale) * 0.01 * k)
    half = f32(.5)
    xlo = (X & np.uint64(0xffffffff)).astype(np.int64)                # (int32_t)(ai->x - aj->x) inside one strand | contig
    yq = (Y & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32).astype(np.int64)
    qs = ((Y >> np.uint64(32)) & np.uint64(0xff)).astype(np.int64)
    Xl, hi, span = X.tolist(), (X >> np.uint64(32)).tolist(), qs.tolist()
    _, segs = segment_census(X, mdx)
    seg_begin = np.zeros(n, np.int64)
    is_long = np.zeros(n, bool)
    for b, e in segs.tolist():
        seg_begin[b:e] = b
        is_long[b:e] = e - b > CHAIN_SMALL
    seg_begin, is_long = seg_begin.tolist(), is_long.tolist()
    f = np.zeros(n, np.int64)
    p = np.full(n, -1, np.int64)
    pl, t, v = [-1] * n, [0] * n, [0] * n
    if ring is not None:
        tw = [0] * ring.slots
        smask, tmask = ring.slots - 1, (1 << ring.tag_bits) - 1
    false_marks = 0
    C = census
    st, max_ii = 0, -1
    for i in range(n):
        xi, hi_i = Xl[i], hi[i]
        big = is_long[i]
        use_ring = ring is not None and big
        batch_writes = use_ring and ring.batch_writes
        st0 = st
        while st < i and (hi_i != hi[st] or xi > Xl[st] + mdx):
            st += 1
        st1 = st
        if i - st > max_iter:
            st = i - max_iter
        if use_ring:
            if i == seg_begin[i] or (ring.clear and (i & tmask) == 0):
                tw = [0] * ring.slots
            tag = (i & tmask) | (1 << ring.tag_bits)
        max_f, max_j, n_skip = span[i], -1, 0
        end_j = st - 1
        yi, xli = int(yq[i]), int(xlo[i])
        n_batches = (i - st + WAVE - 1) // WAVE                       # batch b holds j = i - 1 - 64 b .. i - 64 (b + 1)
        cur_b = brk_lane = brk_batch = -1
        ev_carry = ev_reflect = ev_tie = broke = False
        f_before, marked_seen, btots = max_f, False, []
        # the window in pieces of whole batches (128 anchors, then 1024, then the rest): most scans break inside the first
        top, step = i, 2 * WAVE
        while top > st and not broke:
            lo = max(st, top - step)
            step *= 8
            dq = yi - yq[lo:top]
            dr = xli - xlo[lo:top]
            dd = np.abs(dr - dq)
            ok = (dq > 0) & (dq <= mdx) & (dr != 0) & (dq <= mdy) & (dd <= bw)
            idx = np.flatnonzero(ok)[::-1]                             # the j that comput_sc accepts, in the order of the sequential scan
            if len(idx):
                dq, dr, dd, q = dq[idx], dr[idx], dd[idx], qs[lo:top][idx]
                dg = np.minimum(dr, dq)
                sc = np.minimum(q, dg)
                pen = (dd != 0) | (dg > q)
                lin = pen_gap * dd.astype(f32) + pen_skip * dg.astype(f32)
                log_pen = np.where(dd >= 1, _mg_log2((np.maximum(dd, 1) + 1).astype(f32)), f32(0))
                sc = sc - np.where(pen, (lin + half * log_pen).astype(np.int64), 0)
                js = idx + lo
                tot, jl = (sc + f[js]).tolist(), js.tolist()
                for kk in range(len(jl)):
                    j = jl[kk]
                    b = (i - 1 - j) >> 6
                    if b != cur_b:                                     # the first accepted j of another batch
                        if max_f > f_before and btots.count(max_f) >= 2:
                            ev_tie = True
                        if n_skip > 0:
                            ev_carry = True
                        cur_b, f_before, marked_seen, btots = b, max_f, False, []
                        if batch_writes:                               # every lane of the batch writes its mark before any lane reads one
                            k2 = kk
                            while k2 < len(jl) and (i - 1 - jl[k2]) >> 6 == b:
                                if pl[jl[k2]] >= st:
                                    tw[pl[jl[k2]] & smask] = tag
                                k2 += 1
                    s = tot[kk]
                    btots.append(s)
                    if s > max_f:
                        max_f, max_j = s, j
                        if n_skip > 0:
                            n_skip -= 1
                        elif marked_seen:
                            ev_reflect = True                          # the walk is reflected at 0 after it had been above it in this batch
                    else:
                        m = t[j] == i
                        if use_ring:
                            rm = tw[j & smask] == tag
                            if rm != m:
                                false_marks += 1
                                m = rm
                        if m:
                            marked_seen = True
                            n_skip += 1
                            if n_skip > max_skip:
                                broke, brk_lane, brk_batch, end_j = True, (i - 1 - j) & (WAVE - 1), b, j
                                break
                    if pl[j] >= 0:
                        t[pl[j]] = i
                        if use_ring and not batch_writes and pl[j] >= st:
                            tw[pl[j] & smask] = tag
            top = lo
        if max_f > f_before and btots.count(max_f) >= 2:
            ev_tie = True
        if not broke and n_skip > 0 and cur_b < n_batches - 1:
            ev_carry = True                                            # into batches in which comput_sc accepts nothing
        nb = brk_batch + 1 if broke else n_batches
        # max_ii
        rescan = max_ii < 0 or ((xi - Xl[max_ii]) & 0xffffffffffffffff) > mdx
        rescan_tie = False
        if rescan:
            max_ii = -1
            if i > st:
                w = f[st:i][::-1]
                r = int(np.argmax(w))                                  # the first of the largest from the top: ties go to the larger j
                max_ii = i - 1 - r
                rescan_tie = int((w == w[r]).sum()) >= 2
        maxii_dist = i - max_ii if max_ii >= 0 else 0
        rescue = False
        if max_ii >= 0 and max_ii < end_j:
            assert hi[max_ii] == hi_i
            dq, dr = yi - int(yq[max_ii]), xli - int(xlo[max_ii])
            dd = abs(dr - dq)
            if 0 < dq <= mdx and dr != 0 and dq <= mdy and dd <= bw:
                dg, q = min(dr, dq), span[max_ii]
                tmp = min(q, dg)
                if dd or dg > q:
                    lin = pen_gap * f32(dd) + pen_skip * f32(dg)
                    log_pen = _mg_log2(np.array([dd + 1], f32))[0] if dd >= 1 else f32(0)
                    tmp -= int(lin + half * log_pen)
                if max_f < tmp + int(f[max_ii]):
                    max_f, max_j, rescue = tmp + int(f[max_ii]), max_ii, True
        f[i] = max_f; p[i] = max_j; pl[i] = max_j
        v[i] = v[max_j] if max_j >= 0 and v[max_j] > max_f else max_f
        if max_ii < 0 or (((xi - Xl[max_ii]) & 0xffffffffffffffff) <= mdx and f[max_ii] < max_f):
            max_ii = i
        if C is not None and big:
            win = i - st
            C["win_le_128" if win <= CH_NEAR else "win_129_896" if win <= CH_XNEAR else "win_gt_896"] += 1
            C["st_jump_64"] += st1 - st0 >= WAVE and st0 >= seg_begin[i]
            C["iter_clamp"] += i - st1 > max_iter
            if nb:
                C["batches_1" if nb == 1 else "batches_2" if nb == 2 else "batches_3up"] += 1
            C["far_batch"] += nb >= 3                                   # the third batch is the first whose j lie beyond CH_NEAR
            if brk_lane >= 0:
                C["break_first_batch" if brk_batch == 0 else "break_later_batch"] += 1
                C["break_lane_0"] += brk_lane == 0
                C["break_lane_63"] += brk_lane == WAVE - 1
            C["skip_carried"] += ev_carry
            C["reflect"] += ev_reflect
            C["tie_in_batch"] += ev_tie
            C["rescan"] += rescan and i > st
            C["rescan_tie"] += rescan_tie
            C["rescue_wins"] += rescue
            C["maxii_gt_128"] += maxii_dist > CH_NEAR
            C["maxii_gt_896"] += maxii_dist > CH_XNEAR
            C["v_far"] += max_j >= 0 and i - max_j > CH_NEAR
            C["idx_ge_32768"] += i - seg_begin[i] >= TW_TAG_SPAN
    return dict(f=f.astype(np.int32), p=p, v=np.array(v, np.int32), t=np.array(t, np.int32), false_marks=false_marks)


def census(orc, read, mo=None):
    """(counts, anchors, literal fill) of one read under MapOpt `mo` (default: the oracle's own)"""
    mo = orc.mo if mo is None else mo
    a = orc.anchors(read, sorted_=True)[0]
    c = collections.Counter({k: 0 for k in ALL_KEYS})
    c.update(segment_census(a[:, 0], max_dist(mo, len(read))[0])[0])
    r = fill(a, len(read), mo, orc.k, census=c)
    c["anchors"] = len(a)
    return c, a, r


def ring_census(a, qlen, mo, k, ring, literal):
    """what the ring changes on one read: (answers of the table that differ from the literal t[], anchors whose f or p differ from the
    literal fill's)"""
    r = fill(a, qlen, mo, k, ring=ring)
    return r["false_marks"], int(((r["f"] != literal["f"]) | (r["p"] != literal["p"])).sum())


def table(rows):
    """a markdown table of census counters: rows = [(label, Counter)]"""
    out = ["| class | " + " | ".join(label for label, _ in rows) + " |", "|---|" + "---|" * len(rows)]
    for key in ("anchors",) + ALL_KEYS:
        out.append("| %s | " % key + " | ".join(str(int(c[key])) for _, c in rows) + " |")
    return "\n".join(out)


if __name__ == "__main__":      # python tests/_chain_census.py: the census of the inputs of tests/test_gpu_chain_edges.py
    from oracle import oracle as O  # noqa: F401
    import _chain_worlds as W
    rows = []
    for world, opts in (("stages", "default"), ("stages", "iter_40"), ("stages", "skip_60"), ("arrays", "default"), ("arrays", "iter_8000"),
                        ("arrays", "skip_1"), ("mosaic", "skip_1")):
        wd = W.mosaic_world() if world == "mosaic" else W.WORLDS[world]()
        orc = W.oracle_for(wd, W.MOSAIC_SETS[opts] if world == "mosaic" else W.OPTION_SETS[opts])
        tot = collections.Counter()
        for rd in wd["reads"].values():
            tot.update(census(orc, rd)[0])
        rows.append((world + " " + opts, tot))
    print(table(rows))
