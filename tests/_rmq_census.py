"""A plain model of mg_lchain_rmq as the device runs it (k_rmq_sort, k_rmq_dp of mappy-rs_amd/csrc/mm355_rmq.hip, and rmq_pass /
mm355_run_rmq of mm355_pipeline.hip around them) and a census of where its inputs go: for every anchor of a read the kernel chains to
the end, which branches of rmq_dp_read it takes -- the pieces of the range-minimum window (HBM prefix, ragged ends, block summaries and
what each summary answers), where the winner is read from, which form of the inner walk runs and where it breaks -- and per read what
makes the kernel hand it to the host.

Plain Python / numpy over the oracle (orc.anchors, orc.chains, orc._lchain_rmq for the inputs of a pass, orc.rmq_fill to be compared
with); the product is not imported.  fill() restates the fill loop of oracle/mmo_lchain.c::lchain_rmq_fill without the AVL trees: a
tree is observable only through the set it holds and through WHICH element a range-minimum query returns when two elements share the
minimal priority.  The model works on the sets and stops at the first anchor where that choice would matter (event `tie`), or where the
kernel's rings no longer hold the inner set (`inner_capacity`), or before the first anchor under a negative cap (`cap_negative`): these
are the kernel's documented reasons to flag a read MM355_RMQ_HOST.  predict() turns that into the state every read of a batch must come
back with, the chains or anchors it must hold, and its share of the four statistics rmq_pass keeps.

Its use: tests/test_rmq_census_host.py asserts on the CPU that the model's f, p, v are the oracle's and that the inputs of
tests/test_gpu_rmq_edges.py reach the branches they are there for; the GPU test holds the device to the predictions."""
import collections

import numpy as np

if __name__ == "__main__":      # run as a script (the census table, at the end): the repository root is not on the path yet
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from _chain_census import _mg_log2

WAVE = 64                      # WAVE: one step of every scan of rmq_dp_read; a block of the (y, pri) ring
RQ_RING = 512                  # RQ_RING: x, y, f, p of the last anchors
RQ_WRING = 2048                # RQ_WRING: (y, pri) of the last anchors, with RQ_NB = 32 block summaries
RQ_NB = RQ_WRING // WAVE
RQ_NEAR = RQ_RING - WAVE       # a winner j with i - j <= RQ_NEAR is read from the rings, a further one from HBM (a[], f[])
RQ_INNER = RQ_RING - 2 * WAVE  # the read is handed over when the inner set and the current run span more than this
RQ_WNEAR = RQ_WRING - WAVE     # [i - RQ_WNEAR, i0) is served by the (y, pri) ring and the summaries, what lies before by HBM (yy[], pri[])
A_STAGE = 2048                 # A_STAGE: anchors of a read that k_rmq_sort stages in LDS
RS_MIN_SIZE = 64               # MM355_RS_MIN_SIZE: radix_sort_128x is an insertion sort up to here
KEEP, DONE, HOST, HOST_ALL = 0, 1, 2, 3      # MM355_RMQ_KEEP / _DONE / _HOST / _HOST_ALL
MM_F_RMQ, MM_F_NO_LJOIN, MM_F_SPLICE, MM_F_SR = 0x80000000, 0x400, 0x080, 0x1000

f32 = np.float32

READ_KEYS = ("n_le_64", "n_not_mult_64", "n_gt_512", "n_gt_2048", "strand_change", "run_ge_2", "run_cross_64")
SORT_KEYS = ("sort_le_64", "sort_gt_64", "sort_gt_stage")
RESCUE_KEYS = ("rescue_size", "rescue_ratio_only", "rescue_no", "one_chain")
WINDOW_KEYS = ("win_empty", "win_no_block", "win_blocks", "blk_inside", "blk_cut_lo", "blk_cut_hi", "blk_outside", "blk_btie_not_min",
               "win_hbm_prefix", "winner_in_prefix", "cap_moves_st", "cap_moves_st_in")
WINNER_KEYS = ("winner_none", "winner_near", "winner_far", "winner_width_rejected", "winner_exact", "winner_eq_y_j0")
INNER_KEYS = ("inner_off", "inner_ascending", "inner_checked", "inner_sorted", "inner_gt_64", "break_first_batch", "break_later_batch",
              "skip_carried", "break_lane_0", "break_lane_63", "walk_improves")
EVENT_KEYS = ("tie_lane", "tie_summary", "tie_btie", "tie_hbm", "inner_capacity", "cap_negative")
ALL_KEYS = READ_KEYS + SORT_KEYS + RESCUE_KEYS + WINDOW_KEYS + WINNER_KEYS + INNER_KEYS + EVENT_KEYS
# classes counted per read (the others: per anchor of a read chained to the end)
PER_READ = READ_KEYS + SORT_KEYS + RESCUE_KEYS + EVENT_KEYS

Params = collections.namedtuple("Params", "max_dist max_dist_inner bw max_skip cap pen_gap pen_skip")


def params(mo, k, bw):
    """the arguments of mg_lchain_rmq as mm_map_frag passes them (bw: mo.bw for the primary chainer, mo.bw_long for the long join)"""
    return Params(int(mo.max_gap), int(mo.rmq_inner_dist), int(bw), int(mo.max_chain_skip), int(mo.rmq_size_cap),
                  f32(np.float64(mo.chain_gap_scale) * 0.01 * k), f32(np.float64(mo.chain_skip_scale) * 0.01 * k))


def _sc_simple(dr, dq, q, pen_gap, pen_skip):
    """comput_sc_simple on int64 arrays (dr = x_i - x_j, dq = y_i - y_j, q = q_span of j), float32 with one rounding per operation:
    (score, width, exact)"""
    dd = np.abs(dr - dq)
    dg = np.minimum(dr, dq)
    sc = np.minimum(q, dg)
    pen = (dd != 0) | (dq > q)
    lin = pen_gap * dd.astype(f32) + pen_skip * dg.astype(f32)
    log_pen = np.where(dd >= 1, _mg_log2((np.maximum(dd, 1) + 1).astype(f32)), f32(0))
    sc = sc - np.where(pen, (lin + f32(.5) * log_pen).astype(np.int64), 0)
    return sc, dd, (dd == 0) & (dg <= q)


def fill(a, pr, census=None):
    """mg_lchain_rmq's fill loop on the anchors a [n, 2] (uint64, sorted by x) under Params pr.  Returns dict(event, at, f, p, v,
    scanned): event None = f, p, v are the reference's and `scanned` is the sum of i0 - st (what k_rmq_dp adds to its counter);
    otherwise the name of the first event and the anchor it happens at, and f, p, v hold only what lies before it.  census: a Counter
    that takes the per-anchor classes (they are meaningful only when no event ends the pass) and the event."""
    n = len(a)
    C = collections.Counter() if census is None else census
    X, Y = np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])
    max_dist, mdi, bw, max_skip, cap = pr.max_dist, pr.max_dist_inner, pr.bw, pr.max_skip, pr.cap
    if max_dist < bw:
        max_dist = bw
    mdi = min(max(mdi, 0), max_dist)
    f = np.zeros(n, np.int64)
    p = np.full(n, -1, np.int64)
    v = np.zeros(n, np.int64)
    out = dict(event=None, at=-1, f=f, p=p, v=v, scanned=0)
    if cap < 0:
        C["cap_negative"] += 1
        out.update(event="cap_negative", at=0)
        return out
    hi = X >> np.uint64(32)
    xlo = (X & np.uint64(0xffffffff)).astype(np.int64)
    x32 = (X & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32).astype(np.int64)
    y32 = (Y & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32).astype(np.int64)
    qs = ((Y >> np.uint64(32)) & np.uint64(0xff)).astype(np.int64)
    # lb(i): the first anchor of i's strand | contig whose x lies within dist of x_i -- where the reference's `while (st < i && ...) ++st` stops
    lb = lambda dist: np.searchsorted(X, (hi << np.uint64(32)) | np.maximum(xlo - dist, 0).astype(np.uint64), "left")
    lb_out, lb_in = lb(max_dist).tolist(), lb(mdi).tolist()
    run_start = np.flatnonzero(np.append(True, X[1:] != X[:-1]))
    i0_of = np.repeat(run_start, np.diff(np.append(run_start, n))).tolist()      # the start of i's run of equal x
    badc = np.cumsum(np.append(False, y32[1:] < y32[:-1]))                        # rbad: descents of y in index order up to k
    pri = np.zeros(n, np.float64)
    half_gap = 0.5 * float(pr.pen_gap)                                           # 0.5 * chn_pen_gap in double
    xy = (x32 + y32).astype(np.float64)
    nb = (n + WAVE - 1) // WAVE
    ypad = np.full(nb * WAVE, 0, np.int64); ypad[:n] = y32
    bmin, bmax = ypad.reshape(nb, WAVE).min(1), ypad.reshape(nb, WAVE).max(1)     # of complete blocks only (the last one is never asked)
    bpri = np.zeros(nb, np.float64)
    btie = np.zeros(nb, bool)
    t = [0] * n
    pl = [-1] * n
    yl, ql = y32.tolist(), qs.tolist()
    st = st_in = 0
    scanned = 0
    L = collections.Counter()

    def stop(event, i):
        C[event] += 1
        out.update(event=event, at=i)
        return out

    for i in range(n):
        if i and (i & (WAVE - 1)) == 0:      # the block that has just been finished gets its summary
            b = (i >> 6) - 1
            w = pri[i - WAVE:i]
            bpri[b] = w.min()
            btie[b] = int((w == bpri[b]).sum()) > 1
        i0 = i0_of[i]
        yi = yl[i]
        if lb_out[i] > st:
            st = lb_out[i]
        if st < i0 and i0 - st > cap:
            st = i0 - cap
            L["cap_moves_st"] += 1
        if mdi > 0:
            if lb_in[i] > st_in:
                st_in = lb_in[i]
            if st_in < i0 and i0 - st_in > cap:
                st_in = i0 - cap
                L["cap_moves_st_in"] += 1
            if st_in < i0 and i - st_in > RQ_INNER:
                return stop("inner_capacity", i)
        # ---- the outer set and its minimum
        lo_y = yi - max_dist
        near0 = max(i - RQ_WNEAR, st)
        if st >= i0:
            L["win_empty"] += 1
        else:
            if st < near0:
                L["win_hbm_prefix"] += 1
            fb0, fb1 = (near0 + WAVE - 1) >> 6, i0 >> 6
            if near0 < i0:
                L["win_blocks" if fb0 < fb1 else "win_no_block"] += 1
        scanned += i0 - st
        max_f, max_j = ql[i], -1
        j = -1
        if st < i0:
            yw = y32[st:i0]
            m = (yw > lo_y) & (yw < yi)
            if st == 0 and yw[0] == yi:
                m[0] = True
            idx = np.flatnonzero(m)
            inside = None
            if near0 < i0 and fb0 < fb1:
                bn, bx = bmin[fb0:fb1], bmax[fb0:fb1]
                inside = (bn > lo_y) & (bx < yi)
                outside = (bx <= lo_y) | (bn > yi) | ((bn == yi) & (np.arange(fb0, fb1) != 0))
                cut = ~inside & ~outside
                L["blk_inside"] += int(inside.sum())
                L["blk_outside"] += int(outside.sum())
                L["blk_cut_lo"] += int((cut & (bn <= lo_y)).sum())
                L["blk_cut_hi"] += int((cut & (bx >= yi)).sum())
            if len(idx):
                pw = pri[st:i0][idx]
                k = int(np.argmin(pw))
                best = pw[k]
                if inside is not None:
                    L["blk_btie_not_min"] += int((inside & btie[fb0:fb1] & (bpri[fb0:fb1] > best)).sum())
                if int((pw == best).sum()) > 1:
                    # where the kernel meets the equal priorities: in the HBM prefix, through a block summary, or lane by lane
                    js = st + idx[pw == best]
                    summed = [jj >> 6 for jj in js.tolist() if inside is not None and fb0 <= (jj >> 6) < fb1 and inside[(jj >> 6) - fb0]]
                    if js[0] >= near0 and len(summed) > len(set(summed)):
                        C["tie_btie"] += 1                                  # both inside one block: only the summary's "attained twice" flag tells
                    return stop("tie_hbm" if js[0] < near0 else "tie_summary" if summed else "tie_lane", i)
                j = st + int(idx[k])
        if j < 0:
            L["winner_none"] += 1
        else:
            L["winner_near" if i - j <= RQ_NEAR else "winner_far"] += 1
            L["winner_in_prefix"] += j < near0
            L["winner_eq_y_j0"] += yl[j] == yi
            sc, width, exact = _sc_simple(x32[i:i + 1] - x32[j:j + 1], yi - y32[j:j + 1], qs[j:j + 1], pr.pen_gap, pr.pen_skip)
            sc, width, exact = int(sc[0]) + int(f[j]), int(width[0]), bool(exact[0])
            if width <= bw and sc > max_f:
                max_f, max_j = sc, j
            L["winner_width_rejected"] += width > bw
            L["winner_exact"] += exact
            L["inner_off"] += (not exact) and mdi == 0
            if not exact and mdi > 0 and st_in < i0 and yi > 0:
                yw = y32[st_in:i0]
                cand = st_in + np.flatnonzero((yw >= yi - mdi) & (yw < yi))
                yc = y32[cand]
                ascending = badc[i0 - 1] == badc[st_in]
                in_order = ascending or len(cand) < 2 or bool((yc[1:] >= yc[:-1]).all())
                L["inner_ascending" if ascending else "inner_checked" if in_order else "inner_sorted"] += 1
                L["inner_gt_64"] += len(cand) > WAVE
                if not in_order:
                    cand = cand[np.lexsort((cand, yc))]
                cand = cand[::-1]                                           # descending (y, j): the order of the reference's iterator
                if len(cand):
                    sc2, w2, _ = _sc_simple(x32[i] - x32[cand], yi - y32[cand], qs[cand], pr.pen_gap, pr.pen_skip)
                    ok = np.flatnonzero(w2 <= bw)
                    # the kernel's batches of 64: by index below i0 in the walk over j, by rank in the sorted redo
                    pos = (i0 - 1 - cand[ok]) if in_order else ok
                    tot, jl, pos = (sc2[ok] + f[cand[ok]]).tolist(), cand[ok].tolist(), pos.tolist()
                    n_skip, f_before, cur_b = 0, max_f, 0
                    for kk in range(len(jl)):
                        j2 = jl[kk]
                        if pos[kk] >> 6 != cur_b:
                            L["skip_carried"] += n_skip > 0
                            cur_b = pos[kk] >> 6
                        if tot[kk] > max_f:
                            max_f, max_j = tot[kk], j2
                            if n_skip > 0:
                                n_skip -= 1
                        elif t[j2] == i:
                            n_skip += 1
                            if n_skip > max_skip:
                                L["break_first_batch" if cur_b == 0 else "break_later_batch"] += 1
                                L["break_lane_0"] += (pos[kk] & (WAVE - 1)) == 0
                                L["break_lane_63"] += (pos[kk] & (WAVE - 1)) == WAVE - 1
                                break
                        if pl[j2] >= 0:
                            t[pl[j2]] = i
                    L["walk_improves"] += max_f > f_before
        f[i] = max_f; p[i] = max_j; pl[i] = max_j
        v[i] = v[max_j] if max_j >= 0 and v[max_j] > max_f else max_f
        pri[i] = -(float(max_f) + half_gap * xy[i])
    out["scanned"] = scanned
    C.update(L)
    return out


def read_census(a, C):
    """the classes of one read that rmq_dp_read chains (READ_KEYS)"""
    n = len(a)
    X = a[:, 0]
    C["n_le_64"] += n <= WAVE
    C["n_not_mult_64"] += n % WAVE != 0
    C["n_gt_512"] += n > RQ_RING
    C["n_gt_2048"] += n > RQ_WRING
    C["strand_change"] += bool(((X[1:] >> np.uint64(32)) != (X[:-1] >> np.uint64(32))).any())
    b = np.flatnonzero(np.append(True, X[1:] != X[:-1]))
    e = np.append(b[1:], n)
    C["run_ge_2"] += bool((e - b >= 2).any())
    C["run_cross_64"] += bool(((e - 1) // WAVE != b // WAVE).any())


def rescue(u, a, qlen, mo):
    """the rescue test of mm_map_frag on the chains (u, a): None = no more than one chain, else (fires, by rescue_size)"""
    if len(u) <= 1:
        return None
    i32 = lambda x: int(np.int32(x & np.uint64(0xffffffff)))
    st, en = i32(a[0, 1]), i32(a[int(u[0] & np.uint64(0xffffffff)) - 1, 1])
    by_size = qlen - (en - st) > mo.rmq_rescue_size
    return bool(by_size or f32(en - st) > f32(qlen) * f32(mo.rmq_rescue_ratio)), bool(by_size)


def radix_sorted(a):
    from oracle import oracle as O
    srt = np.ascontiguousarray(a, dtype=np.uint64).copy()
    O.lib().mmo_radix_sort_128x(srt.ctypes.data, srt.ctypes.data + srt.shape[0] * 16)
    return srt


def predict(orc, read, mo=None, anchors=None):
    """what the device must report for one read under MapOpt mo (default: the oracle's own, which the oracle's chainers read anyway):
    dict(state, u, a, sorted_only, stats, census, passes).  u, a: the chains the read must come back with (KEEP / DONE), or, for HOST /
    HOST_ALL, empty u and the anchors the handed-over pass started from (sorted_only: compare them as a multiset sorted by x).  stats:
    the read's share of n_rmq_reads, n_rmq_host, n_v_rmq and rmq_scanned as rmq_pass counts them.  passes: [(kind, anchors, bw,
    fill result)] of every pass the model ran, for the comparison with orc.rmq_fill"""
    mo = orc.mo if mo is None else mo
    a0 = orc.anchors(read, sorted_=True)[0] if anchors is None else anchors
    qlen = len(read)
    primary = bool(mo.flag & MM_F_RMQ)
    ljoin = mo.bw_long > mo.bw and (mo.flag & (MM_F_SPLICE | MM_F_SR | MM_F_NO_LJOIN)) == 0
    S = collections.Counter(n_rmq_reads=0, n_rmq_host=0, n_v_rmq=0, rmq_scanned=0)
    C = collections.Counter({k: 0 for k in ALL_KEYS})
    passes = []
    res = dict(state=KEEP, stats=S, census=C, passes=passes, sorted_only=False)
    empty_u = np.zeros(0, np.uint64)

    def one_pass(kind, a, bw):
        c = collections.Counter()
        r = fill(a, params(mo, orc.k, bw), c)
        passes.append((kind, a, bw, r))
        if r["event"] is None:
            read_census(a, c)
            S["n_rmq_reads"] += 1
            S["rmq_scanned"] += r["scanned"]
            C.update(c)
        else:
            S["n_rmq_host"] += 1
            C[r["event"]] += 1
            C["tie_btie"] += c["tie_btie"]
        return r["event"] is None

    if primary:
        if len(a0) == 0:
            res.update(u=empty_u, a=a0)
            return res
        S["n_v_rmq"] += len(a0)
        if not one_pass("primary", a0, mo.bw):
            res.update(state=HOST_ALL, u=empty_u, a=a0, sorted_only=True)
            return res
        u, a = orc._lchain_rmq(a0, mo.bw)
    else:
        u, a = orc.chains(a0, qlen)
    res.update(u=u, a=a)
    if not ljoin:
        return res
    go = rescue(u, a, qlen, mo)
    if go is None:
        C["one_chain"] += 1
        return res
    S["n_v_rmq"] += len(a)
    C["rescue_size" if go[1] else "rescue_ratio_only" if go[0] else "rescue_no"] += 1
    if not go[0]:
        return res
    C["sort_le_64" if len(a) <= RS_MIN_SIZE else "sort_gt_64"] += 1
    C["sort_gt_stage"] += len(a) > A_STAGE
    srt = radix_sorted(a)
    if not one_pass("ljoin", srt, mo.bw_long):
        res.update(state=HOST, u=empty_u, a=srt, sorted_only=True)
        return res
    u, a = orc._lchain_rmq(srt, mo.bw_long)
    res.update(state=DONE, u=u, a=a)
    return res


def table(rows):
    """a markdown table of census counters: rows = [(label, Counter)]"""
    out = ["| class | " + " | ".join(label for label, _ in rows) + " |", "|---|" + "---|" * len(rows)]
    for key in ("reads", "anchors") + ALL_KEYS:
        out.append("| %s | " % key + " | ".join(str(int(c[key])) for _, c in rows) + " |")
    return "\n".join(out)


if __name__ == "__main__":      # python tests/_rmq_census.py: the census of the inputs of tests/test_gpu_rmq_edges.py
    import _rmq_worlds as W
    rows = []
    for world, opts in W.TABLE:
        tot = collections.Counter()
        for pd in W.predictions(world, opts):
            tot.update(pd["census"])
            tot["reads"] += 1
            tot["anchors"] += sum(len(a) for _, a, _, r in pd["passes"] if r["event"] is None)
        rows.append((world + " " + opts, tot))
    print(table(rows))
