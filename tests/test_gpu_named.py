"""Query names on the GPU (mm355_map_batch_named / mm355_batch_upload_named / mm355_stage_anchors_named, Aligner.map(name=...),
Aligner(name_key=...)): skip_seed's NO_DIAG / NO_DUAL branch in k_seed_select_named / k_seed_expand_named, MM_SEED_SELF, the name in the
read hash on every region route, and the unnamed path unchanged byte for byte.  Truth: tests/_named_truth.py (proved on the CPU by
tests/test_named_host.py)."""
import ctypes as C
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import _named_truth as T
import _capi
from _capi import pair, stats

OUT_CS, OUT_TAGS = 1, 4


def map_named(al, reads, names, flags=OUT_TAGS, entry="named"):
    """(per read: list of (row tuple, cigar bytes, cs bytes or None, tags tuple or None)), (raw hit rows, CIGAR words, string arena).
    entry: named (mm355_map_batch_named), batch (mm355_map_batch when names is None), resident (mm355_batch_upload_named +
    mm355_map_resident), nullarr (named entry, an array of NULL pointers)"""
    assert names is None or entry in ("named", "resident")
    v = _capi.map_raw(al, reads, flags, names, entry)
    rows, tg, cb, sb = v.hits, v.tags, v.cigar.tobytes(), v.str
    out = []
    for i in range(len(reads)):
        one = []
        for j in range(v.off[i], v.off[i + 1]):
            r = rows[j]
            tt = None
            if tg is not None:
                t = tg[j]; fl = int(t["flags"])
                tt = (int(t["score"]), T.f32_bits(t["div"]), int(t["rep_len"]), int(t["n_ambi"]), int(t["n_gap"]), int(t["n_gapo"]),
                      fl & 1, fl >> 1 & 1, fl >> 2 & 3)
            co, nc = int(r["cigar_off"]), int(r["n_cigar"])
            cs = sb[int(r["cs_off"]):int(r["cs_off"]) + int(r["cs_len"])] if int(r["cs_len"]) >= 0 else None
            one.append((tuple(int(r[k]) for k in T.ROW_FIELDS), cb[co * 4:(co + nc) * 4], cs, tt))
        out.append(one)
    return out, (_capi.raw(v.hits), cb, sb)


def want_rows(dicts, tags=True):
    return [(T.row_tuple(d), d["cigar"], d["cs"], T.tag_tuple(d) if tags else None) for d in dicts]


@pytest.fixture(scope="module")
def W(built):
    return T.overlap_world()


@pytest.fixture(scope="module")
def D(built):
    return T.dup_world()


# ------------------------------------------------------------------ 1. the seed kernels, anchor by anchor
@pytest.mark.parametrize("preset,xf", [("ava-ont", 0), ("map-ont", 1), ("map-ont", 2), ("map-ont", 3), ("map-ont", 3 | T.FOR_ONLY)],
                         ids=["ava-ont", "no_diag", "no_dual", "both", "both+for_only"])
def test_stage_anchors_named(W, preset, xf):
    al, orc = pair(W["fa"], preset, False, **({"extra_flags": xf} if xf else {}))
    names = [nm for nm, _ in W["queries"]]; seqs = [s for _, s in W["queries"]]
    sr = al._stage_runner()
    got, rep, nmp = sr.anchors(seqs, sorted_=False, names=names)
    n_self = n_drop = 0
    for i, (nm, s) in enumerate(W["queries"]):
        a, rep_len, mini_pos, ns = T.filtered_anchors(orc, s, nm)
        assert got[i].shape == a.shape and np.array_equal(got[i], a), (preset, xf, i, nm)      # element by element, bit 43 included
        assert int(rep[i]) == rep_len and int(nmp[i]) == len(mini_pos)                            # fixed before the filter
        n_self += ns; n_drop += len(orc.anchors(s, sorted_=False)[0]) - len(a)
    assert n_drop > 3000 and (n_self > 100) == bool(al._mo.flag & T.NO_DIAG)
    if al._mo.flag & T.NO_DIAG and al._mo.flag & T.NO_DUAL:      # the read with the greatest name loses every anchor
        gi = names.index(W["targets"][W["greatest"]][0])
        assert len(orc.anchors(seqs[gi], sorted_=False)[0]) > 500 and len(got[gi]) == 0
    # sorted = 1 carries the same multiset through the sort, SELF bits included
    srt, _, _ = sr.anchors(seqs[:4] + seqs[-5:], sorted_=True, names=names[:4] + names[-5:])
    for g, i in zip(srt, list(range(4)) + list(range(len(seqs) - 5, len(seqs)))):
        key = lambda m: sorted(map(tuple, m.tolist()))
        assert key(g) == key(got[i])
    sr.close()


# ------------------------------------------------------------------ 2. the name in the read hash, on every region route
@pytest.mark.parametrize("cigar", [False, True], ids=["chain_only", "cigar"])
def test_hash_routes_duplicate_world(D, monkeypatch, cigar):
    al, orc = pair(D["fa"], "map-ont", cigar)
    reads, names = [], []
    for s in D["reads"]:
        for nm in [None] + D["names"]:
            reads.append(s); names.append(nm)
    flags = OUT_TAGS | (OUT_CS if cigar else 0)
    exp = [want_rows(T.oracle_named(orc, s, nm, with_cs=cigar)) for s, nm in zip(reads, names)]
    assert len({tuple(e) for e in exp[:5]}) > 1                       # the name decides between the two identical contigs
    got, raw = map_named(al, reads, names, flags)
    assert got == exp
    if not cigar:
        assert stats(al).n_regs_dev == len(reads)                     # k_regs
    assert map_named(al, reads, names, flags, entry="resident")[0] == exp
    # MM_F_NO_HASH_NAME: the names no longer count
    al._mo.flag |= T.NO_HASH_NAME
    assert map_named(al, reads, names, flags)[0] == [exp[i - i % 5] for i in range(len(reads))]
    al._mo.flag &= ~T.NO_HASH_NAME
    if not cigar:
        monkeypatch.setenv("MM355_REGS_LOGT_N", "1200")               # the device defers reads with larger chain scores: host route, merged
        dfr, raw_d = map_named(al, reads, names, flags)
        st = stats(al)
        assert st.n_regs_host > 0 and dfr == exp and raw_d == raw
        monkeypatch.delenv("MM355_REGS_LOGT_N")
        monkeypatch.setenv("MM355_REGS_HOST", "1")
        hst, raw_h = map_named(al, reads, names, flags)
        assert stats(al).n_regs_dev == 0 and hst == exp and raw_h == raw


# ------------------------------------------------------------------ 3. all-vs-all, chain-only
@pytest.mark.parametrize("preset,xf", [("ava-ont", 0), ("map-ont", 3)], ids=["ava-ont", "map-ont+3"])
def test_overlap_chain_only(W, preset, xf):
    al, orc = pair(W["fa"], preset, False, **({"extra_flags": xf} if xf else {}))
    names = [nm for nm, _ in W["queries"]]; seqs = [s for _, s in W["queries"]]
    tn = [nm for nm, _ in W["targets"]]
    got, _ = map_named(al, seqs, names)
    unnamed, _ = map_named(al, seqs, None, entry="batch")
    n_rows = 0
    seen = {}
    for i, (nm, s) in enumerate(W["queries"]):
        exp, _ = T.compose_named(orc, s, nm)
        assert got[i] == want_rows(exp), (preset, i, nm)
        n_rows += len(exp)
        if nm is None:
            assert got[i] == unnamed[i]
            continue
        if orc.mo.flag & T.ALL_CHAINS:    # independent check: what is left on other names is what mmo_map reports for qname < tname
            whole = T.oracle_named(orc, s, nm)
            assert [r[0] for r in got[i] if tn[r[0][0]] != nm] == [T.row_tuple(d) for d in whole if nm < tn[d["rid"]]]
        for row, _, _, _ in got[i]:
            rid, qs, qe, _, ts, te = row[:6]
            # no self hit along the diagonal (self = the contig of this name AND this length: a read that only shares a contig's name, the
            # 2500-base `rd10` query, is no copy of it and keeps its diagonal, as in U:map.c::skip_seed)
            assert not (tn[rid] == nm and len(W["targets"][rid][1]) == len(s) and qs == ts and qe == te)
            if i < len(tn) and tn.count(nm) == 1 and tn[rid] != nm:
                assert nm < tn[rid]
                seen.setdefault(frozenset((nm, tn[rid])), set()).add(nm)
    assert n_rows > 30 and len(seen) > 15 and all(len(v) == 1 for v in seen.values())  # each unordered pair from one side only
    if orc.mo.flag & T.ALL_CHAINS:
        assert 2 * sum(map(len, got)) < sum(map(len, unnamed))                         # the second report of every pair and the self hits are gone


# ------------------------------------------------------------------ 4. all-vs-all with base-level alignment
def _target_from_cs(cs, q):
    """the target bases a cs string (short form) implies for the query bases q (already on the alignment's strand)"""
    out, qi = [], 0
    for m in re.finditer(r":(\d+)|\*([acgtn])([acgtn])|\+([acgtn]+)|-([acgtn]+)", cs):
        if m.group(1):
            n = int(m.group(1)); out.append(q[qi:qi + n]); qi += n
        elif m.group(2):
            out.append(m.group(2).upper()); qi += 1
        elif m.group(4):
            qi += len(m.group(4))
        else:
            out.append(m.group(5).upper())
    return "".join(out), qi


def _revcomp(s):
    return s.translate(str.maketrans("ACGTN", "TGCAN"))[::-1]


@pytest.mark.parametrize("preset,xf", [("ava-ont", 0), ("map-ont", 3)], ids=["ava-ont", "map-ont+3"])
def test_overlap_cigar(W, preset, xf):
    al, orc = pair(W["fa"], preset, True, **({"extra_flags": xf} if xf else {}))
    names = [nm for nm, _ in W["queries"]]; seqs = [s for _, s in W["queries"]]
    tseq = [s for _, s in W["targets"]]
    got, _ = map_named(al, seqs, names, OUT_TAGS | OUT_CS)
    n_plain = n_self_reads = n_self_rows = 0
    for i, (nm, s) in enumerate(W["queries"]):
        n_self = T.filtered_anchors(orc, s, nm)[3]
        if n_self == 0:                                       # truth (b) holds: the oracle needs no clamp here
            exp, _ = T.compose_named(orc, s, nm, with_cs=True)
            assert got[i] == want_rows(exp), (preset, i, nm)
            n_plain += len(exp)
            continue
        n_self_reads += 1
        for row, cg, cs, _ in got[i]:                         # reads with SELF anchors: the records must be sound alignments
            rid, qs, qe, strand, ts, te = row[:6]
            ops = np.frombuffer(cg, dtype=np.uint32); ln, op = ops >> 4, ops & 0xf
            assert int(ln[(op == 0) | (op == 1)].sum()) == qe - qs and int(ln[(op == 0) | (op == 2)].sum()) == te - ts
            q = s[qs:qe] if strand > 0 else _revcomp(s[qs:qe])
            t, used = _target_from_cs(cs.decode(), q)
            assert used == qe - qs and t == tseq[rid][ts:te]
            assert not (W["targets"][rid][0] == nm and len(tseq[rid]) == len(s) and qs == ts and qe == te)
            n_self_rows += 1
    assert n_plain > 20 and n_self_reads >= 1 and n_self_rows >= 1


# ------------------------------------------------------------------ 5. no name: not a byte changes
@pytest.mark.parametrize("preset,cigar", [("ava-ont", False), ("map-ont", False), ("map-ont", True)], ids=["ava-chain", "ont-chain", "ont-cigar"])
def test_unnamed_is_byte_identical(W, preset, cigar):
    al, _ = pair(W["fa"], preset, cigar)
    seqs = [s for _, s in W["queries"]]
    flags = OUT_TAGS | (OUT_CS if cigar else 0)
    base, raw = map_named(al, seqs, None, flags, entry="batch")
    assert sum(map(len, base)) > 20
    for entry in ("named", "nullarr", "resident"):
        g, r = map_named(al, seqs, None, flags, entry=entry)
        assert r == raw and g == base, entry
    # a resident batch forgets the names of the batch before it
    map_named(al, seqs, [nm for nm, _ in W["queries"]], flags, entry="resident")
    g, r = map_named(al, seqs, None, flags, entry="resident")
    assert r == raw
    sr = al._stage_runner()
    a0, rep0, n0 = sr.anchors(seqs, sorted_=False)
    a1, rep1, n1 = sr.anchors(seqs, sorted_=False, names=[None] * len(seqs))
    assert all(np.array_equal(x, y) for x, y in zip(a0, a1)) and np.array_equal(rep0, rep1) and np.array_equal(n0, n1)
    sr.close()


# ------------------------------------------------------------------ 6. a read's rows do not depend on its batch
def test_batch_independence(W):
    al, _ = pair(W["fa"], "ava-ont", False)
    names = [nm for nm, _ in W["queries"]]; seqs = [s for _, s in W["queries"]]
    whole, _ = map_named(al, seqs, names)
    perm = np.random.default_rng(5).permutation(len(seqs)).tolist()
    shuf, _ = map_named(al, [seqs[j] for j in perm], [names[j] for j in perm])
    assert [shuf[perm.index(i)] for i in range(len(seqs))] == whole
    parts = []
    for a, b in ((0, 1), (1, 7), (7, 8), (8, 19), (19, len(seqs))):       # (7, 8): the unnamed read alone -- a batch without names
        parts += map_named(al, seqs[a:b], names[a:b])[0]
    assert parts == whole


# ------------------------------------------------------------------ 7. Python
def test_python_names(W):
    import mappy_rs
    al = mappy_rs.Aligner(W["fa"], preset="ava-ont", cigar=False, tags=True, name_key="id")
    orc = O.OracleAligner(W["fa"], preset="ava-ont")
    orc.mo.flag &= ~4
    tn = [nm for nm, _ in W["targets"]]
    qs = [(nm, s) for nm, s in W["queries"] if nm is None or nm.isascii() or nm == "rdé".encode()]
    key = lambda ms: [(m.ctg, m.r_st, m.r_en, m.q_st, m.q_en, m.strand, m.mapq, m.s1) for m in ms]
    want = lambda d: (tn[d["rid"]].decode(), d["target_start"], d["target_end"], d["query_start"], d["query_end"], d["strand"], d["mapq"], d["score"])
    exp = [[want(d) for d in T.compose_named(orc, s, nm)[0]] for nm, s in qs]
    for (nm, s), e in zip(qs, exp):
        assert key(al.map(s, name=None if nm is None else nm.decode())) == e          # names are encoded as UTF-8 (rdé)
    assert key(al.map(qs[0][1])) != exp[0]                                            # without the name: the self hit is there
    items = [dict(seq=s, i=i, **({} if nm is None else {"id": nm.decode()})) for i, (nm, s) in enumerate(qs)]
    items[3]["id"] = None                                                             # None = unnamed, like a missing key
    exp[3] = [want(d) for d in T.compose_named(orc, qs[3][1], None)[0]]
    al.enable_threading(2)
    for feed in (items, (it for it in items)):                                        # the C-level fast path, the element-wise loop
        res = {d["i"]: key(m) for m, d in al.map_batch(feed)}
        assert [res[i] for i in range(len(items))] == exp
    bad = [dict(it) for it in items]; bad[2]["id"] = 7
    for feed in (bad, (it for it in bad)):
        with pytest.raises(ValueError):
            al.map_batch(feed)
    al2 = mappy_rs.Aligner(W["fa"], preset="ava-ont", cigar=False, tags=True, name_key="id", devices=[0])
    al2.enable_threading(1)
    res = {d["i"]: key(m) for m, d in al2.map_batch(items)}
    assert [res[i] for i in range(len(items))] == exp
    nm, s = qs[0]
    m = al.map(s, name=nm.decode())[0]
    f = mappy_rs.paf_line(m, nm.decode(), len(s)).split("\t")
    assert f[0] == nm.decode() and f[5] == m.ctg and f[5] != f[0] and f[0] < f[5] and "tp:A:" in f[12]


# ------------------------------------------------------------------ 8. an index built on the device
def test_device_built_index(W):
    """mm355_index_build_device assembles the build device's replica itself: the named kernels must find the rank table there too"""
    from mappy_rs import _ffi
    L = _ffi.lib()
    orc = O.OracleAligner(W["fa"], preset="ava-ont")
    orc.mo.flag &= ~4
    io, mo = _ffi.IdxOpt(), _ffi.MapOpt()
    L.mm355_set_opt(None, C.byref(io), C.byref(mo))
    _ffi.check(L.mm355_set_opt(b"ava-ont", C.byref(io), C.byref(mo)))
    lut = np.full(256, 4, np.uint8); lut[list(b"ACGT")] = [0, 1, 2, 3]
    codes = [lut[np.frombuffer(s.encode(), np.uint8)] for _, s in W["targets"]]
    n = len(codes)
    ptrs = (C.c_char_p * n)(*[C.cast(c.ctypes.data, C.c_char_p) for c in codes])
    lens = (C.c_int64 * n)(*[len(c) for c in codes])
    nm = (C.c_char_p * n)(*[t for t, _ in W["targets"]])
    idx = C.c_void_p()
    _ffi.check(L.mm355_index_build_device(C.byref(io), n, ptrs, lens, nm, 0, C.byref(idx)))
    try:
        L.mm355_mapopt_update(C.byref(mo), idx)
        mo.flag &= ~4
        assert mo.mid_occ == orc.mo.mid_occ
        names = [q for q, _ in W["queries"]]; seqs = [s for _, s in W["queries"]]
        sr = _ffi.StageRunner(idx, mo, 0)
        got, rep, nmp = sr.anchors(seqs, sorted_=False, names=names)
        n_self = 0
        for i, (q, s) in enumerate(W["queries"]):
            a, rep_len, mini_pos, ns = T.filtered_anchors(orc, s, q)
            assert np.array_equal(got[i], a) and int(rep[i]) == rep_len and int(nmp[i]) == len(mini_pos), (i, q)
            n_self += ns
        assert n_self > 100
        off = _ffi.map_raw(L, sr.ctx, mo, seqs, 0, names, "named").off
        assert [int(off[i + 1] - off[i]) for i in range(len(seqs))] == [len(T.compose_named(orc, s, q)[0]) for q, s in W["queries"]]
        sr.close()
    finally:
        L.mm355_index_free(idx)


# ------------------------------------------------------------------ 9. an index without names
def test_index_without_names_hash_only(W, tmp_path):
    """MM_I_NO_NAME (index flag 4): skip_seed's name branch is inert -- the unnamed seed kernels run -- and only the hash applies, which is
    exactly what the oracle's mmo_map(qname) computes.  The .mmi is the oracle's dump of the overlap world with the flag bit set."""
    import mappy_rs
    orc = O.OracleAligner(W["fa"], preset="ava-ont")
    orc.mo.flag &= ~4
    mmi = str(tmp_path / "noname.mmi")
    O.lib().mmo_idx_dump(orc.idx, mmi.encode())
    raw = bytearray(open(mmi, "rb").read())
    assert raw[:4] == b"MMI\2"
    raw[20:24] = (int.from_bytes(raw[20:24], "little") | 4).to_bytes(4, "little")          # magic, w, k, b, n_seq, flag
    open(mmi, "wb").write(bytes(raw))
    al = mappy_rs.Aligner(mmi, preset="ava-ont", cigar=False)
    assert al._info()[3] & 4 and al._mo.flag & 3 == 3
    names = [q for q, _ in W["queries"]]; seqs = [s for _, s in W["queries"]]
    got, _ = map_named(al, seqs, names)
    assert got == [want_rows(T.oracle_named(orc, s, q)) for q, s in W["queries"]]             # nothing filtered, the name hashed
    sr = al._stage_runner()
    a1, _, _ = sr.anchors(seqs, sorted_=False, names=names)
    a0, _, _ = sr.anchors(seqs, sorted_=False)
    assert all(np.array_equal(x, y) for x, y in zip(a0, a1))
    sr.close()
