"""_ffi.read_hits and _batch_to_mappings without a GPU: mm355_hits_t records built by hand with ctypes (as tests/test_bench_dump.py builds
them) -- tags null and non-null, a null CIGAR arena, no hits, no reads; what comes back is a copy, and the Mapping records hold what the
rows hold."""
import ctypes as C

import numpy as np
import pytest

import mappy_rs
from mappy_rs import _ffi

NAMES = ["chrA", "chrB", "chrC"]


def _record(per_read, tags=True, cigar=True, status=None):
    """one mm355_hits_t: (pointer, truth, the objects that keep its memory alive).  Hit j has j + 1 CIGAR words (none without `cigar`), a cs
    string unless j % 3 == 0 and an MD string when j is odd."""
    n_reads, nh = len(per_read), int(sum(per_read))
    off = np.concatenate([[0], np.cumsum(per_read)]).astype(np.int64)
    st = np.asarray(status if status is not None else [0] * n_reads, np.int32)
    hits = (_ffi.Hit * max(1, nh))()
    tg = (_ffi.Tags * max(1, nh))()
    words, strs, truth = [], b"", []
    for j in range(nh):
        h, t = hits[j], tg[j]
        h.query_start, h.query_end, h.strand, h.rid = 10 + j, 500 + j, (-1 if j % 2 else 1), j % 3
        h.target_len, h.target_start, h.target_end = 100000 + j, 2000 + j, 2490 + j
        h.match_len, h.block_len, h.mapq, h.is_primary, h.NM = 400 + j, 495 + j, j % 61, int(j % 4 != 1), 7 * j
        h.score0, h.dp_max, h.dp_max2, h.dp_score, h.cnt, h.n_sub, h.subsc = 300 + j, 800 + j, 40 + j, 790 + j, 30 + j, j, 100 + j
        w = [(50 + k) << 4 | (k % 3) for k in range(j + 1)] if cigar else []
        h.n_cigar, h.cigar_off = len(w), len(words)
        words += w
        cs = None if j % 3 == 0 or not cigar else (":%d*ag" % j).encode()
        md = ("%dA" % j).encode() if j % 2 and cigar else None
        h.cs_len = h.md_len = -1
        if cs is not None:
            h.cs_off, h.cs_len = len(strs), len(cs); strs += cs + b"\0"
        if md is not None:
            h.md_off, h.md_len = len(strs), len(md); strs += md + b"\0"
        t.score, t.div, t.rep_len, t.n_ambi, t.n_gap, t.n_gapo, t.flags = 310 + j, 0.015625 * (j + 1), 77, j % 2, 12 + j, 3 + j, (j % 2) | 2 * (j == 0) | (j % 4) << 2
        truth.append(dict(words=w, cs=cs, md=md))
    cig = np.asarray(words, np.uint32)
    sb = C.create_string_buffer(strs, max(1, len(strs)))
    hs = _ffi.Hits(n_reads=n_reads, hit_off=off.ctypes.data_as(C.POINTER(C.c_int64)), status=st.ctypes.data_as(C.POINTER(C.c_int32)), hits=hits,
                   str=C.cast(sb, C.POINTER(C.c_char)), n_hits=nh, n_cigar=len(cig), n_str=len(strs))
    if len(cig):
        hs.cigar = cig.ctypes.data_as(C.POINTER(C.c_uint32))      # (else: a null arena with n_cigar = 0)
    if tags:
        hs.tags = tg
    return C.pointer(hs), truth, [off, st, hits, tg, cig, sb, hs]


@pytest.mark.parametrize("tags", [False, True], ids=["no_tags", "tags"])
@pytest.mark.parametrize("cigar", [False, True], ids=["null_cigar", "cigar"])
def test_read_hits_copies_every_array(tags, cigar):
    per_read = [2, 0, 1, 0, 0, 3]
    hp, truth, keep = _record(per_read, tags=tags, cigar=cigar, status=[0, _ffi.MM355_EEMPTY, 0, 0, 0, 0])
    off, st, hits, tg, cig, sb, hs = keep
    assert bool(hs.cigar) == cigar
    v = _ffi.read_hits(hp, len(per_read))
    want_hits, want_tags, want_str = C.string_at(hits, 6 * C.sizeof(_ffi.Hit)), C.string_at(tg, 6 * C.sizeof(_ffi.Tags)), sb.raw[:hs.n_str]
    want_cig = cig.copy()

    def check():
        assert v.off.tolist() == [0, 2, 2, 3, 3, 3, 6] and v.status.tolist() == [0, _ffi.MM355_EEMPTY, 0, 0, 0, 0]
        assert v.hits.dtype == mappy_rs._HIT_DTYPE == _ffi._HIT_DTYPE and v.hits.view("u1").tobytes() == want_hits
        assert v.cigar.dtype == np.uint32 and np.array_equal(v.cigar, want_cig) and (len(v.cigar) > 0) == cigar
        assert isinstance(v.str, bytes) and v.str == want_str
        assert (v.tags is None) == (not tags)
        if tags:
            assert v.tags.dtype == mappy_rs._TAG_DTYPE and v.tags.view("u1").tobytes() == want_tags
            assert v.tags["div"].tolist() == [0.015625 * (j + 1) for j in range(6)]
        assert v.hits["NM"].tolist() == [7 * j for j in range(6)] and v.hits["cs_len"][0] == -1
    check()
    # copies: overwrite every source buffer
    off[:] = -1; st[:] = 9; cig[:] = 0
    C.memset(hits, 0xff, C.sizeof(hits)); C.memset(tg, 0xff, C.sizeof(tg)); C.memset(sb, 0x41, len(sb))
    check()


def test_read_hits_empty_records():
    hp, _, keep = _record([0, 0, 0])                     # reads, no hits
    v = _ffi.read_hits(hp, 3)
    assert v.off.tolist() == [0, 0, 0, 0] and v.status.tolist() == [0, 0, 0] and len(v.hits) == 0 and v.hits.dtype == _ffi._HIT_DTYPE
    assert len(v.cigar) == 0 and v.str == b"" and v.tags is not None and len(v.tags) == 0
    assert mappy_rs._batch_to_mappings(hp, 3, NAMES) == [[], [], []]
    hp, _, keep = _record([], tags=False)                # no reads
    v = _ffi.read_hits(hp, 0)
    assert v.off.tolist() == [0] and len(v.status) == 0 and len(v.hits) == 0 and len(v.cigar) == 0 and v.str == b"" and v.tags is None
    assert mappy_rs._batch_to_mappings(hp, 0, NAMES) == []


@pytest.mark.parametrize("tags", [False, True], ids=["no_tags", "tags"])
@pytest.mark.parametrize("cigar", [False, True], ids=["chain_only", "cigar"])
def test_batch_to_mappings_holds_the_records(tags, cigar):
    per_read = [2, 0, 1, 0, 3]
    hp, truth, keep = _record(per_read, tags=tags, cigar=cigar, status=[0, 0, 0, _ffi.MM355_EEMPTY, 0])
    hits, tg = keep[2], keep[3]
    out = mappy_rs._batch_to_mappings(hp, len(per_read), NAMES, chain_only=not cigar)
    C.memset(hits, 0xff, C.sizeof(hits)); C.memset(tg, 0xff, C.sizeof(tg)); keep[4][:] = 0; C.memset(keep[5], 0x41, len(keep[5]))
    assert isinstance(out[3], RuntimeError) and str(out[3]) == "Sequence is empty"
    assert [len(o) for i, o in enumerate(out) if i != 3] == [2, 0, 1, 3]
    flat = [m for i, o in enumerate(out) if i != 3 for m in o]
    for j, (m, t) in enumerate(zip(flat, truth)):
        assert (m.query_start, m.query_end, m.strand, m.target_name, m.target_len, m.target_start, m.target_end, m.match_len, m.block_len, m.mapq,
                m.is_primary, m.NM) == (10 + j, 500 + j, -1 if j % 2 else 1, NAMES[j % 3], 100000 + j, 2000 + j, 2490 + j, 400 + j, 495 + j, j % 61,
                                        j % 4 != 1, 7 * j)
        if tags:
            assert (m.s1, m.s2, m.cm, m.ms, m.AS, m.nn, m.rl, m.zd) == (310 + j, 100 + j, 30 + j, 800 + j, 790 + j, j % 2, 77, j % 4)
            assert m.tp == (("I" if j % 2 else "P") if j % 4 != 1 else ("i" if j % 2 else "S"))
            assert m.is_supplementary == (j % 4 != 1 and j != 0)
            assert m.dv == (None if cigar else 0.015625 * (j + 1))
            assert (m.de is None) == (not cigar)
        else:
            assert m.s1 is None and m.tp is None and m.dv is None and m.is_supplementary is None
        assert m.cigar == [(w >> 4, w & 15) for w in t["words"]]
        assert m.cs == (None if t["cs"] is None else t["cs"].decode()) and m.MD == (None if t["md"] is None else t["md"].decode())
        assert ("cg:Z:" in str(m)) == cigar
