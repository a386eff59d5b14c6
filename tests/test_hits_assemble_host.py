"""The assembler of mm355_hits_t (mappy-rs_amd/csrc/mm355_hits.h) on the CPU: compiled with g++ (tests/host_harness/hits_host.cpp), fed
hand-made spans -- rows of a "device" buffer at scattered offsets between rows of per-read vectors, reads without rows, an empty read,
CIGAR words and cs / MD strings, tags on and off, the chain-only form, no reads at all -- and every array of the record is compared with
a layout computed here in numpy.  Every record is released with mm355_free_hits."""
import ctypes as C

import numpy as np
import pytest

from mappy_rs import _ffi
import _capi

HIT, TAG = _ffi._HIT_DTYPE, _ffi._TAG_DTYPE


@pytest.fixture(scope="module")
def hits_lib():
    L = _capi.build_harness("hits_host", flags=["-Wall"], headers=["mm355_hits.h"])
    L.hits_assemble_host.argtypes = [C.c_int64] + [C.c_void_p] * 8 + [C.c_int, C.POINTER(C.POINTER(_ffi.Hits))]
    L.mm355_free_hits.argtypes = [C.POINTER(_ffi.Hits)]
    return L


def _rows(rng, n):
    """n hit rows and tags rows of random bytes (padding and reserved words included: the assembler copies rows whole)"""
    h = np.frombuffer(rng.integers(0, 256, n * HIT.itemsize, dtype=np.uint8).tobytes(), dtype=HIT).copy()
    t = np.frombuffer(rng.integers(0, 256, n * TAG.itemsize, dtype=np.uint8).tobytes(), dtype=TAG).copy()
    h["cigar_off"] = h["n_cigar"] = h["cs_off"] = h["md_off"] = 0
    h["cs_len"] = h["md_len"] = -1
    return h, t


def _vector_read(rng, spec):
    """a read of the host path.  spec: per row (n_cigar, cs, md) with cs / md a bytes object or None.  Returns rows, tags, CIGAR words, string
    bytes; a row without a string keeps an arbitrary offset (77 / 99) that must come out unchanged."""
    h, t = _rows(rng, len(spec))
    words, s = [], b""
    for k, (nc, cs, md) in enumerate(spec):
        h["n_cigar"][k], h["cigar_off"][k] = nc, len(words)
        words += rng.integers(1, 1 << 20, nc).tolist()
        h["cs_off"][k], h["md_off"][k] = 77, 99
        if cs is not None:
            h["cs_off"][k], h["cs_len"][k] = len(s), len(cs); s += cs + b"\0"
        if md is not None:
            h["md_off"][k], h["md_len"][k] = len(s), len(md); s += md + b"\0"
    return h, t, np.asarray(words, np.uint32), s


def _assemble(L, reads, status, want_tags, pass_tags=True):
    """reads: per read (hits, tags, cigar words, string bytes), arrays or views.  Returns the HitsView of the record, after freeing it."""
    n = len(reads)
    keep = [(np.ascontiguousarray(c), C.create_string_buffer(s, max(1, len(s)))) for _, _, c, s in reads]
    addr = lambda a: a.ctypes.data if len(a) else 0
    nr = np.asarray([len(h) for h, _, _, _ in reads], np.int64)
    ncg = np.asarray([len(c) for _, _, c, _ in reads], np.int64)
    nst = np.asarray([len(s) for _, _, _, s in reads], np.int64)
    hp = np.asarray([addr(h) for h, _, _, _ in reads], np.uint64)
    tp = np.asarray([addr(t) for _, t, _, _ in reads], np.uint64)
    cp = np.asarray([addr(c) for c, _ in keep], np.uint64)
    sp = np.asarray([C.addressof(b) if len(s) else 0 for (_, b), (_, _, _, s) in zip(keep, reads)], np.uint64)
    st = np.asarray(status, np.int32)
    out = C.POINTER(_ffi.Hits)()
    p = lambda a: a.ctypes.data if len(a) else None
    rc = L.hits_assemble_host(n, p(st), p(nr), p(hp), p(tp) if pass_tags else None, p(ncg), p(cp), p(nst), p(sp), int(want_tags), C.byref(out))
    assert rc == 0 and out
    h = out.contents
    assert h.n_reads == n and bool(h.hit_off) and bool(h.status) and bool(h.hits) and bool(h.cigar) and bool(h.str)     # arenas never null
    assert bool(h.tags) == bool(want_tags)
    v = _ffi.read_hits(out, n)
    counts = (int(h.n_hits), int(h.n_cigar), int(h.n_str))
    L.mm355_free_hits(out)
    return v, counts


def _expected(reads):
    """the layout in numpy: rows in read order, cigar_off rebased by the words before the read, cs_off / md_off by the bytes before it where
    the length is >= 0"""
    off = np.concatenate([[0], np.cumsum([len(h) for h, _, _, _ in reads])]).astype(np.int64)
    raw = lambda xs, dt: np.frombuffer(bytearray(b"".join(_capi.raw(x) for x in xs)), dtype=dt)      # (bytes: the padding travels too, which a structured copy does not promise)
    hits, nc, ns = raw([h for h, _, _, _ in reads], HIT), 0, 0
    for i, (_, _, c, s) in enumerate(reads):
        h = hits[off[i]:off[i + 1]]
        h["cigar_off"] += nc
        h["cs_off"] += np.where(h["cs_len"] >= 0, ns, 0)
        h["md_off"] += np.where(h["md_len"] >= 0, ns, 0)
        nc += len(c); ns += len(s)
    return (off, hits, raw([t for _, t, _, _ in reads], TAG), raw([np.asarray(c, np.uint32) for _, _, c, _ in reads], np.uint32),
            b"".join(s for _, _, _, s in reads))


NO_C, NO_S = np.zeros(0, np.uint32), b""


def _world(rng):
    """first read without rows, two in a row, the last one; device spans at hoff 40, 3 and 17 between four vector reads.  `v0` fills both
    arenas (2 words, 5 bytes) before any other read, so every later vector row is rebased by a shift that is not zero."""
    dev_h, dev_t = _rows(rng, 64)
    dev = lambda a, n: (dev_h[a:a + n], dev_t[a:a + n], NO_C, NO_S)
    none = (dev_h[:0], dev_t[:0], NO_C, NO_S)
    v0 = _vector_read(rng, [(2, b":9", b"9")])
    va = _vector_read(rng, [(3, b":12*ag", b"12A"), (1, None, None), (4, b"", None)])        # cs_len = -1 beside cs_len = 0
    vb = _vector_read(rng, [(2, None, b"5^AC3")])                                             # md without cs
    vc = _vector_read(rng, [(0, b":7", None), (5, b"+a:3", b"3"), (1, b"", b"")])             # cs_len = 0 and md_len = 0
    reads = [none, v0, dev(40, 3), va, none, none, dev(3, 1), vb, dev(17, 2), vc, none]
    status = [_ffi.MM355_EEMPTY, 0, 0, 0, 0, _ffi.MM355_EEMPTY, 0, 0, 0, 0, 0]
    return reads, status


@pytest.mark.parametrize("want_tags", [False, True], ids=["no_tags", "tags"])
def test_mixed_sources_cigar_and_strings(hits_lib, want_tags):
    reads, status = _world(np.random.default_rng(3))
    v, (nh, nc, ns) = _assemble(hits_lib, reads, status, want_tags)
    off, hits, tags, cig, s = _expected(reads)
    assert nh == len(hits) == 14 and nc == len(cig) == 18 and ns == len(s) == 35
    assert np.array_equal(v.off, off) and v.off.tolist() == [0, 0, 1, 4, 7, 7, 7, 8, 9, 11, 14, 14] and v.status.tolist() == status
    assert _capi.raw(v.hits) == _capi.raw(hits)
    assert np.array_equal(v.cigar, cig) and v.str == s
    assert (_capi.raw(v.tags) == _capi.raw(tags)) if want_tags else v.tags is None
    # The rules in literal numbers, worked by hand.  `va` (rows 4..6) lies behind 2 words and 5 bytes: its offsets were 0 / 3 / 4 words,
    # cs at 0 / - / 11 and MD at 7 / - / -; an offset whose length is -1 (77, 99) stays, the one whose length is 0 moves.
    a = v.hits[4:7]
    assert a["cigar_off"].tolist() == [2, 5, 6] and a["cs_len"].tolist() == [6, -1, 0] and a["md_len"].tolist() == [3, -1, -1]
    assert a["cs_off"].tolist() == [5, 77, 16] and a["md_off"].tolist() == [12, 99, 99]
    assert s[5:11] == b":12*ag" and s[12:15] == b"12A" and s[16:17] == b"\0"
    # `vb` (row 8) behind 10 words and 17 bytes: MD without cs
    b = v.hits[8]
    assert (b["cigar_off"], b["cs_len"], b["cs_off"], b["md_len"], b["md_off"]) == (10, -1, 77, 5, 17) and s[17:22] == b"5^AC3"
    # `vc` (rows 11..13) behind 12 words and 23 bytes; its last row has an empty cs at 10 and an empty MD at 11: both move
    c = v.hits[11:14]
    assert c["cigar_off"].tolist() == [12, 12, 17] and c["cs_off"].tolist() == [23, 26, 33] and c["md_off"].tolist() == [99, 31, 34]
    assert c["cs_len"].tolist() == [2, 4, 0] and c["md_len"].tolist() == [-1, 1, 0] and s[26:30] == b"+a:3" and s[31:32] == b"3"


def test_rows_without_a_tags_source(hits_lib):
    """tags not asked for: the spans' tags pointers are not read (the CIGAR path passes none)"""
    reads, status = _world(np.random.default_rng(4))
    v, _ = _assemble(hits_lib, reads, status, False, pass_tags=False)
    assert v.tags is None and _capi.raw(v.hits) == _capi.raw(_expected(reads)[1])


@pytest.mark.parametrize("want_tags", [False, True], ids=["no_tags", "tags"])
def test_chain_only_form(hits_lib, want_tags):
    rng = np.random.default_rng(5)
    dev_h, dev_t = _rows(rng, 32)
    vh, vt = _rows(rng, 2)
    reads = [(dev_h[20:22], dev_t[20:22], NO_C, NO_S), (dev_h[:0], dev_t[:0], NO_C, NO_S), (vh, vt, NO_C, NO_S), (dev_h[5:8], dev_t[5:8], NO_C, NO_S)]
    v, counts = _assemble(hits_lib, reads, [0, _ffi.MM355_EEMPTY, 0, 0], want_tags)         # (_assemble: the two arenas are not null)
    off, hits, tags, _, _ = _expected(reads)
    assert counts == (7, 0, 0) and len(v.cigar) == 0 and v.str == b""
    assert np.array_equal(v.off, off) and _capi.raw(v.hits) == _capi.raw(hits) and v.status.tolist() == [0, _ffi.MM355_EEMPTY, 0, 0]
    assert (_capi.raw(v.tags) == _capi.raw(tags)) if want_tags else v.tags is None


@pytest.mark.parametrize("want_tags", [False, True], ids=["no_tags", "tags"])
def test_no_reads_and_no_rows(hits_lib, want_tags):
    v, counts = _assemble(hits_lib, [], [], want_tags)
    assert counts == (0, 0, 0) and v.off.tolist() == [0] and len(v.status) == 0 and len(v.hits) == 0
    none = (np.zeros(0, HIT), np.zeros(0, TAG), NO_C, NO_S)
    v, counts = _assemble(hits_lib, [none, none], [0, _ffi.MM355_EEMPTY], want_tags)
    assert counts == (0, 0, 0) and v.off.tolist() == [0, 0, 0] and v.status.tolist() == [0, _ffi.MM355_EEMPTY] and len(v.hits) == 0
    assert (v.tags is not None and len(v.tags) == 0) if want_tags else v.tags is None
