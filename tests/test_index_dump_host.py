"""mm355_index_dump on indices with a host image (loaded from .mmi, built from FASTA / FASTQ / gzip): the file against minimap2's own
fixture and against the oracle's mmo_idx_dump of the same reference, the canonical order of include/mm355.h, the error codes, and
Aligner.save_index.  No GPU: every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import _mmi
from oracle import oracle as O


@pytest.fixture(scope="module")
def ffi(built):
    from mappy_rs import _ffi
    _ffi.lib()
    return _ffi


@pytest.fixture(scope="module")
def world(ffi, tmp_path_factory):
    """the repeat-rich reference as plain FASTA, FASTQ and gzip"""
    d = tmp_path_factory.mktemp("idxdump")
    recs = _mmi.repeat_rich_records()
    fa, fq, gz = str(d / "rep.fa"), str(d / "rep.fq"), str(d / "rep.fa.gz")
    _mmi.write_fasta(fa, recs); _mmi.write_fastq(fq, recs); _mmi.write_gzip(gz, fa)
    return dict(dir=d, recs=recs, fa=fa, fq=fq, gz=gz)


def _oracle_index(fa, k, w, flag):
    L = O.lib()
    io, mo = O.IdxOpt(), O.MapOpt()
    L.mmo_set_opt(None, C.byref(io), C.byref(mo))
    io.k, io.w, io.flag = k, w, flag
    idx = L.mmo_idx_load(fa.encode(), C.byref(io))
    assert idx
    return idx


def _oracle_entries(idx):
    """every minimizer of an oracle index with its occurrence count"""
    mi = idx.contents
    out = []
    for i in range(1 << mi.b):
        bk = mi.B[i]
        if not bk.cap:
            continue
        keys = np.ctypeslib.as_array(bk.keys, shape=(bk.cap,))
        vals = np.ctypeslib.as_array(bk.vals, shape=(bk.cap,))
        for key, val in zip(keys.tolist(), vals.tolist()):
            if key != 0xffffffffffffffff:
                out.append(((key >> 1) << mi.b | i, 1 if key & 1 else val & 0xffffffff))
    return out


def _oracle_get(idx, minier):
    n = C.c_int()
    p = O.lib().mmo_idx_get(idx, minier, C.byref(n))
    return [p[j] for j in range(n.value)]


# ------------------------------------------------------------------ 1. minimap2's own file
def test_fixture_round_trip(ffi, golden_dir, tmp_path):
    src = os.path.join(golden_dir, "test.mmi")
    rc, h = _mmi.load(ffi, src, _mmi.idxopt(ffi, 15, 10, 0))
    assert rc == 0
    try:
        ours = _mmi.parse_mmi(_mmi.dump(ffi, h, tmp_path / "out.mmi"))
    finally:
        ffi.lib().mm355_index_free(h)
    theirs = _mmi.parse_mmi(open(src, "rb").read())
    _mmi.assert_same_index(ours, theirs)       # header, contigs, S, per bucket n / size / p[] identical; pairs equal as sets
    _mmi.assert_canonical(ours)


# ------------------------------------------------------------------ 2. a repeat-rich FASTA against the oracle's own index and dump
@pytest.mark.parametrize("k,w,flag", _mmi.SETTINGS)
def test_repeat_rich_against_oracle(ffi, world, tmp_path, k, w, flag):
    L, OL = ffi.lib(), O.lib()
    io = _mmi.idxopt(ffi, k, w, flag)
    rc, h = _mmi.load(ffi, world["fa"], io)
    assert rc == 0
    mine = str(tmp_path / "mine.mmi")
    try:
        raw = _mmi.dump(ffi, h, mine)
        for other in ("fq", "gz"):               # the FASTQ and the gzip copy are the same reference
            rc2, h2 = _mmi.load(ffi, world[other], io)
            assert rc2 == 0
            try:
                assert _mmi.dump(ffi, h2, tmp_path / (other + ".mmi")) == raw
            finally:
                L.mm355_index_free(h2)
    finally:
        L.mm355_index_free(h)
    ours = _mmi.parse_mmi(raw)
    assert (ours["k"], ours["w"], ours["flag"], ours["n_seq"]) == (k, w, flag, len(world["recs"]))
    assert ours["b"] == min(14, 2 * k)
    _mmi.assert_canonical(ours)
    orc = _oracle_index(world["fa"], k, w, flag)
    back = None
    try:
        theirs_fn = str(tmp_path / "oracle.mmi")
        assert OL.mmo_idx_dump(orc, theirs_fn.encode()) == 0
        theirs = _mmi.parse_mmi(open(theirs_fn, "rb").read())
        _mmi.assert_same_index(ours, theirs)
        longest = max((int(v) & 0xffffffff for _, pairs in ours["buckets"] for kk, v in pairs if not int(kk) & 1), default=0)
        assert longest >= 100                    # the tandem repeat is in there
        if k == 6:
            assert all(len(pairs) <= 1 for _, pairs in ours["buckets"]) and len(ours["buckets"]) == 4096
        # the oracle reads OUR file
        io_o = O.IdxOpt()
        back = OL.mmo_idx_load(mine.encode(), C.byref(io_o))
        assert back
        nd, nd2 = C.c_int64(), C.c_int64()
        assert OL.mmo_idx_n_minimizers(back, C.byref(nd)) == OL.mmo_idx_n_minimizers(orc, C.byref(nd2)) and nd.value == nd2.value > 0
        ents = _oracle_entries(orc)
        assert len(ents) == nd2.value
        for minier, cnt in ents:
            want = _oracle_get(orc, minier)
            assert len(want) == cnt and _oracle_get(back, minier) == want
        for rid, (_, s) in enumerate(world["recs"]):
            a, b = np.zeros(len(s), np.uint8), np.full(len(s), 9, np.uint8)
            assert OL.mmo_idx_getseq(orc, rid, 0, len(s), a.ctypes.data) == len(s)
            assert OL.mmo_idx_getseq(back, rid, 0, len(s), b.ctypes.data) == len(s)
            assert a.tobytes() == b.tobytes() == bytes("ACGTN".index(c) for c in s)
    finally:
        OL.mmo_idx_destroy(orc)
        if back:
            OL.mmo_idx_destroy(back)


# ------------------------------------------------------------------ 3. fixed point
@pytest.mark.parametrize("k,w,flag", _mmi.SETTINGS)
def test_dump_is_a_fixed_point(ffi, world, tmp_path, k, w, flag):
    L = ffi.lib()
    io = _mmi.idxopt(ffi, k, w, flag)
    rc, h = _mmi.load(ffi, world["fa"], io)
    assert rc == 0
    try:
        first = _mmi.dump(ffi, h, tmp_path / "a.mmi")
        assert _mmi.dump(ffi, h, tmp_path / "b.mmi") == first          # two dumps of one index
    finally:
        L.mm355_index_free(h)
    rc, h = _mmi.load(ffi, tmp_path / "a.mmi", _mmi.idxopt(ffi, 15, 10, 0))   # (the file decides k, w, flag)
    assert rc == 0
    try:
        assert _mmi.dump(ffi, h, tmp_path / "c.mmi") == first
    finally:
        L.mm355_index_free(h)


# ------------------------------------------------------------------ 4. MM_I_NO_SEQ
def test_no_seq_index(ffi, golden_dir, tmp_path):
    L = ffi.lib()
    orc = O.OracleAligner(os.path.join(golden_dir, "test.fa"))
    src = str(tmp_path / "full.mmi")
    assert O.lib().mmo_idx_dump(orc.idx, src.encode()) == 0
    raw = bytearray(open(src, "rb").read())
    raw[20:24] = (2).to_bytes(4, "little")                                # as tests/test_gpu_chain_only.py: the flag set, S cut off
    noseq = bytes(raw[:-((4 * 400 + 7) // 8 * 4)])
    (tmp_path / "noseq.mmi").write_bytes(noseq)
    io = _mmi.idxopt(ffi, 15, 10, 0)
    rc, h = _mmi.load(ffi, tmp_path / "noseq.mmi", io)
    assert rc == 0
    try:
        out = _mmi.dump(ffi, h, tmp_path / "out.mmi")
    finally:
        L.mm355_index_free(h)
    m = _mmi.parse_mmi(out)
    assert m["flag"] == 2 and m["S"] == b""
    _mmi.assert_same_index(m, _mmi.parse_mmi(noseq))
    rc, h = _mmi.load(ffi, tmp_path / "out.mmi", io)
    assert rc == 0
    try:
        fl = C.c_int32()
        L.mm355_index_info(h, None, None, None, C.byref(fl), None)
        assert fl.value == 2 and L.mm355_index_getseq(h, 0, 0, 10, (C.c_uint8 * 10)()) == -1
        assert _mmi.dump(ffi, h, tmp_path / "again.mmi") == out
    finally:
        L.mm355_index_free(h)


# ------------------------------------------------------------------ 5. errors
def test_errors(ffi, golden_dir, tmp_path):
    L = ffi.lib()
    rc, h = _mmi.load(ffi, os.path.join(golden_dir, "test.mmi"), _mmi.idxopt(ffi, 15, 10, 0))
    assert rc == 0
    try:
        bad = tmp_path / "no_such_dir" / "x.mmi"
        assert L.mm355_index_dump(h, str(bad).encode()) == ffi.MM355_EIO and not bad.exists() and not bad.parent.exists()
        assert L.mm355_index_dump(h, str(tmp_path).encode()) == ffi.MM355_EIO and tmp_path.is_dir()      # a directory cannot be created as a file
        assert L.mm355_index_dump(None, str(tmp_path / "null.mmi").encode()) == ffi.MM355_ENOIDX and not (tmp_path / "null.mmi").exists()
    finally:
        L.mm355_index_free(h)
    for n_name, want in ((255, 0), (256, ffi.MM355_EINVAL)):
        h = _mmi.build(ffi, [("n" * n_name, "ACGTTGCAGGCTAATCGGATCCATTAGACCAGTTGA" * 4)], _mmi.idxopt(ffi, 15, 10, 0))
        try:
            f = tmp_path / ("name%d.mmi" % n_name)
            assert L.mm355_index_dump(h, str(f).encode()) == want
            assert f.exists() == (want == 0)
            if want == 0:
                assert _mmi.parse_mmi(f.read_bytes())["contigs"][0] == (b"n" * 255, 144)
        finally:
            L.mm355_index_free(h)


# ------------------------------------------------------------------ 6. Python
def test_aligner_save_index(ffi, golden_dir, tmp_path):
    import mappy_rs
    mmi = os.path.join(golden_dir, "test.mmi")
    al = mappy_rs.Aligner(mmi)
    p = str(tmp_path / "saved.mmi")
    assert al.save_index(p) is None
    al2 = mappy_rs.Aligner(p)
    assert (al2.k, al2.w, al2.n_seq, al2.seq_names) == (al.k, al.w, al.n_seq, al.seq_names)
    for name in al.seq_names:
        assert al2.seq(name) == al.seq(name) and al2.seq(name, 5, 25) == al.seq(name, 5, 25) and len(al.seq(name, 5, 25)) == 20
    al.save_index(tmp_path / "as_path.mmi")                               # os.PathLike
    assert (tmp_path / "as_path.mmi").read_bytes() == open(p, "rb").read()
    with pytest.raises(RuntimeError, match="^mm355: "):
        al.save_index(str(tmp_path / "missing" / "x.mmi"))
    with pytest.raises(NotImplementedError, match="Not Implemented"):
        mappy_rs.Aligner(mmi, seq="ACGT")
    with pytest.raises(NotImplementedError, match="Not Implemented"):
        mappy_rs.Aligner(mmi, fn_idx_out="x")
    assert not os.path.exists("x")
    assert mappy_rs.Aligner(mmi, build_on_gpu=False).seq_names == al.seq_names
