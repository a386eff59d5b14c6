"""The BAM writer on the GPU (mm355_recdev.h with BamFmt: k_rec_len, the scans, k_rec_fields; mm355_bam.hip: k_bam_bulk, k_bgzf_frame): the framing kernel against
tests/_bam.py::frame byte for byte; the device formatter against the host formatter and record_of of mappy_rs.sam_lines on constructed
result sets (tests/_bam_sets.py); end to end through Aligner.map_bam on the two-contig world of tests/test_gpu_tags.py, and from a reads
file to a BAM file through Aligner.map_bam_file; and the three writers in turn on one context, whose one set of buffers they share.
CPU side: tests/test_bam_host.py."""
import ctypes as C
import gzip
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import synthdata as S
import _bam
import _bam_sets as BS
import _capi
import _paf_sets as PS
import _sam_sets as SS
from test_gpu_tags import world, _rc          # noqa: F401  (the fixture: its genome and reads)
from test_gpu_sam import _format as _sam_format, _sam_reads, _write_fastq_gz

OUT_CS, OUT_MD, OUT_TAGS = 1, 2, 4
P = _bam.PAYLOAD
TILE = 4096                                   # BAM_TILE of mm355_bam.hip: output bytes of one k_bam_bulk block (8192 bases, 4096 quality bytes)
CHUNK, LANES = 256, 256                       # BGZF_CHUNK, BGZF_LANES: the framing kernel's CRC chunk per lane


@pytest.fixture(scope="module")
def stage(built, tmp_path_factory):
    """an Aligner whose index has the contig names of the constructed sets"""
    import mappy_rs
    fa = str(tmp_path_factory.mktemp("gbam") / "three.fa")
    S.write_fasta(fa, S.make_genome(5, [3000, 3000, 3000]), SS.CONTIGS)
    al = mappy_rs.Aligner(fa, preset="map-ont")
    assert al.seq_names == SS.CONTIGS
    return al


# ---------------------------------------------------------------- framing on the device
def _wrap(al, data, where):
    from mappy_rs import _ffi
    tp = C.POINTER(_ffi.Text)()
    _ffi.check(al._L.mm355_bgzf_wrap(al._context(), data, len(data), where, C.byref(tp)))
    try:
        t = tp.contents
        assert t.n_lines == (len(data) + P - 1) // P and t.n_reads == 0
        return bytes(_ffi.text_view(tp)), t.on_device
    finally:
        al._L.mm355_free_text(tp)


def test_device_framing_equals_frame(stage):
    """every length at which the kernel takes another path: nothing, one byte, each side of a lane's chunk and of the last lane but one,
    each side of chunk x lanes and of the block payload, three blocks and a tail; random bytes, zeros and 0xFF (a CRC that mishandles
    leading zeros or its final inversion passes random data only by luck)"""
    from mappy_rs import _ffi
    rng = np.random.default_rng(17)
    sizes = (0, 1, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, P - CHUNK - 1, P - CHUNK, P - CHUNK + 1, P - 1, P, P + 1,
             CHUNK * LANES - 1, CHUNK * LANES, CHUNK * LANES + 1, 3 * P + 77)
    for n in sizes:
        for fill in (None, 0, 255):
            data = rng.integers(0, 256, n, dtype=np.uint8).tobytes() if fill is None else bytes([fill]) * n
            want = _bam.frame(data)
            got, on = _wrap(stage, data, _ffi.PAF_DEVICE)
            assert on == 1 and got == want, (n, fill, len(got), len(want), next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), -1))
            assert _bam.inflate(got) == data
    data = rng.integers(0, 256, P + 5, dtype=np.uint8).tobytes()
    for where in (_ffi.PAF_HOST, _ffi.PAF_AUTO):
        assert _wrap(stage, data, where) == (_bam.frame(data), 0)
    import mappy_rs
    assert mappy_rs.bgzf_wrap(data) == _bam.frame(data) and mappy_rs.bgzf_wrap(b"") == b"" and mappy_rs.BAM_EOF == _bam.EOF


# ---------------------------------------------------------------- the device formatter
def _format(al, s, where, mo=None, sam_flags=None, raw=False):
    """mm355_bam_format on the set -> (BGZF bytes, line_off, on_device, n_lines), or the return code alone"""
    from mappy_rs import _ffi
    L = al._L
    h, qn, sp, ql, qp, rl, keep = s if raw else SS.sam_args(s)
    tp = C.POINTER(_ffi.Text)()
    fl = sam_flags if sam_flags is not None else 0 if raw else s["sam_flags"]
    rc = L.mm355_bam_format(al._context(), C.byref(mo or al._mo), C.byref(h), qn, sp, ql, qp, rl, fl, where, C.byref(tp))
    if raw:
        assert not tp or rc == 0
        if tp:
            L.mm355_free_text(tp)
        return rc
    _ffi.check(rc)
    try:
        t = tp.contents
        assert t.n_reads == len(s["seqs"]) and t.ms_format >= 0.0
        return bytes(_ffi.text_view(tp)), [t.line_off[i] for i in range(t.n_reads + 1)], t.on_device, t.n_lines
    finally:
        L.mm355_free_text(tp)


def _row(qs, qe, strand, kind, cigar, n_cigar=1, rid=0, ts=100):
    """a row over read[qs:qe]: kind 0 the primary with sam_pri, 1 a supplementary, 2 a secondary; its CIGAR words are appended to `cigar`"""
    r = dict(query_start=qs, query_end=qe, strand=strand, rid=rid, target_len=3000, target_start=ts, target_end=ts + (qe - qs), match_len=qe - qs,
             block_len=max(1, qe - qs), mapq=60, is_primary=int(kind != 2), n_cigar=n_cigar, cigar_off=len(cigar))
    cigar += [max(1, qe - qs) << 4] + [3 << 4 | 7] * (n_cigar - 1)
    return r, dict(score=qe - qs, flags=2 if kind == 0 else 0)


def _alignment_sets(rng):
    """SEQ / QUAL runs whose source and destination move independently through all residues mod 16 (an odd slice start puts a base in each
    nibble of a source byte pair): 16 reads per set, the name (and so the destination) `d` bytes long and the slice start at base `q`; per
    length one set where both grow from read to read, one where only the name grows and one where only the slice start moves; lengths 1, 2,
    around the 32 bases of a 16-byte piece, around the wave and around the tile of packed bases (2 x TILE) and of quality bytes (TILE).  Per
    read: the whole read forwards, a reverse-strand and a forward hard-clipped slice of the length; every third read without quality."""
    out = []
    for k, ln in enumerate((1, 2, 31, 32, 33, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 4 * TILE + 3)):
        fixed = 1 + (5 * k) % 16
        for walk in (lambda a: (a + 1, a), lambda a: (a + 1, fixed), lambda a: (fixed, a)):
            rows, tags, cigar, hit_off, names, seqs, quals = [], [], [], [0], [], [], []
            for a in range(16):
                d, q = walk(a)
                seq, qual = SS.random_read(rng, ln + 40 + a)
                for r, t in (_row(0, len(seq), 1, 0, cigar), _row(q, q + ln, -1, 1, cigar, a % 5 + 1, 1), _row(q + 3, q + 3 + ln, 1, 1, cigar, 1, 2)):
                    rows.append(r); tags.append(t)
                hit_off.append(len(rows)); names.append("n" * d); seqs.append(seq); quals.append(qual if a % 3 else None)
            out.append(BS.scrub(SS.make_set(rows, tags, hit_off, [0] * 16, names, seqs, quals, [0] * 16, 0, cigar=cigar), rng))
    return out


def _straddle_set(rng):
    """three unmapped reads: the first record is 0xff00 bytes exactly and ends on the block boundary, the second begins the second block, the
    third straddles the boundary between the second and the third"""
    n = (P - 36 - 2 - 4) * 2 // 3                       # 36 fixed bytes, "a" and its NUL, rl:C: the rest is 1.5 bytes per base
    reads = [SS.random_read(rng, k) for k in (n, 30000, 30000)]
    s = BS.scrub(SS.make_set([], [], [0, 0, 0, 0], [0, 0, 0], ["a", "b", "c"], [r for r, _ in reads], [q for _, q in reads], [7, 8, 9], 0), rng)
    recs = BS.expected(s)[0]
    assert len(recs[0]) == P and len(recs[0]) + len(recs[1]) < 2 * P < sum(map(len, recs))
    return s


def test_device_formatter_equals_host_and_record_of(stage, monkeypatch):
    from mappy_rs import _ffi
    al = stage
    rng = np.random.default_rng(12)
    special = [_straddle_set(rng), BS.boundary_set(), BS.long_cigar_set(65535, rng, -1), BS.long_cigar_set(65536, rng, 1), BS.long_cigar_set(65536, rng, -1, n_reads=2),
               SS.make_set([], [], [0, 0, 0], [0, SS.EEMPTY], ["a", None], ["ACGT", ""], [None, None], [3, 0], SS.HIT_ONLY)]
    sets = BS.random_sets(357, 300) + _alignment_sets(rng) + special
    n_rec = 0
    for k, s in enumerate(sets):
        want, want_off = BS.expected(s)
        framed = _bam.frame(b"".join(want))
        host, host_off, on, nl = _format(al, s, _ffi.PAF_HOST)
        assert on == 0 and host == framed and host_off == want_off and nl == len(want), k
        dev, dev_off, on, nl = _format(al, s, _ffi.PAF_DEVICE)
        assert on == 1 and nl == len(want), k
        if dev != framed:
            got = _bam.cut(gzip.decompress(dev)) if dev else []
            bad = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), -1)
            at = next((i for i, (a, b) in enumerate(zip(got[bad], want[bad])) if a != b), -1) if bad >= 0 else -1
            assert False, (k, len(dev), len(framed), len(got), len(want), bad, at, got[bad][max(0, at - 24):at + 24].hex() if bad >= 0 else "",
                           want[bad][max(0, at - 24):at + 24].hex() if bad >= 0 else "")
        assert dev_off == want_off, k
        n_rec += len(want)
    assert n_rec > 2500 and _format(al, special[-1], _ffi.PAF_DEVICE)[0] == b""
    # MM355_PAF_AUTO: the hit count against MM355_BAM_MIN_HITS
    twelve = BS.boundary_set()
    for env, on in (("1", 1), ("13", 0), ("12", 1)):
        monkeypatch.setenv("MM355_BAM_MIN_HITS", env)
        assert _format(al, twelve, _ffi.PAF_AUTO)[2] == on


def test_format_refuses_what_bam_cannot_hold(stage):
    """MM355_EINVAL from both formatters, before anything is allocated or launched"""
    from mappy_rs import _ffi
    for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
        for name, s in BS.refused_sets():
            rc = _format(stage, SS.sam_args(s), where, raw=True, sam_flags=s["sam_flags"])
            assert rc == (0 if name in ("good", "name254") else _ffi.MM355_EINVAL), (where, name)


# ---------------------------------------------------------------- all writers on one context
def _shared_buffer_sets(rng):
    """large: three reads -- one of 2 * TILE + 1 bases with quality, whose primary has a CIGAR of 150 operations and cs and MD strings and whose
    reverse-strand hard-clipped supplementary has 70 operations and takes more than a tile, one without quality, one without hits: more than
    one tile per run, more than one CIGAR tile of the wave.  small: one read of 40 bases, one hit."""
    cigar, sbuf = [], b":17*ac:5\0" + b"17A3^C" * 40 + b"\0"
    (sq0, ql0), (sq1, _), (sq2, ql2) = SS.random_read(rng, 2 * TILE + 1), SS.random_read(rng, 333), SS.random_read(rng, 77)
    rows = [_row(0, len(sq0), 1, 0, cigar, 150), _row(17, 17 + TILE + 5, -1, 1, cigar, 70, 1), _row(3, 300, -1, 2, cigar, 3, 2)]
    rows[0][0].update(cs_off=0, cs_len=9, md_off=10, md_len=240)
    large = BS.scrub(SS.make_set([r for r, _ in rows], [t for _, t in rows], [0, 2, 3, 3], [0, 0, 0], ["first read", "second", None], [sq0, sq1, sq2],
                                 [ql0, None, ql2], [0, 0, 5], 0, cigar=cigar, sbuf=sbuf), rng)
    cigar = []
    sq, ql = SS.random_read(rng, 40)
    r, t = _row(2, 38, 1, 0, cigar)
    small = BS.scrub(SS.make_set([r], [t], [0, 1], [0], ["s"], [sq], [ql], [0], 0, cigar=cigar), rng)
    return large, small


def test_all_writers_share_one_context(built, tmp_path):
    """mm355_bam_format, _paf_format, _sam_format, _paf_format, _bam_format, mm355_bgzf_wrap, _sam_format on one context, on the device, the
    large and the small set by turns, beginning once with the small one on a context that has written nothing (every buffer has to grow for
    the large one) and once with the large one: each result is the host formatter's on the same set.  A length taken from a buffer's
    capacity, or from what the call before left there, shows in a small call after a large one."""
    import mappy_rs
    from mappy_rs import _ffi
    fa = str(tmp_path / "three.fa")
    S.write_fasta(fa, S.make_genome(5, [3000, 3000, 3000]), SS.CONTIGS)
    al = mappy_rs.Aligner(fa, preset="map-ont")
    L = al._L

    def bam(s, where):
        return _format(al, s, where)

    def paf(s, where):
        h, qn, ql, keep = PS.hits_struct(s)
        tp = C.POINTER(_ffi.Text)()
        _ffi.check(L.mm355_paf_format(al._context(), C.byref(al._mo), C.byref(h), qn, ql, where, C.byref(tp)))   # (al._mo: CIGAR mode)
        try:
            t = tp.contents
            return bytes(_ffi.text_view(tp)), [t.line_off[i] for i in range(t.n_reads + 1)], t.on_device, t.n_lines
        finally:
            L.mm355_free_text(tp)

    def sam(s, where):
        text, off, on = _sam_format(al, s, where)
        return text, off, on, text.count(b"\n")

    def wrap(s, where):
        data = b"".join(BS.expected(s)[0])
        return _wrap(al, data, where) + (len(data),)

    sets = _shared_buffer_sets(np.random.default_rng(31))
    assert len(sets[0]["cigar"]) > 64 and sets[0]["hits"][1]["strand"] < 0 and len(sets[0]["seqs"][0]) == 2 * TILE + 1 and len(sets[1]["seqs"][0]) == 40
    calls = (bam, paf, sam, paf, bam, wrap, sam)
    want = {(f, k): f(s, _ffi.PAF_HOST) for f in set(calls) for k, s in enumerate(sets)}
    assert all(w[-2] == 0 for w in want.values()) and want[(paf, 0)][3] == 3 and want[(sam, 0)][3] == 4 and want[(paf, 1)][3] == 1
    for first in (1, 0):
        for n, f in enumerate(calls):
            k = (first + n) % 2
            got = f(sets[k], _ffi.PAF_DEVICE)
            w = want[(f, k)]
            assert got[-2] == 1 and got[0] == w[0] and (f is wrap or got[1] == w[1]) and got[-1] == w[-1], (first, n, k, len(got[0]), len(w[0]))


# ---------------------------------------------------------------- end to end
def _records_of_sam(al, text):
    return [_bam.record_of(ln, al.seq_names) for ln in text.split(b"\n")[:-1]]


@pytest.mark.parametrize("preset,kw", [("map-ont", dict(cs=True)), ("map-ont", dict(MD=True)), ("map-hifi", {})], ids=["map-ont-cs", "map-ont-MD", "map-hifi"])
def test_map_bam(world, preset, kw):
    import mappy_rs
    from mappy_rs import _ffi
    al = mappy_rs.Aligner(world["fa"], preset=preset)
    reads, names, quals = _sam_reads(world)
    for more in (dict(quals=quals), dict(quals=None, softclip=True), dict(quals=quals, hit_only=True)):
        sam = al.map_sam(reads, names=names, where=_ffi.PAF_HOST, **kw, **more)
        want = _records_of_sam(al, sam)
        flags = {struct.unpack_from("<H", r, 18)[0] for r in want}
        assert ({2048, 2064, 256} <= flags) and ((4 in flags) == ("hit_only" not in more)) and any(b"SAZ" in r for r in want)
        assert any(b"csZ" in r for r in want) == ("cs" in kw) and any(b"MDZ" in r for r in want) == ("MD" in kw)
        for where, on in ((_ffi.PAF_HOST, False), (_ffi.PAF_DEVICE, True)):
            got = al.map_bam(reads, names=names, where=where, **kw, **more)
            assert al.paf_on_device is on
            assert got == _bam.frame(b"".join(want)), (more.keys(), where, len(got))
    if preset == "map-hifi":
        with pytest.raises(ValueError):
            al.map_bam(reads[:2], quals=["II"])
        with pytest.raises(TypeError):
            al.map_bam([b"ACGT"])
        with pytest.raises(RuntimeError):
            al.map_bam(reads[:2], names=["n" * 255, None])
        with pytest.raises(ValueError):
            mappy_rs.Aligner(world["fa"], preset="map-ont", cigar=False).map_bam(reads[:2])


def _header_payload(al):
    text = al.sam_header()
    refs = b"".join(struct.pack("<I", len(n) + 1) + n.encode() + b"\0" + struct.pack("<I", len(al.seq(n))) for n in al.seq_names)
    return b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(al.seq_names)) + refs


def test_map_bam_file(world, tmp_path):
    """reads file in, BAM file out: header blocks, the records in input order across three workers and sub-batches of 64 reads, the EOF block"""
    import mappy_rs
    from mappy_rs import _ffi
    reads, _, _ = _sam_reads(world, n_plain=120)
    reads = reads[:-1]                                                   # (a FASTQ record has bases)
    names = ["r%03d" % i for i in range(len(reads))]
    quals = ["@" + "".join(chr(35 + (i + j) % 50) for j in range(len(r) - 1)) for i, r in enumerate(reads)]
    fq, fa = str(tmp_path / "reads.fq.gz"), str(tmp_path / "reads.fa")
    _write_fastq_gz(fq, reads, names, quals)
    with open(fa, "w") as f:
        f.write("".join(">%s\n%s\n" % (n, r) for n, r in zip(names, reads)))
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", tags=True, devices=[0])
    assert al.bam_header() == _bam.frame(_header_payload(al))
    al.enable_threading(3)
    sam, paf = str(tmp_path / "out.sam"), str(tmp_path / "out.paf")
    al.map_file(fq, sam, cs=True, sub_batch_reads=64, format="sam")
    al.map_file(fq, paf, cs=True, sub_batch_reads=64)
    sam_before, paf_before = open(sam, "rb").read(), open(paf, "rb").read()
    want = _records_of_sam(al, sam_before[len(al.sam_header()):])
    # the file is the header, each sub-batch framed by itself, the EOF block
    chunks = [al.map_bam(reads[a:a + 64], names=names[a:a + 64], quals=quals[a:a + 64], cs=True, where=_ffi.PAF_HOST) for a in range(0, len(reads), 64)]
    assert b"".join(_bam.inflate(c) for c in chunks) == b"".join(want)
    whole = al.bam_header() + b"".join(chunks) + mappy_rs.BAM_EOF
    out = str(tmp_path / "out.bam")
    open(out, "wb").write(b"what was here before\n")
    for where, n_dev in ((_ffi.PAF_DEVICE, 3), (_ffi.PAF_HOST, 0), (_ffi.PAF_AUTO, None)):
        res = al.map_bam_file(fq, out, cs=True, sub_batch_reads=64, where=where)
        got = open(out, "rb").read()
        assert got == whole, (where, len(got), len(whole))
        assert res["n_sub_batches"] == 3 and (n_dev is None or res["n_on_device"] == n_dev) and not os.path.exists(out + ".part")
        assert (res["n_reads"], res["n_lines"]) == (len(reads), len(want))
    assert got[-28:] == _bam.EOF and gzip.decompress(got) == _header_payload(al) + b"".join(want)
    # a FASTA input: 0xFF qualities; soft clipping and hit-only reach the records
    al.map_bam_file(fa, out, cs=True, sub_batch_reads=64, where=_ffi.PAF_DEVICE, softclip=True, hit_only=True)
    want_fa = _records_of_sam(al, al.map_sam(reads, names=names, cs=True, softclip=True, hit_only=True, where=_ffi.PAF_HOST))
    got = open(out, "rb").read()
    assert gzip.decompress(got) == _header_payload(al) + b"".join(want_fa) and got[-28:] == _bam.EOF and len(want_fa) < len(want)
    # a reads file cut in the middle leaves no file, and leaves the previous one in place
    cut = str(tmp_path / "cut.fq.gz")
    blob = open(fq, "rb").read()
    open(cut, "wb").write(blob[:len(blob) // 2])
    out3 = str(tmp_path / "out3.bam")
    for target in (out3, out):
        with pytest.raises(RuntimeError):
            al.map_bam_file(cut, target, cs=True, sub_batch_reads=16)
        assert not os.path.exists(target + ".part")
    assert not os.path.exists(out3) and open(out, "rb").read() == got
    # map_file writes what it wrote before the BAM calls
    al.map_file(fq, sam, cs=True, sub_batch_reads=64, format="sam")
    al.map_file(fq, paf, cs=True, sub_batch_reads=64)
    assert open(sam, "rb").read() == sam_before and open(paf, "rb").read() == paf_before
    with pytest.raises(ValueError):
        al.map_file(fq, sam, cs=True, format="bam")


def test_bam_header_of_many_contigs(built, tmp_path):
    """6000 contigs: the header takes several blocks"""
    import mappy_rs
    fa = str(tmp_path / "many.fa")
    names = ["contig%04d" % i for i in range(6000)]
    S.write_fasta(fa, S.make_genome(6, [48] * 6000), names)
    al = mappy_rs.Aligner(fa, preset="map-ont")
    hd = al.bam_header()
    payload = _bam.inflate(hd)
    assert payload == _header_payload(al) and len(payload) > 3 * P and hd == _bam.frame(payload)


def test_a_bam_request_changes_nothing_else(world):
    """mm355_map_batch_named's raw hits, CIGAR words and string bytes are the same before and after mm355_map_batch_bam calls on the context"""
    import mappy_rs
    from mappy_rs import _ffi
    al = mappy_rs.Aligner(world["fa"], preset="map-ont")
    reads, names, quals = _sam_reads(world, n_plain=40)

    def raw():
        v = _capi.map_raw(al, reads, OUT_CS | OUT_TAGS, names, entry="named")
        return _capi.raw(v.hits), _capi.raw(v.tags), v.cigar.tobytes(), v.str, v.off.tobytes(), v.status.tobytes()
    before = raw()
    for where in (_ffi.PAF_DEVICE, _ffi.PAF_HOST):
        assert len(_bam.split(al.map_bam(reads, names=names, quals=quals, cs=True, where=where, hit_only=True))) == len(before[0]) // _ffi._HIT_DTYPE.itemsize
        assert raw() == before
