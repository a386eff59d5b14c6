"""Copied aux tags on the GPU (mm355_recdev.h with BamFmt's third tile run; mm355_bam.hip: k_bam_bulk mode 5): the device formatter against
the host formatter and the model of tests/_bamaux.py on constructed result sets, at level 0 and level 1; the calls with aux == NULL against
the calls without the argument; and from a BAM with tags to a BAM with tags through Aligner.map_bam_file with both readers.
CPU side: tests/test_bamaux_host.py."""
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
import _bamaux as A
import _inflate as I
import _sam_sets as SS
from test_gpu_tags import world, _rc          # noqa: F401  (the fixture: its genome and reads)
from test_gpu_sam import _sam_reads
from test_bamaux_host import _auxes, _row

EINVAL = -2


@pytest.fixture(scope="module")
def stage(built, tmp_path_factory):
    """an Aligner whose index has the contig names of the constructed sets"""
    import mappy_rs
    fa = str(tmp_path_factory.mktemp("gbamaux") / "three.fa")
    S.write_fasta(fa, S.make_genome(5, [3000, 3000, 3000]), SS.CONTIGS)
    al = mappy_rs.Aligner(fa, preset="map-ont")
    assert al.seq_names == SS.CONTIGS
    return al


def _format(al, s, auxes, where, level=0, raw=False, arrays=None):
    """mm355_bam_format_aux on the set -> (BGZF bytes, line_off, on_device, n_lines), or the return code alone; auxes None: aux == NULL"""
    from mappy_rs import _ffi
    L = al._L
    h, qn, sp, ql, qp, rl, keep = SS.sam_args(s)
    ptr, ln, md, bufs = arrays if arrays else A.aux_arrays(auxes) if auxes is not None else (None, None, None, None)
    tp = C.POINTER(_ffi.Text)()
    rc = L.mm355_bam_format_aux(al._context(), C.byref(al._mo), C.byref(h), qn, sp, ql, qp, rl, ptr, ln, md, s["sam_flags"], where, level, C.byref(tp))
    if raw:
        assert not tp or rc == 0
        if tp:
            L.mm355_free_text(tp)
        return rc
    _ffi.check(rc)
    try:
        t = tp.contents
        return bytes(_ffi.text_view(tp)), [t.line_off[i] for i in range(t.n_reads + 1)], t.on_device, t.n_lines
    finally:
        L.mm355_free_text(tp)


def _residue_sets(rng):
    """per tag length of A.LENGTHS a set of 17 reads whose names are 1 .. 17 bytes long: the records, and so the tags' destination, start at
    every residue mod 16, while the blocks lie back to back behind reads of 50 .. 66 bases in the upload: source and destination move
    independently.  Per read a forward primary, a reverse hard-clipped supplementary and a secondary (both get the first group only);
    every fourth read has no hits (the unmapped record: all tags), every third no quality"""
    out = []
    for k, n in enumerate(A.LENGTHS):
        rows, tags, cigar, hit_off, names, seqs, quals, auxes = [], [], [], [0], [], [], [], []
        for d in range(1, 18):
            seq, qual = SS.random_read(rng, 49 + d)
            if d % 4:
                for r, t in (_row(0, len(seq), 1, 0, cigar), _row(3, 30 + d, -1, 1, cigar, d % 3 + 1, 1), _row(5, 40, 1, 2, cigar, 1, 2)):
                    rows.append(r); tags.append(t)
            hit_off.append(len(rows)); names.append("n" * d); seqs.append(seq); quals.append(qual if d % 3 else None)
            auxes.append(A.two_groups(n, rng, first=(4 if d % 2 else n - 8 - d) if n > 4000 else None))
        out.append((BS.scrub(SS.make_set(rows, tags, hit_off, [0] * 17, names, seqs, quals, [d for d in range(17)], k % 2, cigar=cigar), rng), auxes))
    return out


def _first_difference(dev, want):
    got = _bam.cut(gzip.decompress(dev)) if dev else []
    bad = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), -1)
    at = next((i for i, (a, b) in enumerate(zip(got[bad], want[bad])) if a != b), -1) if bad >= 0 else -1
    return (len(got), len(want), bad, at, got[bad][max(0, at - 24):at + 24].hex() if bad >= 0 else "", want[bad][max(0, at - 24):at + 24].hex() if bad >= 0 else "")


def test_device_equals_host_with_tags(stage):
    from mappy_rs import _ffi
    al = stage
    rng = np.random.default_rng(21)
    cases = _residue_sets(rng)
    cases += [(s, _auxes(s, rng, k)) for k, s in enumerate(BS.random_sets(358, 120))]
    # tags, empty tags and no tags side by side, a read without records (MM355_EEMPTY) and an unmapped one between them
    cigar = []
    reads = [SS.random_read(rng, n) for n in (70, 33, 90, 41)]
    rows = [_row(0, 70, 1, 0, cigar), _row(10, 60, -1, 1, cigar, 2, 1), _row(0, 90, -1, 0, cigar)]
    mixed = BS.scrub(SS.make_set([r for r, _ in rows], [t for _, t in rows], [0, 2, 2, 2, 3, 3], [0, 0, SS.EEMPTY, 0, 0], ["a", "bb", None, "dddd", "e"],
                                 [reads[0][0], reads[1][0], "", reads[2][0], reads[3][0]], [reads[0][1], None, None, reads[2][1], reads[3][1]], [0, 9, 0, 0, 3], 0, cigar=cigar), rng)
    cases.append((mixed, [A.two_groups(4097, rng), (b"", 0), A.two_groups(17, rng), None, A.two_groups(16, rng, first=0)]))
    # the long-CIGAR record: CG stays last
    cases += [(BS.long_cigar_set(65536, rng, st), [A.two_groups(n, rng)]) for st, n in ((1, 4097), (-1, 15))]
    n_rec = 0
    for k, (s, ax) in enumerate(cases):
        want, want_off = A.expected(s, ax)
        framed = _bam.frame(b"".join(want))
        host, host_off, on, nl = _format(al, s, ax, _ffi.PAF_HOST)
        assert on == 0 and host == framed and host_off == want_off and nl == len(want), k
        dev, dev_off, on, nl = _format(al, s, ax, _ffi.PAF_DEVICE)
        assert on == 1 and nl == len(want), k
        assert dev == framed, (k,) + _first_difference(dev, want)
        assert dev_off == want_off, k
        host1, off1, _, _ = _format(al, s, ax, _ffi.PAF_HOST, level=1)
        dev1, doff1, on, _ = _format(al, s, ax, _ffi.PAF_DEVICE, level=1)
        assert on == 1 and dev1 == host1 and doff1 == off1 == want_off and (gzip.decompress(dev1) if dev1 else b"") == b"".join(want), k
        n_rec += len(want)
    assert n_rec > 600
    (s, ax) = cases[-3]
    recs = A.expected(s, ax)[0]
    plain = BS.expected(s)[0]
    assert [len(r) - len(p) for r, p in zip(recs, plain)] == [4097, len(ax[0][0][:ax[0][1]]), 0, 0, 16]   # all, the first group, empty, absent, all (unmapped)
    s, ax = cases[-2]
    r, = A.expected(s, ax)[0]
    at = r.find(b"CGBI" + struct.pack("<I", 65536))
    assert at > 0 and len(r) - at == 8 + 4 * 65536 and r[at - 4097:at] == ax[0][0]


def test_null_aux_is_the_call_without_it(stage, world):
    """mm355_bam_format_aux and mm355_map_batch_bam_aux with aux == NULL against the four calls that have no such argument: the same bytes;
    so are tags that are absent or empty on every read"""
    from mappy_rs import _ffi
    from test_gpu_bam import _format as _old_format
    import mappy_rs
    al = stage
    for s in BS.random_sets(359, 40):
        for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
            old = _old_format(al, s, where)
            assert _format(al, s, None, where) == old
            assert _format(al, s, [None] * len(s["seqs"]), where) == old and _format(al, s, [(b"", 0)] * len(s["seqs"]), where) == old
    al = mappy_rs.Aligner(world["fa"], preset="map-ont")
    reads, names, quals = _sam_reads(world, n_plain=20)
    L = al._L
    for level in (0, 1):
        for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
            old = al.map_bam(reads, names=names, quals=quals, cs=True, where=where, compress=bool(level))
            new = al._map_records(reads, names, quals, al._sam_flags(True, False), 0, where, mappy_rs._Entry(L.mm355_map_batch_bam_aux, True, True, (level,), _ffi.Text))
            assert new == old and len(old) > 1000
            assert al.map_bam(reads, names=names, quals=quals, cs=True, where=where, compress=bool(level), aux=[None] * len(reads)) == old


def test_refused_call_then_a_valid_one(stage):
    from mappy_rs import _ffi
    al = stage
    rng = np.random.default_rng(23)
    s, ax = _residue_sets(rng)[4]
    want = _bam.frame(b"".join(A.expected(s, ax)[0]))
    for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
        ptr, ln, md, bufs = A.aux_arrays(ax)
        for break_it in ("len", "mod", "mod_neg", "null"):
            p2, l2, m2, _ = A.aux_arrays(ax)
            if break_it == "len": l2[3] = -1
            if break_it == "mod": m2[3] = l2[3] + 1
            if break_it == "mod_neg": m2[0] = -1
            if break_it == "null": p2[5] = None
            assert _format(al, s, ax, where, raw=True, arrays=(p2, l2, m2, None)) == EINVAL, (where, break_it)
            assert _format(al, s, ax, where)[0] == want, (where, break_it)
        # aux without its lengths
        assert _format(al, s, ax, where, raw=True, arrays=(ptr, None, md, bufs)) == EINVAL and _format(al, s, ax, where, raw=True, arrays=(ptr, ln, None, bufs)) == EINVAL
        assert _format(al, s, ax, where)[0] == want


# ---------------------------------------------------------------- end to end: a BAM with tags in, a BAM with tags out
def _tagged_bam(reads, names, quals, rng, bad=None):
    """an unaligned BAM of the reads as a basecaller writes it (MM / ML of about half a byte per base each, RG, qs, mv, a stale NM); one
    record in five stored on the reverse strand, as an aligner's BAM would; bad: the index of a record whose aux is cut inside a tag"""
    body, auxes = b"", []
    for i, (r, n, q) in enumerate(zip(reads, names, quals)):
        aux = A.tag("RG", "Z", b"run1") + A.tag("qs", "f", 11.0 + i) + A.mod_pair(len(r), rng) + A.tag("NM", "C", 7) + A.tag("mv", "B", ("c", rng.integers(0, 2, 10 + i).tolist())) + \
            A.tag("MN", "i", len(r))
        if i % 6 == 5:
            aux = b""
        auxes.append(aux)
        body += I.bam_record(n.encode(), r.encode(), q.encode(), flag=0x10 if i % 5 == 2 else 4, aux=aux[:-3] if i == bad else aux)
    return I.bam_header(b"@HD\tVN:1.6\tSO:unknown\n@RG\tID:run1\tPL:ONT\n@PG\tID:basecaller\n") + body, auxes


def _file_records(path):
    """the file's header text and its records by read name"""
    data = gzip.decompress(open(path, "rb").read())
    l_text, = struct.unpack_from("<I", data, 4)
    text = data[8:8 + l_text]
    at = 8 + l_text
    n_ref, = struct.unpack_from("<I", data, at)
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<I", data, at)[0]
    recs = _bam.cut(data[at:])
    return text, recs


def test_map_bam_file_copies_tags(world, tmp_path):
    import mappy_rs
    from mappy_rs import _ffi
    rng = np.random.default_rng(29)
    all_reads, _, _ = _sam_reads(world, n_plain=90)
    reads = all_reads[-7:-1] + all_reads[80:100]                              # chimeric reads (supplementaries), random ones (unmapped), ordinary ones
    reads = [r.replace("N", "A") for r in reads]
    names = ["r%03d" % i for i in range(len(reads))]
    quals = ["".join(chr(35 + (i + j) % 50) for j in range(len(r))) for i, r in enumerate(reads)]
    blob, auxes = _tagged_bam(reads, names, quals, rng)
    bam, fq = str(tmp_path / "calls.bam"), str(tmp_path / "calls.fq")
    open(bam, "wb").write(I.bgzf_file(blob, 0xff00))
    open(fq, "w").write("".join("@%s\n%s\n+\n%s\n" % t for t in zip(names, reads, quals)))
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", tags=True, devices=[0])
    al.enable_threading(2)
    out = str(tmp_path / "out.bam")
    # without the keyword: the file made from the FASTQ of the same reads, which no change to the tags' path can touch
    al.map_bam_file(fq, out, cs=True, sub_batch_reads=9)
    today = open(out, "rb").read()
    res0 = al.map_bam_file(bam, out, cs=True, sub_batch_reads=9)
    assert open(out, "rb").read() == today and "n_aux_bytes" not in res0
    assert al.map_bam_file(bam, out, cs=True, sub_batch_reads=9, copy_tags=False).keys() == res0.keys() and open(out, "rb").read() == today
    head0, plain = _file_records(out)
    flags = {struct.unpack_from("<H", r, 18)[0] & 0x904 for r in plain}
    assert {0, 0x800, 4} <= flags
    name_of = lambda r: r[36:36 + r[12] - 1].decode()
    for copy_tags, keep in ((True, "*"), (("MM", "ML"), "MMML"), (["RG", "MN"], "RGMN")):
        split = {n: A.split(a, keep) for n, a in zip(names, auxes)}
        want = [A.with_aux(r, A.aux_of_record(r, *split[name_of(r)], False)) for r in plain]
        variants = (dict(where=_ffi.PAF_DEVICE), dict(where=_ffi.PAF_HOST), dict(read_on_gpu=True), dict(compress=True, read_on_gpu=True, where=_ffi.PAF_DEVICE))
        for kw in variants if keep == "*" else variants[3:]:
            res = al.map_bam_file(bam, out, cs=True, sub_batch_reads=9, copy_tags=copy_tags, **kw)
            head, got = _file_records(out)
            assert got == want, (keep, kw, next(i for i, (a, b) in enumerate(zip(got, want)) if a != b))
            assert head == head0.replace(b"@PG\tID:mappy_rs", b"@RG\tID:run1\tPL:ONT\n@PG\tID:mappy_rs") and head.count(b"@RG") == 1
            assert res["n_aux_bytes"] == sum(len(v[0]) for v in split.values()) and res["n_lines"] == len(want) and res["n_reads"] == len(reads)
            assert res.get("reader_on_device", False) == bool(kw.get("read_on_gpu"))
            assert not os.path.exists(out + ".part")
    # (the last of them, RG and MN: a hard-clipped supplementary has RG and not MN, which counts the read's bases)
    sup = {w[len(r):] for r, w in zip(plain, want) if struct.unpack_from("<H", r, 18)[0] & 0x800}
    assert A.tag("RG", "Z", b"run1") in sup and sup <= {A.tag("RG", "Z", b"run1"), b""}
    # a reads file that is no BAM: the keyword copies nothing
    res = al.map_bam_file(fq, out, cs=True, sub_batch_reads=9, copy_tags=True)
    assert open(out, "rb").read() == today and res["n_aux_bytes"] == 0
    # a corrupt aux block in the third sub-batch: no file, no .part file, and the file that was there stays
    bad_blob, _ = _tagged_bam(reads, names, quals, rng, bad=20)
    open(bam, "wb").write(I.bgzf_file(bad_blob, 0xff00))
    out2 = str(tmp_path / "out2.bam")
    for target, kw in ((out2, {}), (out, dict(read_on_gpu=True))):
        with pytest.raises(RuntimeError):
            al.map_bam_file(bam, target, cs=True, sub_batch_reads=9, copy_tags=True, **kw)
        assert not os.path.exists(target + ".part")
    assert not os.path.exists(out2) and open(out, "rb").read() == today
    assert al.map_bam_file(bam, out2, cs=True, sub_batch_reads=9)["n_reads"] == len(reads)      # (skipped unseen when nothing is kept)
    for bad in ("MM", ["M"], 3, [b"MM"]):
        with pytest.raises(ValueError):
            al.map_bam_file(bam, out2, copy_tags=bad)


def test_map_bam_takes_tags(world):
    import mappy_rs
    from mappy_rs import _ffi
    rng = np.random.default_rng(31)
    al = mappy_rs.Aligner(world["fa"], preset="map-ont")
    all_reads, _, _ = _sam_reads(world, n_plain=90)
    reads = all_reads[-7:-3] + all_reads[20:28]
    names = ["q%d" % i for i in range(len(reads))]
    aux = [None if i % 4 == 3 else A.mod_pair(len(r), rng) + A.tag("RG", "Z", b"g") + A.tag("AS", "i", 5) for i, r in enumerate(reads)]
    plain = _bam.split(al.map_bam(reads, names=names, where=_ffi.PAF_HOST))
    split = {n: (None if a is None else A.split(a)) for n, a in zip(names, aux)}
    name_of = lambda r: r[36:36 + r[12] - 1].decode()
    want = [r if split[name_of(r)] is None else A.with_aux(r, A.aux_of_record(r, *split[name_of(r)], False)) for r in plain]
    for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
        assert _bam.split(al.map_bam(reads, names=names, where=where, aux=aux)) == want
        assert _bam.cut(gzip.decompress(al.map_bam(reads, names=names, where=where, aux=aux, compress=True))) == want
    with pytest.raises(ValueError, match=r"aux\[2\]"):
        al.map_bam(reads, names=names, aux=aux[:2] + [b"xxQ\0"] + aux[3:])
    for bad in (aux[:-1], ["x"] * len(reads)):
        with pytest.raises(ValueError):
            al.map_bam(reads, names=names, aux=bad)
