"""The SAM writer on the GPU (mm355_recdev.h with SamFmt: k_rec_len, the scans, k_rec_fields; mm355_sam.hip: k_sam_copy): the device formatter against the host formatter
and mappy_rs.sam_lines, byte for byte -- on constructed result sets (tests/_sam_sets.py), end to end through Aligner.map_sam on the
two-contig world of tests/test_gpu_tags.py, and from a reads file to a SAM file through Aligner.map_file.  CPU side: tests/test_sam_host.py."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import synthdata as S
import _capi
import _paf_sets as PS
import _sam_sets as SS
from test_gpu_tags import world, _rc          # noqa: F401  (the fixture: its genome and reads)

OUT_CS, OUT_MD, OUT_TAGS = 1, 2, 4
T = SS.TILE


def _format(al, s, where, mo=None, sam_flags=None, raw=False):
    """mm355_sam_format on the set -> (text, line_off, on_device), or the return code alone"""
    from mappy_rs import _ffi
    L = al._L
    h, qn, sp, ql, qp, rl, keep = s if raw else SS.sam_args(s)
    tp = C.POINTER(_ffi.Text)()
    fl = sam_flags if sam_flags is not None else 0 if raw else s["sam_flags"]
    rc = L.mm355_sam_format(al._context(), C.byref(mo or al._mo), C.byref(h), qn, sp, ql, qp, rl, fl, where, C.byref(tp))
    if raw:
        assert not tp or rc == 0
        if tp:
            L.mm355_free_text(tp)
        return rc
    _ffi.check(rc)
    try:
        t = tp.contents
        assert t.n_reads == len(s["seqs"]) and t.ms_format >= 0.0
        text = bytes(_ffi.text_view(tp))
        assert t.n_lines == text.count(b"\n")
        return text, [t.line_off[i] for i in range(t.n_reads + 1)], t.on_device
    finally:
        L.mm355_free_text(tp)


@pytest.fixture(scope="module")
def stage(built, tmp_path_factory):
    """an Aligner whose index has the contig names of the constructed sets (names of 1 and 255 bytes)"""
    import mappy_rs
    fa = str(tmp_path_factory.mktemp("gsam") / "three.fa")
    S.write_fasta(fa, S.make_genome(5, [3000, 3000, 3000]), SS.CONTIGS)
    al = mappy_rs.Aligner(fa, preset="map-ont")
    assert al.seq_names == SS.CONTIGS
    return al


def _row(qs, qe, strand, kind, cigar, n_cigar=1, rid=0, ts=100):
    """a row over read[qs:qe]: kind 0 the primary with sam_pri, 1 a supplementary, 2 a secondary; its CIGAR words are appended to `cigar`"""
    r = dict(query_start=qs, query_end=qe, strand=strand, rid=rid, target_len=3000, target_start=ts, target_end=ts + (qe - qs), match_len=qe - qs,
             block_len=max(1, qe - qs), mapq=60, is_primary=int(kind != 2), n_cigar=n_cigar, cigar_off=len(cigar))
    cigar += [max(1, qe - qs) << 4] + [3 << 4 | 7] * (n_cigar - 1)
    return r, dict(score=qe - qs, flags=2 if kind == 0 else 0)


def _alignment_sets(rng):
    """SEQ / QUAL runs at source and destination residues mod 16 that move independently of each other: 16 reads per set, the name (and so
    the destination) `d` bytes long and the slice start at base `q`; per length one set where both grow from read to read, one where only
    the name grows and one where only the slice start moves (another fixed value per length), with a CIGAR of a few operations in front of
    the run; lengths around the wave and around the copy tile.  Per read: the whole read forwards, a reverse-strand and a forward
    hard-clipped slice of the length."""
    out = []
    for k, ln in enumerate((63, 64, 65, T - 1, T, T + 1, 2 * T + 1)):
        fixed = 1 + (5 * k) % 16
        for walk in (lambda a: (a + 1, a), lambda a: (a + 1, fixed), lambda a: (fixed, a)):
            rows, tags, cigar, hit_off, names, seqs, quals = [], [], [], [0], [], [], []
            for a in range(16):
                d, q = walk(a)
                seq, qual = SS.random_read(rng, ln + 40 + a)
                for r, t in (_row(0, len(seq), 1, 0, cigar), _row(q, q + ln, -1, 1, cigar, a % 5 + 1, 1), _row(q + 3, q + 3 + ln, 1, 1, cigar, 1, 2)):
                    rows.append(r); tags.append(t)
                hit_off.append(len(rows)); names.append("n" * d); seqs.append(seq); quals.append(qual if a % 3 else None)
            out.append(SS.make_set(rows, tags, hit_off, [0] * 16, names, seqs, quals, [0] * 16, 0, cigar=cigar))
    return out


def _special_sets(rng):
    cigar = []
    seq, qual = SS.random_read(rng, 200003)
    rows = [_row(0, 150000, 1, 0, cigar), _row(150001, 200002, -1, 1, cigar, 5, 1)]          # a long read with a reverse-strand hard-clipped supplementary
    long_read = SS.make_set([r for r, _ in rows], [t for _, t in rows], [0, 2], [0], ["long"], [seq], [qual], [0], 0, cigar=cigar)
    no_lines = SS.make_set([], [], [0, 0, 0], [0, SS.EEMPTY], ["a", None], ["ACGT", ""], [None, None], [3, 0], SS.HIT_ONLY)
    cigar = []
    seq, qual = SS.random_read(rng, 900)
    rows = [_row(100 * k, 100 * k + 90, 1 if k % 2 else -1, 0 if k == 0 else 1, cigar, 2, k % 3, 1000 * k) for k in range(9)]
    many_sa = SS.make_set([r for r, _ in rows], [t for _, t in rows], [0, 9], [0], ["chimera"], [seq], [qual], [0], 0, cigar=cigar)
    return long_read, no_lines, many_sa


def test_device_formatter_equals_host_and_python(stage, monkeypatch):
    from mappy_rs import _ffi
    al = stage
    rng = np.random.default_rng(11)
    long_read, no_lines, many_sa = _special_sets(rng)
    sets = SS.random_sets(356, 300) + _alignment_sets(rng) + [long_read, no_lines, many_sa]
    n_lines = 0
    for k, s in enumerate(sets):
        want, want_off = SS.expected(s)
        host, host_off, on = _format(al, s, _ffi.PAF_HOST)
        assert on == 0 and host == want and host_off == want_off, k
        dev, dev_off, on = _format(al, s, _ffi.PAF_DEVICE)
        assert on == 1, k
        if dev != want:
            at = next(i for i, (x, y) in enumerate(zip(dev, want)) if x != y) if len(dev) == len(want) else -1
            assert False, (k, len(dev), len(want), at, dev[max(0, at - 60):at + 60], want[max(0, at - 60):at + 60])
        assert dev_off == want_off, k
        n_lines += want.count(b"\n")
    assert n_lines > 1000
    sa = next(f for f in SS.expected(many_sa)[0].split(b"\n")[0].split(b"\t") if f.startswith(b"SA:Z:"))
    assert SS.expected(no_lines)[0] == b"" and sa.count(b";") == 8 > 4      # more SA entries than the run table has places
    w = SS.expected(long_read)[0].split(b"\n")
    assert w[1].split(b"\t")[1] == b"2064" and len(w[1].split(b"\t")[9]) == 50001 and b"150001H" in w[1].split(b"\t")[5]
    # MM355_PAF_AUTO: the hit count against MM355_SAM_MIN_HITS
    monkeypatch.setenv("MM355_SAM_MIN_HITS", "1")
    assert _format(al, many_sa, _ffi.PAF_AUTO)[2] == 1
    monkeypatch.setenv("MM355_SAM_MIN_HITS", "10")
    assert _format(al, many_sa, _ffi.PAF_AUTO)[2] == 0
    monkeypatch.setenv("MM355_SAM_MIN_HITS", "9")
    assert _format(al, many_sa, _ffi.PAF_AUTO)[2] == 1


def test_format_refuses_what_the_check_refuses(stage):
    """MM355_EINVAL from both formatters, nothing allocated or launched: no tags array, a row past its arena, a contig that does not exist, a
    row outside the read, rows on an empty read, a read without bytes, unknown sam_flags, an option record without MM_F_CIGAR"""
    from mappy_rs import _ffi
    al = stage
    s = next(s for s in SS.random_sets(8, 400) if len(s["hits"]) > 1 and len(s["cigar"]) > 2 and s["hit_off"][1] > 0 and len(s["seqs"]) > 1)
    mo_chain = _ffi.MapOpt.from_buffer_copy(al._mo)
    mo_chain.flag &= ~4
    for where in (_ffi.PAF_HOST, _ffi.PAF_DEVICE):
        assert _format(al, SS.sam_args(s), where, raw=True, sam_flags=s["sam_flags"]) == 0
        for broken in ("tags", "cigar", "rid", "qs", "qe", "empty", "seq", "flags", "mo"):
            args = list(SS.sam_args(s))
            h, mo, fl = args[0], None, s["sam_flags"]
            if broken == "tags":
                h.tags = None
            elif broken == "cigar":
                h.n_cigar -= 1
            elif broken == "rid":
                h.hits[0].rid = len(SS.CONTIGS)
            elif broken == "qs":
                h.hits[0].query_start = h.hits[0].query_end + 1
            elif broken == "qe":
                h.hits[0].query_end = len(s["seqs"][0]) + 1
            elif broken == "empty":
                h.status[0] = SS.EEMPTY
            elif broken == "seq":
                args[2][0] = None
            elif broken == "flags":
                fl = 4
            else:
                mo = mo_chain
            assert _format(al, tuple(args), where, mo=mo, raw=True, sam_flags=fl) == _ffi.MM355_EINVAL, (where, broken)


# ---------------------------------------------------------------- end to end
def _sam_reads(world, n_plain=90):
    """inversion reads, ordinary reads (the CPU oracle gives reads 74 and 89 of them forward and reverse secondaries under map-ont, and
    read 89 under map-hifi too), chimeric reads of two loci of the two contigs (the second half reverse-complemented in three of
    four: the CPU oracle gives them a primary and a supplementary, strands + / - and + / +), two random reads, one empty string"""
    g = world["g"]
    rng = np.random.default_rng(2026)
    chim = []
    for a, b, rc2 in ((200000, 100000, True), (500000, 400000, True), (900000, 700000, False), (1200000, 50000, True)):
        x = S.mutate(g[0][a:a + 3000], rng, 0.004, 0.003, 0.003)
        y = S.mutate(g[1][b:b + 2500], rng, 0.004, 0.003, 0.003)
        chim.append(S.codes_to_str(np.concatenate([x, _rc(y) if rc2 else y])))
    junk = [S.codes_to_str(S.random_codes(rng, n)) for n in (1500, 700)]
    reads = world["cigar_reads"][True][:12] + world["reads"][:n_plain] + chim + junk + [""]
    names = [None if i % 7 == 3 else "read%d comment %d" % (i, i) if i % 5 == 0 else "read%d" % i for i in range(len(reads))]
    quals = [None if i % 4 == 1 else "".join(chr(33 + (i + j) % 60) for j in range(len(r))) for i, r in enumerate(reads)]
    return reads, names, quals


def _expected_sam(al, recs, reads, names, quals, rl, softclip=False, hit_only=False):
    import mappy_rs
    out = []
    for i, ms in enumerate(recs):
        if isinstance(ms, list) and (ms or (reads[i] and not hit_only)):
            out += [ln + "\n" for ln in mappy_rs.sam_lines(ms, names[i] if names else None, reads[i], quals[i] if quals else None, softclip=softclip, rl=rl.get(i))]
    return "".join(out).encode()


def _rep_len_of_unmapped(al, recs, reads):
    idx = [i for i, ms in enumerate(recs) if isinstance(ms, list) and not ms]
    sr = al._stage_runner()
    try:
        rep = sr.anchors([reads[i] for i in idx])[1] if idx else []
    finally:
        sr.close()
    return {i: int(r) for i, r in zip(idx, rep)}


def _flags_of(text):
    return {int(ln.split(b"\t")[1]) for ln in text.split(b"\n") if ln}


@pytest.mark.parametrize("preset,kw,flags", [("map-ont", dict(cs=True), OUT_CS), ("map-ont", dict(MD=True), OUT_MD), ("map-hifi", {}, 0)],
                         ids=["map-ont-cs", "map-ont-MD", "map-hifi"])
def test_map_sam(world, preset, kw, flags):
    import mappy_rs
    from mappy_rs import _ffi
    al = mappy_rs.Aligner(world["fa"], preset=preset)
    reads, names, quals = _sam_reads(world)
    recs = al._map_many(reads, flags | OUT_TAGS, names=names)
    rl = _rep_len_of_unmapped(al, recs, reads)
    want = _expected_sam(al, recs, reads, names, quals, rl)
    fl = _flags_of(want)
    assert {2048, 2064, 256, 4} <= fl and b"\tSA:Z:" in want
    assert (b"\tcs:Z:" in want) == bool(flags & OUT_CS) and (b"\tMD:Z:" in want) == bool(flags & OUT_MD)
    cases = [(dict(quals=quals), want),
             (dict(quals=None, softclip=True), _expected_sam(al, recs, reads, names, None, rl, softclip=True)),
             (dict(quals=quals, hit_only=True), _expected_sam(al, recs, reads, names, quals, rl, hit_only=True))]
    assert 4 not in _flags_of(cases[2][1]) and b"H" not in b"".join(ln.split(b"\t")[5] for ln in cases[1][1].split(b"\n") if ln)
    for more, w in cases:
        for where, on in ((_ffi.PAF_HOST, False), (_ffi.PAF_DEVICE, True)):
            got = al.map_sam(reads, names=names, where=where, **kw, **more)
            assert al.paf_on_device is on
            assert got == w, (more.keys(), where, len(got), len(w))
    if preset == "map-hifi":
        with pytest.raises(ValueError):
            al.map_sam(reads[:2], quals=["II"])
        with pytest.raises(ValueError):
            al.map_sam(reads[:2], quals=["I", None])
        with pytest.raises(TypeError):
            al.map_sam([b"ACGT"])
        with pytest.raises(ValueError):
            mappy_rs.Aligner(world["fa"], preset="map-ont", cigar=False).map_sam(reads[:2])
        hd = al.sam_header()
        assert hd == (b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n@SQ\tSN:chrA\tLN:%d\n@SQ\tSN:chrB\tLN:%d\n@PG\tID:mappy_rs\tPN:mappy_rs\n"
                      % (len(world["g"][0]), len(world["g"][1])))


def _write_fastq_gz(path, reads, names, quals):
    with gzip.open(path, "wt") as f:
        for n, r, q in zip(names, reads, quals):
            f.write("@%s ch=%d start_time=x\n%s\n+\n%s\n" % (n, len(r) % 512, r, q))


def test_map_file_sam(world, tmp_path):
    """reads file in, SAM file out: the header, then the lines in input order across three workers and sub-batches of 64 reads"""
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
    recs = al._map_many(reads, OUT_CS | OUT_TAGS, names=names)
    rl = _rep_len_of_unmapped(al, recs, reads)
    want = al.sam_header() + _expected_sam(al, recs, reads, names, quals, rl)
    assert want.startswith(b"@HD\t") and {2048, 2064, 4} <= _flags_of(want[len(al.sam_header()):])
    al.enable_threading(3)
    out = str(tmp_path / "out.sam")
    open(out, "wb").write(b"what was here before\n")
    res = al.map_file(fq, out, cs=True, sub_batch_reads=64, where=_ffi.PAF_DEVICE, format="sam")
    got = open(out, "rb").read()
    assert got == want, (len(got), len(want))
    assert res["n_on_device"] == res["n_sub_batches"] == 3 and not os.path.exists(out + ".part")
    assert (res["n_reads"], res["n_lines"]) == (len(reads), want.count(b"\n") - 4)
    res = al.map_file(fq, out, cs=True, sub_batch_reads=64, where=_ffi.PAF_HOST, format="sam")
    assert open(out, "rb").read() == want and res["n_on_device"] == 0
    al.map_file(fq, out, cs=True, sub_batch_reads=64, format="sam")          # AUTO
    assert open(out, "rb").read() == want
    # a FASTA input: `*` qualities
    al.map_file(fa, out, cs=True, sub_batch_reads=64, where=_ffi.PAF_DEVICE, format="sam")
    assert open(out, "rb").read() == al.sam_header() + _expected_sam(al, recs, reads, names, None, rl)
    # any other format: ValueError, out_path untouched
    with pytest.raises(ValueError):
        al.map_file(fq, out, cs=True, format="bam")
    assert open(out, "rb").read() == al.sam_header() + _expected_sam(al, recs, reads, names, None, rl) and not os.path.exists(out + ".part")
    # a reads file cut in the middle leaves no file
    cut = str(tmp_path / "cut.fq.gz")
    blob = open(fq, "rb").read()
    open(cut, "wb").write(blob[:len(blob) // 2])
    out3 = str(tmp_path / "out3.sam")
    with pytest.raises(RuntimeError):
        al.map_file(cut, out3, cs=True, sub_batch_reads=16, format="sam")
    assert not os.path.exists(out3) and not os.path.exists(out3 + ".part")
    # format="paf" is the call without format=
    p1, p2 = str(tmp_path / "a.paf"), str(tmp_path / "b.paf")
    al.map_file(fq, p1, cs=True, sub_batch_reads=64, where=_ffi.PAF_DEVICE)
    al.map_file(fq, p2, cs=True, sub_batch_reads=64, where=_ffi.PAF_DEVICE, format="paf")
    paf = "".join(mappy_rs.paf_line(m, n, len(r)) + "\n" for n, r, ms in zip(names, reads, recs) for m in ms).encode()
    assert open(p1, "rb").read() == open(p2, "rb").read() == paf


def test_a_sam_request_changes_nothing_else(world):
    """mm355_map_batch_named's raw hits, CIGAR words and string bytes are the same before and after mm355_map_batch_sam calls on the context"""
    import mappy_rs
    from mappy_rs import _ffi
    al = mappy_rs.Aligner(world["fa"], preset="map-ont")
    reads, names, quals = _sam_reads(world, n_plain=40)

    def raw():
        v = _capi.map_raw(al, reads, OUT_CS | OUT_TAGS, names, entry="named")
        return _capi.raw(v.hits), _capi.raw(v.tags), v.cigar.tobytes(), v.str, v.off.tobytes(), v.status.tobytes()
    before = raw()
    for where in (_ffi.PAF_DEVICE, _ffi.PAF_HOST):
        assert al.map_sam(reads, names=names, quals=quals, cs=True, where=where, hit_only=True).count(b"\n") == len(before[0]) // _ffi._HIT_DTYPE.itemsize
        assert raw() == before
