"""The host side of the SAM writer (mappy-rs_amd/csrc/mm355_sam.h, the quality-keeping reader of mm355_index.cpp), built with g++ under
AddressSanitizer and UBSan into a stand-alone program (tests/host_harness/sam_host.cpp): mappy_rs.sam_lines against hand-written lines --
the only independent pin of the layout --, the host formatter against sam_lines on about 2000 result sets (tests/_sam_sets.py), the
complement table, mm355_sam_check, the reader's qualities.  GPU side: tests/test_gpu_sam.py."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import _capi
import _paf_sets as PS
import _sam_sets as SS

EINVAL, EIO = -2, -4
TWO = ["chr1", "chr2"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sam_host") / "sam_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(_capi.HERE, "host_harness", "sam_host.cpp"), "-o", exe, "-lz", "-lpthread"])
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


# ---------------------------------------------------------------- sam_lines against literal lines
def _row(qs, qe, strand, rid, ts, te, mlen, blen, mapq, pri, NM, n_cigar, cigar_off, cnt, subsc, dp_max, dp_score, **kw):
    return dict(query_start=qs, query_end=qe, strand=strand, rid=rid, target_len=5000, target_start=ts, target_end=te, match_len=mlen, block_len=blen,
                mapq=mapq, is_primary=pri, NM=NM, n_cigar=n_cigar, cigar_off=cigar_off, cnt=cnt, subsc=subsc, dp_max=dp_max, dp_score=dp_score, **kw)


def _records(built, rows, tags, cigar, sbuf=b""):
    import mappy_rs
    s = PS.make_set(rows, tags, True, [0, len(rows)], [0], [0], ["x"], TWO, cigar=cigar, sbuf=sbuf)
    h, _, _, keep = PS.hits_struct(s)
    return mappy_rs._batch_to_mappings(C.pointer(h), 1, TWO)[0]


M, I, D = 0, 1, 2
READ20, QUAL20 = "AAAACCCCGGGGTTTTACGT", "abcdefghijklmnopqrst"
TAGS0 = "NM:i:0\tms:i:24\tAS:i:24\tnn:i:0\ttp:A:P\tcm:i:5\ts1:i:50\ts2:i:0\tde:f:0"
TAGS1 = "NM:i:1\tms:i:10\tAS:i:10\tnn:i:0\ttp:A:P\tcm:i:2\ts1:i:20\ts2:i:0\tde:f:0.1111"


def _pair(built, strand1=1, flags1=0, te0=1012):
    """a read of 20 bases with two primaries: bases 0-12 on chr1, bases 12-20 on chr2 (4M1D4M) without sam_pri"""
    rows = [_row(0, 12, 1, 0, 1000, te0, 12, 12, 60, 1, 0, 1, 0, 5, 0, 24, 24),
            _row(12, 20, strand1, 1, 500, 509, 8, 9, 30, 1, 1, 3, 1, 2, 0, 10, 10)]
    tags = [dict(score=50, flags=2), dict(score=20, n_gap=1, n_gapo=1, flags=flags1)]
    return _records(built, rows, tags, [12 << 4 | M, 4 << 4 | M, 1 << 4 | D, 4 << 4 | M])


def test_sam_lines_forward_primary_with_quality(built):
    import mappy_rs
    ms = _records(built, [_row(2, 9, 1, 0, 99, 106, 7, 7, 60, 1, 0, 1, 0, 3, 0, 14, 14)], [dict(score=40, rep_len=5, flags=2)], [7 << 4 | M])
    assert mappy_rs.sam_lines(ms, "r1 comment", "ACGTACGTAC", "ABCDEFGHIJ") == [
        "r1\t0\tchr1\t100\t60\t2S7M1S\t*\t0\t0\tACGTACGTAC\tABCDEFGHIJ\tNM:i:0\tms:i:14\tAS:i:14\tnn:i:0\ttp:A:P\tcm:i:3\ts1:i:40\ts2:i:0\tde:f:0\trl:i:5"]
    # without a quality string, and unnamed
    assert mappy_rs.sam_lines(ms, None, "ACGTACGTAC") == [
        "*\t0\tchr1\t100\t60\t2S7M1S\t*\t0\t0\tACGTACGTAC\t*\tNM:i:0\tms:i:14\tAS:i:14\tnn:i:0\ttp:A:P\tcm:i:3\ts1:i:40\ts2:i:0\tde:f:0\trl:i:5"]


def test_sam_lines_reverse_primary(built):
    """SEQ reverse-complemented with an N, a lower-case base and an R; QUAL reversed; the clips swap sides"""
    import mappy_rs
    ms = _records(built, [_row(1, 6, -1, 1, 0, 5, 4, 5, 7, 1, 1, 1, 0, 2, 11, 8, 6)], [dict(score=30, rep_len=0, flags=2)], [5 << 4 | M])
    assert mappy_rs.sam_lines(ms, "r2", "ACGNtRAC", "12345678") == [
        "r2\t16\tchr2\t1\t7\t2S5M1S\t*\t0\t0\tGTYaNCGT\t87654321\tNM:i:1\tms:i:8\tAS:i:6\tnn:i:0\ttp:A:P\tcm:i:2\ts1:i:30\ts2:i:11\tde:f:0.2000\trl:i:0"]


def test_sam_lines_secondary(built):
    """`*` for SEQ and QUAL, S clips, tp:A:S without s2; the primary names no secondary in an SA tag"""
    import mappy_rs
    rows = [_row(2, 9, 1, 0, 99, 106, 7, 7, 60, 1, 0, 1, 0, 3, 0, 14, 14), _row(3, 9, -1, 1, 10, 16, 6, 6, 0, 0, 0, 1, 1, 3, 0, 12, 12)]
    ms = _records(built, rows, [dict(score=40, flags=2), dict(score=33, flags=0)], [7 << 4 | M, 6 << 4 | M])
    got = mappy_rs.sam_lines(ms, "r1", "ACGTACGTAC", "ABCDEFGHIJ")
    assert got[0] == "r1\t0\tchr1\t100\t60\t2S7M1S\t*\t0\t0\tACGTACGTAC\tABCDEFGHIJ\tNM:i:0\tms:i:14\tAS:i:14\tnn:i:0\ttp:A:P\tcm:i:3\ts1:i:40\ts2:i:0\tde:f:0\trl:i:0"
    assert got[1] == "r1\t272\tchr2\t11\t0\t1S6M3S\t*\t0\t0\t*\t*\tNM:i:0\tms:i:12\tAS:i:12\tnn:i:0\ttp:A:S\tcm:i:3\ts1:i:33\tde:f:0\trl:i:0"
    # soft clipping prints the read on the secondary too, reverse-complemented
    assert mappy_rs.sam_lines(ms, "r1", "ACGTACGTAC", "ABCDEFGHIJ", softclip=True)[1].split("\t")[9:11] == ["GTACGTACGT", "JIHGFEDCBA"]


def test_sam_lines_supplementary_and_SA(built):
    import mappy_rs
    ms = _pair(built)
    assert mappy_rs.sam_lines(ms, "q", READ20, QUAL20) == [
        "q\t0\tchr1\t1001\t60\t12M8S\t*\t0\t0\t" + READ20 + "\t" + QUAL20 + "\t" + TAGS0 + "\tSA:Z:chr2,501,+,12S8M1D,30,1;\trl:i:0",
        "q\t2048\tchr2\t501\t30\t12H4M1D4M\t*\t0\t0\tTTTTACGT\tmnopqrst\t" + TAGS1 + "\tSA:Z:chr1,1001,+,12M8S,60,0;\trl:i:0"]
    assert mappy_rs.sam_lines(ms, "q", READ20, QUAL20, softclip=True) == [
        "q\t0\tchr1\t1001\t60\t12M8S\t*\t0\t0\t" + READ20 + "\t" + QUAL20 + "\t" + TAGS0 + "\tSA:Z:chr2,501,+,12S8M1D,30,1;\trl:i:0",
        "q\t2048\tchr2\t501\t30\t12S4M1D4M\t*\t0\t0\t" + READ20 + "\t" + QUAL20 + "\t" + TAGS1 + "\tSA:Z:chr1,1001,+,12M8S,60,0;\trl:i:0"]
    # a reverse-strand supplementary: the clip moves behind the CIGAR, the slice is reverse-complemented, SA says "-"
    ms = _pair(built, strand1=-1)
    assert mappy_rs.sam_lines(ms, "q", READ20, QUAL20) == [
        "q\t0\tchr1\t1001\t60\t12M8S\t*\t0\t0\t" + READ20 + "\t" + QUAL20 + "\t" + TAGS0 + "\tSA:Z:chr2,501,-,8M1D12S,30,1;\trl:i:0",
        "q\t2064\tchr2\t501\t30\t4M1D4M12H\t*\t0\t0\tACGTAAAA\ttsrqponm\t" + TAGS1 + "\tSA:Z:chr1,1001,+,12M8S,60,0;\trl:i:0"]
    # an inversion pair: the second record is tp:A:I
    ms = _pair(built, strand1=-1, flags1=1)
    assert mappy_rs.sam_lines(ms, "q", READ20)[1] == (
        "q\t2064\tchr2\t501\t30\t4M1D4M12H\t*\t0\t0\tACGTAAAA\t*\t" + TAGS1.replace("tp:A:P", "tp:A:I") + "\tSA:Z:chr1,1001,+,12M8S,60,0;\trl:i:0")
    # more query than target in the other record: l_I instead of l_D
    ms = _pair(built, te0=1010)
    assert mappy_rs.sam_lines(ms, "q", READ20)[1].split("\t")[-2] == "SA:Z:chr1,1001,+,10M2I8S,60,0;"


def test_sam_lines_unmapped_and_string_tags(built):
    import mappy_rs
    assert mappy_rs.sam_lines([], "u 1", "ACGTN", "!!#~I", rl=17) == ["u\t4\t*\t0\t0\t*\t*\t0\t0\tACGTN\t!!#~I\trl:i:17"]
    assert mappy_rs.sam_lines([], None, "acgt", rl=0) == ["*\t4\t*\t0\t0\t*\t*\t0\t0\tacgt\t*\trl:i:0"]
    with pytest.raises(ValueError):
        mappy_rs.sam_lines([], "u", "ACGT")
    # cs and MD stand behind the shared tags (and SA) and before rl
    row = _row(0, 4, 1, 0, 0, 4, 3, 4, 60, 1, 1, 1, 0, 1, 0, 4, 4, cs_off=0, cs_len=7, md_off=8, md_len=3)
    ms = _records(built, [row], [dict(score=9, rep_len=3, flags=2, n_ambi=0)], [4 << 4 | M], sbuf=b":2*ag:1\x002A1\x00\x00")
    assert mappy_rs.sam_lines(ms, "c", "ACGT")[0].endswith("\ts1:i:9\ts2:i:0\tde:f:0.2500\tcs:Z::2*ag:1\tMD:Z:2A1\trl:i:3")
    # records without tags, and chain-only records
    s = PS.make_set([row], [dict(flags=2)], True, [0, 1], [0], [4], ["x"], TWO, cigar=[4 << 4], sbuf=b":2*ag:1\x002A1\x00\x00")
    h, _, _, keep = PS.hits_struct(s)
    with pytest.raises(ValueError):
        mappy_rs.sam_lines(mappy_rs._batch_to_mappings(C.pointer(h), 1, TWO, chain_only=True)[0], "c", "ACGT")
    h.tags = None
    with pytest.raises(ValueError):
        mappy_rs.sam_lines(mappy_rs._batch_to_mappings(C.pointer(h), 1, TWO)[0], "c", "ACGT")


# ---------------------------------------------------------------- the host formatter against sam_lines
@pytest.fixture(scope="module")
def sets(built):
    return SS.random_sets(20261, 2000)


def test_generator_covers_the_cases(sets):
    hits = np.concatenate([s["hits"] for s in sets]); tags = np.concatenate([s["tags"] for s in sets])
    assert set(hits["strand"].tolist()) == {1, -1}
    kinds = set()
    for s in sets:
        for i in range(len(s["seqs"])):
            a, b = s["hit_off"][i], s["hit_off"][i + 1]
            kinds.add((int(b - a), tuple(sorted({0 if not h["is_primary"] else 1 if t["flags"] & 2 else 2 for h, t in zip(s["hits"][a:b], s["tags"][a:b])}))))
    assert {n for n, _ in kinds} == {0, 1, 2, 3, 4, 5} and {k for _, k in kinds} >= {(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)}
    assert any(s["status"][i] == SS.EEMPTY for s in sets for i in range(len(s["status"])))
    assert any(s["hit_off"][i] == s["hit_off"][i + 1] and s["status"][i] == 0 for s in sets for i in range(len(s["status"])))
    assert any(None in s["quals"] and any(q for q in s["quals"]) for s in sets)
    assert {s["sam_flags"] for s in sets} == {0, 1, 2, 3}
    assert set(PS.CIGAR_COUNTS) <= {int(s["hits"][0]["n_cigar"]) for s in sets if len(s["hits"])}
    assert set(SS.LENGTHS) <= {len(x) for s in sets for x in s["seqs"]} and {SS.TILE - 1, SS.TILE + 1} <= set(SS.LENGTHS)
    assert (hits["cs_len"] >= 0).any() and (hits["md_len"] >= 0).any() and (hits["target_start"] == 2**31 - 1).any()
    assert None in [q for s in sets for q in s["qnames"]]
    # rows are consistent with the read they sit on
    for s in sets:
        for i in range(len(s["seqs"])):
            for h in s["hits"][s["hit_off"][i]:s["hit_off"][i + 1]]:
                assert 0 <= h["query_start"] <= h["query_end"] <= len(s["seqs"][i]) and h["target_start"] <= h["target_end"]


def _split(got, sets):
    at = 0
    for s in sets:
        nr = len(s["seqs"])
        n_text, n_lines = np.frombuffer(got, np.int64, 2, at).tolist()
        line_off = np.frombuffer(got, np.int64, nr + 1, at + 16).tolist()
        text = got[at + 8 * (nr + 3):at + 8 * (nr + 3) + n_text]
        at += 8 * (nr + 3) + n_text
        yield text, line_off, n_lines
    assert at == len(got)


def test_host_formatter_equals_sam_lines(harness, sets, tmp_path):
    """the emitter run serially == the joined sam_lines over _batch_to_mappings of the same arrays, under each set's sam_flags; line_off
    delimits the lines of each read; (in the harness) the counting sink equals the written length on every line of every set"""
    src, dst = tmp_path / "sets.bin", tmp_path / "text.bin"
    src.write_bytes(SS.serialize(sets))
    assert _run(harness, "sets", src, dst)[-1] == "sets %d" % len(sets)
    n_total = 0
    for k, (s, (text, line_off, n_lines)) in enumerate(zip(sets, _split(dst.read_bytes(), sets))):
        want, want_off = SS.expected(s)
        assert text == want, (k, s["sam_flags"], text[:400], want[:400])
        assert line_off == want_off and n_lines == want.count(b"\n"), k
        n_total += n_lines
    assert n_total > 4000


def test_complement_table(harness):
    got = bytes.fromhex(_run(harness, "comp")[-1])
    want = bytearray(range(256))
    for a, b in zip(b"ACGTURYKMBVDH", b"TGCAAYRMKVBHD"):
        want[a] = b
        want[a | 0x20] = b | 0x20
    assert got == bytes(want) and got[ord("N")] == ord("N") and got[ord("S")] == ord("S") and got[ord("W")] == ord("W") and got[200] == 200


def test_sam_check_refuses(harness, tmp_path):
    """each violation on its own: MM355_EINVAL; the untouched set passes"""
    rng = np.random.default_rng(4)
    good = next(s for s in SS.random_sets(8, 400) if len(s["hits"]) > 1 and len(s["cigar"]) > 2 and (s["status"] == SS.EEMPTY).any()
                and all(len(x) or st == SS.EEMPTY for x, st in zip(s["seqs"], s["status"])) and len(s["seqs"][0]) and s["hit_off"][1] > 0)

    def variant(f):
        s = {k: (v.copy() if isinstance(v, np.ndarray) else list(v) if isinstance(v, list) else v) for k, v in good.items()}
        f(s)
        return s

    def qs_above_qe(s): s["hits"][0]["query_start"] = s["hits"][0]["query_end"] + 1
    def qe_above_qlen(s): s["hits"][0]["query_end"] = len(s["seqs"][0]) + 1
    def qs_negative(s): s["hits"][0]["query_start"] = -1
    def rid(s): s["hits"][0]["rid"] = len(s["contigs"])
    def cigar_arena(s): s["cigar"] = s["cigar"][:-1]
    def flags(s): s["sam_flags"] = 4

    def rows_on_empty(s):
        e = int(np.flatnonzero(s["status"] == SS.EEMPTY)[0])
        s["status"][e], s["status"][0] = 0, SS.EEMPTY               # the first read has rows
    cases = [("good", good, True, None, 0)] + [(f.__name__, variant(f), True, None, EINVAL)
                                               for f in (qs_above_qe, qe_above_qlen, qs_negative, rid, cigar_arena, flags, rows_on_empty)]
    cases += [("no_cigar_flag", good, False, None, EINVAL), ("null_seq", good, True, 0, EINVAL)]
    for name, s, has_cigar, drop, want in cases:
        p = tmp_path / (name + ".bin")
        p.write_bytes(SS.serialize([s], has_cigar=has_cigar, drop_seq=drop))
        assert _run(harness, "check", p) == ["rc %d" % want, "sets 1"], name


# ---------------------------------------------------------------- the reader with quality
RECS = [("r1", "ACGT" * 40 + "AC"), ("r2", "G" * 61), ("third", "ACGTN" * 30), ("r4", "T"), ("r5", "CA" * 100), ("r6", "GATTACA" * 9), ("last", "ACGTT" * 25)]


def _qual(i, n):
    return "@" + "".join(chr(33 + (7 * i + j) % 94) for j in range(n - 1))       # begins with '@', the character a header begins with


QUALS = [_qual(i, len(s)) for i, (_, s) in enumerate(RECS)]


def _fastq(eol="\n", width=None):
    out = []
    for (nm, s), q in zip(RECS, QUALS):
        w = width or len(s)
        out.append("@%s ch=7%s%s+%s%s" % (nm, eol, "".join(s[i:i + w] + eol for i in range(0, len(s), w)), eol,
                                           "".join(q[i:i + w] + eol for i in range(0, len(q), w))))
    return "".join(out)


def _read(exe, path, max_reads=1000, max_bases=10**9, qual=1):
    lines = _run(exe, "fastx", path, max_reads, max_bases, qual)
    assert lines[-1].startswith("rc ")
    batches, arrays = [], []
    for ln in lines[:-1]:
        f = ln.split(" ")
        if f[0] == "batch":
            batches.append([])
            arrays.append(int(f[2]))
        else:
            assert f[0] == "rec" and int(f[2]) == len(f[3])
            batches[-1].append((f[1], f[3], None if f[4] == "-" else f[4]))
    return int(lines[-1].split()[1]), batches, arrays


@pytest.mark.parametrize("form", ["plain", "gzip", "crlf", "multiline"])
def test_reader_keeps_qualities(harness, tmp_path, form):
    txt = _fastq("\r\n" if form == "crlf" else "\n", 50 if form == "multiline" else None)
    p = tmp_path / ("reads." + form)
    p.write_bytes(gzip.compress(txt.encode()) if form == "gzip" else txt.encode())
    want = [(nm, s, q) for (nm, s), q in zip(RECS, QUALS)]
    rc, batches, arrays = _read(harness, p)
    assert rc == 0 and batches == [want] and arrays == [1]
    # a sub-batch cut by max_bases: the held record keeps its quality
    rc, batches, arrays = _read(harness, p, max_bases=len(RECS[0][1]) + len(RECS[1][1]))
    assert rc == 0 and batches[0] == want[0:2] and [r for b in batches for r in b] == want and len(batches) > 2
    rc, batches, arrays = _read(harness, p, max_reads=1)
    assert rc == 0 and batches == [[r] for r in want]
    # opened without quality: the same records, no array
    rc, batches, arrays = _read(harness, p, qual=0)
    assert rc == 0 and batches == [[(nm, s, None) for nm, s in RECS]] and arrays == [0]


def test_reader_fasta_and_errors(harness, tmp_path):
    fa = tmp_path / "reads.fa"
    fa.write_text("".join(">%s c\n%s\n" % r for r in RECS))
    rc, batches, arrays = _read(harness, fa)
    assert rc == 0 and batches == [[(nm, s, None) for nm, s in RECS]] and arrays == [1]      # the array is there, every entry null
    # a quality of another length than the sequence is dropped, the record stays
    bad = tmp_path / "bad.fq"
    bad.write_text("@a\nACGT\n+\nIIIII\n@b\nAC\n+\nII\n")
    rc, batches, arrays = _read(harness, bad)
    assert rc == 0 and [r[2] for r in batches[0]][1] == "II" and batches[0][0][:2] == ("a", "ACGT") and batches[0][0][2] is None
    blob = gzip.compress((_fastq() * 200).encode())
    cut = tmp_path / "cut.fq.gz"
    cut.write_bytes(blob[:len(blob) // 2])
    rc, batches, arrays = _read(harness, cut, max_reads=16)
    assert rc == EIO and sum(map(len, batches)) > 0
