"""The host side of the PAF writer (mappy-rs_amd/csrc/mm355_paf.h, the streaming FASTA / FASTQ reader of mm355_index.cpp), built with g++
under AddressSanitizer and UBSan into a stand-alone program (tests/host_harness/paf_host.cpp): the %.4f routine and the integer writer
against snprintf, the host formatter against mappy_rs.paf_line on about 2000 result sets (tests/_paf_sets.py), the reader against records
written here.  GPU side: tests/test_gpu_paf.py."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import _capi
import _paf_sets as PS

EINVAL, EIO = -2, -4


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("paf_host") / "paf_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(_capi.HERE, "host_harness", "paf_host.cpp"), "-o", exe, "-lz", "-lpthread"])
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


def test_f4_equals_printf(harness):
    """every k / 20000 as a double and rounded to float32, the exact ties, 0, 1, the smallest denormal, 1 - 630 / 653, a million random
    float32 values, 1 - a / b and float32 neighbours of 5th-decimal midpoints: the digits, and the counting sink's length"""
    name, checked, wrong = _run(harness, "f4")[-1].split()
    assert name == "f4" and int(checked) > 1800000 and int(wrong) == 0


def test_integer_writer(harness):
    name, checked, wrong = _run(harness, "ints")[-1].split()
    assert name == "ints" and int(checked) > 150 and int(wrong) == 0


@pytest.fixture(scope="module")
def sets(built):
    return PS.handmade_sets() + PS.random_sets(20260, 2000)


def test_generator_covers_the_cases(sets):
    rnd = sets[4:]
    assert {len(s["cigar"]) > 0 for s in rnd} == {True, False} and {s["has_cigar"] for s in rnd} == {True, False}
    first = {int(s["hits"][0]["n_cigar"]) for s in rnd if len(s["hits"])}
    assert set(PS.CIGAR_COUNTS) <= first
    ops = np.concatenate([s["cigar"] & 0xf for s in rnd])
    assert set(ops.tolist()) == set(range(9)) and int(max(np.concatenate([s["cigar"] >> 4 for s in rnd]))) == 2**28 - 1
    hits = np.concatenate([s["hits"] for s in rnd]); tags = np.concatenate([s["tags"] for s in rnd])
    assert (hits["cs_len"] >= 0).any() and (hits["cs_len"] < 0).any() and (hits["md_len"] >= 0).any() and (hits["md_len"] < 0).any()
    assert {-1.0, 0.0, 1.5} <= set(tags["div"].tolist()) and set(tags["flags"].tolist()) == set(range(16))
    assert (hits["mapq"] == 2**32 - 1).any() and (hits["dp_score"] < 0).any() and (tags["score"] == -2**31).any()
    names = [q for s in rnd for q in s["qnames"]]
    assert None in names and any(q and " " in q for q in names) and any(q and len(q) == 255 for q in names) and "x" in names
    assert any(s["status"][i] == PS.EEMPTY for s in rnd for i in range(len(s["status"])))
    assert any(s["hit_off"][i] == s["hit_off"][i + 1] and s["status"][i] == 0 for s in rnd for i in range(len(s["status"])))
    assert {len(c) for c in PS.CONTIGS} >= {1, 255}


def test_host_formatter_equals_paf_line(harness, sets, tmp_path):
    """the emitter run serially == "".join(paf_line(...) + "\\n") over _batch_to_mappings of the same arrays; line_off delimits the lines of
    each read; (in the harness) the counting sink equals the written length on every line of every set"""
    src, dst = tmp_path / "sets.bin", tmp_path / "text.bin"
    src.write_bytes(PS.serialize(sets))
    assert _run(harness, "sets", src, dst)[-1] == "sets %d" % len(sets)
    got = dst.read_bytes()
    at = 0
    for k, s in enumerate(sets):
        nr = len(s["qlens"])
        n_text = int(np.frombuffer(got, np.int64, 1, at)[0])
        line_off = np.frombuffer(got, np.int64, nr + 1, at + 8).tolist()
        text = got[at + 8 * (nr + 2):at + 8 * (nr + 2) + n_text]
        at += 8 * (nr + 2) + n_text
        want, want_off = PS.expected(s)
        assert text == want, (k, text[:300], want[:300])
        assert line_off == want_off, k
        for i in range(nr):
            assert text[line_off[i]:line_off[i + 1]].count(b"\n") == s["hit_off"][i + 1] - s["hit_off"][i]
    assert at == len(got)
    # the hand-made lines of tests/test_tags_host.py, spelled out
    assert PS.expected(sets[0])[0] == (b"read1\t5000\t12\t4890\t+\tchr1\t1500000\t100200\t105123\t1741\t4923\t60\ttp:A:P\tcm:i:180\ts1:i:1690\ts2:i:42"
                                       b"\tdv:f:0.0312\trl:i:37\n")


# ---------------------------------------------------------------- the reader
RECS = [("r1", "ACGT" * 40 + "AC"), ("r2", "G" * 61), ("third", "ACGTN" * 30), ("r4", "T"), ("r5", "CA" * 100), ("r6", "GATTACA" * 9), ("last", "ACGTT" * 25)]


def _fasta(recs, eol="\n", comment=" a comment\tmore", last_newline=True):
    out = []
    for nm, s in recs:
        out.append(">" + nm + comment + eol)
        out += [s[i:i + 60] + eol for i in range(0, len(s), 60)]
    txt = "".join(out)
    return txt if last_newline else txt[:-len(eol)]


def _fastq(recs, eol="\n", comment=" ch=7"):
    # the quality string begins with '@', the character a header begins with
    return "".join("@%s%s%s%s%s+%s%s%s" % (nm, comment, eol, s, eol, eol, "@" + "I" * (len(s) - 1), eol) for nm, s in recs)


def _read(exe, path, max_reads=1000, max_bases=10**9):
    lines = _run(exe, "fastx", path, max_reads, max_bases)
    assert lines[-1].startswith("rc ")
    batches = []
    for ln in lines[:-1]:
        f = ln.split(" ")
        if f[0] == "batch":
            batches.append([])
            n = int(f[1])
        else:
            assert f[0] == "rec" and int(f[2]) == len(f[3])
            batches[-1].append((f[1], f[3]))
    return int(lines[-1].split()[1]), batches


@pytest.mark.parametrize("form", ["fasta", "fasta_crlf", "fasta_no_last_newline", "fastq", "fastq_crlf", "fasta_gz", "fastq_gz"])
def test_reader_records(harness, tmp_path, form):
    txt = {"fasta": _fasta(RECS), "fasta_crlf": _fasta(RECS, "\r\n"), "fasta_no_last_newline": _fasta(RECS, last_newline=False),
           "fastq": _fastq(RECS), "fastq_crlf": _fastq(RECS, "\r\n"), "fasta_gz": _fasta(RECS), "fastq_gz": _fastq(RECS)}[form]
    p = tmp_path / ("reads." + form)
    p.write_bytes(gzip.compress(txt.encode()) if form.endswith("_gz") else txt.encode())
    rc, batches = _read(harness, p)
    assert rc == 0 and batches == [RECS]
    rc, batches = _read(harness, p, max_reads=1)
    assert rc == 0 and batches == [[r] for r in RECS]
    rc, batches = _read(harness, p, max_reads=3)
    assert rc == 0 and batches == [RECS[0:3], RECS[3:6], RECS[6:7]]
    # a base limit smaller than any record still returns a record per call; one that fits two of the first three
    rc, batches = _read(harness, p, max_bases=1)
    assert rc == 0 and batches == [[r] for r in RECS]
    rc, batches = _read(harness, p, max_bases=len(RECS[0][1]) + len(RECS[1][1]))
    assert rc == 0 and batches[0] == RECS[0:2] and [r for b in batches for r in b] == RECS


def test_reader_errors(harness, tmp_path):
    rng = np.random.default_rng(5)
    recs = [("r%d" % i, "".join("ACGT"[c] for c in rng.integers(0, 4, 3000))) for i in range(200)]
    blob = gzip.compress(_fastq(recs).encode())
    cut = tmp_path / "cut.fq.gz"
    cut.write_bytes(blob[:len(blob) // 2])
    rc, batches = _read(harness, cut, max_reads=16)
    assert rc == EIO and 0 < sum(map(len, batches)) < len(recs)     # whole sub-batches before the cut were handed out, then the error
    assert [r for b in batches for r in b] == recs[:sum(map(len, batches))]
    rc, batches = _read(harness, tmp_path / "missing.fa")
    assert rc == EIO and batches == []
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b"")
    assert _read(harness, empty) == (0, [])
