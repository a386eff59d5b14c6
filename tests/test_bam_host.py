"""The host side of the BAM writer (mappy-rs_amd/csrc/mm355_bam.h), built with g++ under AddressSanitizer and UBSan into a stand-alone
program (tests/host_harness/bam_host.cpp): tests/_bam.py::record_of against hand-written records -- the only independent pin of the
encoding --, the host formatter against record_of of mappy_rs.sam_lines on about 2000 result sets (tests/_bam_sets.py), the long-CIGAR
switch, the integer type boundaries, mm355_bam_check, the framing against _bam.frame and gzip, and the framing kernel's CRC scheme run
serially against zlib.  GPU side: tests/test_gpu_bam.py."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import _bam
import _bam_sets as BS
import _capi
import _sam_sets as SS
from test_sam_host import _pair, _records, _row, M, READ20, QUAL20

TWO = ["chr1", "chr2"]
H = bytes.fromhex
NONE = H("ffffffff ffffffff 00000000")                     # next_refID, next_pos, tlen


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bam_host") / "bam_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(_capi.HERE, "host_harness", "bam_host.cpp"), "-o", exe, "-lz", "-lpthread"])
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


# ---------------------------------------------------------------- record_of against literal records
def test_record_forward_primary_with_quality(built):
    import mappy_rs
    ms = _records(built, [_row(2, 9, 1, 0, 99, 106, 7, 7, 60, 1, 0, 1, 0, 3, 0, 14, 14)], [dict(score=40, rep_len=5, flags=2)], [7 << 4 | M])
    line, = mappy_rs.sam_lines(ms, "r1 comment", "ACGTACGTAC", "ABCDEFGHIJ")
    assert _bam.record_of(line, TWO) == (
        H("69000000") +                                     # block_size 105
        H("00000000 63000000 03 3c 4912 0300 0000 0a000000") + NONE +      # chr1, pos 99, name + NUL, mapq 60, bin 4681, 3 words, flag 0, 10 bases
        b"r1\0" + H("24000000 70000000 14000000") +         # 2S 7M 1S
        H("12 48 12 48 12") + H("20 21 22 23 24 25 26 27 28 29") +         # A=1 C=2 G=4 T=8; 'A' - 33 = 32 ...
        b"NMC\x00" b"msC\x0e" b"ASC\x0e" b"nnC\x00" b"tpAP" b"cmC\x03" b"s1C\x28" b"s2C\x00" + b"def" + H("00000000") + b"rlC\x05")


def test_record_reverse_primary(built):
    """the read holds N, a lower-case base, R, U, u and =: on the reverse strand U and u become A and a (code 1), = stays 0"""
    import mappy_rs
    ms = _records(built, [_row(1, 6, -1, 1, 0, 5, 4, 5, 7, 1, 1, 1, 0, 2, 11, 8, 6)], [dict(score=30, rep_len=0, flags=2)], [5 << 4 | M])
    line, = mappy_rs.sam_lines(ms, "r2", "ACGNtRUu=C", "0123456789")
    assert line.split("\t")[9:11] == ["G=aAYaNCGT", "9876543210"]
    assert _bam.record_of(line, TWO) == (
        H("69000000") +
        H("01000000 00000000 03 07 4912 0300 1000 0a000000") + NONE +      # chr2, pos 0, mapq 7, flag 16
        b"r2\0" + H("44000000 50000000 14000000") +         # 4S 5M 1S
        H("40 11 a1 f2 48") +                               # G =  a A  Y a  N C  G T
        H("18 17 16 15 14 13 12 11 10 0f") +                # '9' - 33 = 24 down to '0' - 33 = 15
        b"NMC\x01" b"msC\x08" b"ASC\x06" b"nnC\x00" b"tpAP" b"cmC\x02" b"s1C\x1e" b"s2C\x0b" + b"def" + H("cdcc4c3e") + b"rlC\x00")   # de 0.2000: 0x3e4ccccd
    # forwards U and u are no code: 15
    assert _bam.record_of("x\t0\tchr1\t1\t0\t*\t*\t0\t0\tUu=a\t*", TWO)[4 + 32 + 2:] == H("ff 01 ffffffff")


def test_record_secondary(built):
    import mappy_rs
    rows = [_row(2, 9, 1, 0, 99, 106, 7, 7, 60, 1, 0, 1, 0, 3, 0, 14, 14), _row(3, 9, -1, 1, 10, 16, 6, 6, 0, 0, 0, 1, 1, 3, 0, 12, 12)]
    ms = _records(built, rows, [dict(score=40, flags=2), dict(score=33, flags=0)], [7 << 4 | M, 6 << 4 | M])
    line = mappy_rs.sam_lines(ms, "r1", "ACGTACGTAC", "ABCDEFGHIJ")[1]
    assert _bam.record_of(line, TWO) == (
        H("56000000") +                                     # 86
        H("01000000 0a000000 03 00 4912 0300 1001 00000000") + NONE +      # flag 272, no bases
        b"r1\0" + H("14000000 60000000 34000000") +         # 1S 6M 3S
        b"NMC\x00" b"msC\x0c" b"ASC\x0c" b"nnC\x00" b"tpAS" b"cmC\x03" b"s1C\x21" + b"def" + H("00000000") + b"rlC\x00")


def test_record_hard_clipped_reverse_supplementary(built):
    import mappy_rs
    line = mappy_rs.sam_lines(_pair(built, strand1=-1), "q", READ20, QUAL20)[1]
    assert line.split("\t")[5] == "4M1D4M12H"
    assert _bam.record_of(line, TWO) == (
        H("84000000") +                                     # 132
        H("01000000 f4010000 02 1e 4912 0400 1008 08000000") + NONE +      # chr2, pos 500, mapq 30, flag 2064, the 8 bases of the slice
        b"q\0" + H("40000000 12000000 40000000 c5000000") +                # 4M 1D 4M 12H
        H("12 48 11 11") + H("53 52 51 50 4f 4e 4d 4c") +   # ACGTAAAA; "tsrqponm" - 33
        b"NMC\x01" b"msC\x0a" b"ASC\x0a" b"nnC\x00" b"tpAP" b"cmC\x02" b"s1C\x14" b"s2C\x00" + b"def" + H("6688e33d") +   # de 0.1111: 0x3de38866
        b"SAZchr1,1001,+,12M8S,60,0;\0" + b"rlC\x00")


def test_record_unmapped_without_quality(built):
    import mappy_rs
    line, = mappy_rs.sam_lines([], "u 1", "ACGTN", rl=300)
    assert _bam.record_of(line, TWO) == (
        H("2f000000") +                                     # 47
        H("ffffffff ffffffff 02 00 4812 0000 0400 05000000") + NONE +      # bin 4680, flag 4
        b"u\0" + H("12 48 f0") + H("ff ff ff ff ff") + b"rlS" + H("2c01"))


def test_record_integer_types():
    """htslib's smallest type on each side of every boundary, and a negative NM"""
    line = "x\t0\tchr1\t1\t0\t1M\t*\t0\t0\tA\t!\tNM:i:-1\tms:i:255\tAS:i:256\tnn:i:65535\tcm:i:65536\ts1:i:-128\ts2:i:-129\tzd:i:-32768\trl:i:-32769"
    assert _bam.record_of(line, TWO) == (
        H("56000000") +                                     # 86
        H("00000000 00000000 02 00 4912 0100 0000 01000000") + NONE + b"x\0" + H("10000000") + H("10") + H("00") +
        b"NMc\xff" b"msC\xff" b"ASS\x00\x01" b"nnS\xff\xff" b"cmI\x00\x00\x01\x00" b"s1c\x80" b"s2s\x7f\xff" b"zds\x00\x80" b"rli\xff\x7f\xff\xff")


# ---------------------------------------------------------------- the host formatter against record_of
@pytest.fixture(scope="module")
def sets(built):
    return BS.random_sets(20262, 2000)


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


def _host(harness, sets, tmp_path, tag="sets"):
    src, dst = tmp_path / (tag + ".bin"), tmp_path / (tag + ".out")
    src.write_bytes(SS.serialize(sets))
    assert _run(harness, "sets", src, dst)[-1] == "sets %d" % len(sets)
    return list(_split(dst.read_bytes(), sets))


def test_generator_covers_the_cases(sets):
    reads = "".join(x for s in sets for x in s["seqs"])
    assert set("=NRUuacgt.") <= set(reads) and "*" not in reads
    hits = np.concatenate([s["hits"] for s in sets])
    assert hits["mapq"].max() == 255 and max(len(q) for s in sets for q in s["qnames"] if q) == 254
    assert {s["sam_flags"] for s in sets} == {0, 1, 2, 3} and any(None in s["quals"] for s in sets)
    odd = [len(x) % 2 for s in sets for x in s["seqs"]]
    assert 0 in odd and 1 in odd


def test_host_formatter_equals_record_of(harness, sets, tmp_path):
    n_total, kinds = 0, set()
    for k, (s, (text, line_off, n_lines)) in enumerate(zip(sets, _host(harness, sets, tmp_path))):
        want, want_off = BS.expected(s)
        got = _bam.split(text)
        assert got == want, (k, s["sam_flags"], [i for i, (a, b) in enumerate(zip(got, want)) if a != b][:3], len(got), len(want))
        assert line_off == want_off and n_lines == len(want), k
        assert text == _bam.frame(b"".join(want)), k
        n_total += n_lines
        kinds |= {struct.unpack_from("<H", r, 18)[0] & 0x914 for r in want}
    assert n_total > 4000 and kinds >= {0, 0x10, 0x100, 0x110, 0x800, 0x810, 4}


def test_integer_types_and_long_cigar(harness, tmp_path):
    """the boundary values through the emitter; rows of 65534 / 65535 / 65536 words with their clips: the last takes htslib's long form"""
    rng = np.random.default_rng(3)
    sets = [BS.boundary_set()] + [BS.long_cigar_set(n, rng, strand) for n in (65534, 65535, 65536) for strand in (1, -1)]
    out = _host(harness, sets, tmp_path, "special")
    for k, (s, (text, line_off, n_lines)) in enumerate(zip(sets, out)):
        want, want_off = BS.expected(s)
        assert _bam.split(text) == want and line_off == want_off, k
    types = b"".join(bytes([r[r.index(b"NM") + 2]]) for r in BS.expected(sets[0])[0])
    assert types == b"CcCSSIcssiIi"
    for k, n in zip(range(1, 7), (65534, 65534, 65535, 65535, 65536, 65536)):
        r, = BS.expected(sets[k])[0]
        n_op = struct.unpack_from("<H", r, 16)[0]
        assert n_op == (2 if n == 65536 else n) and (r.find(b"CGBI" + struct.pack("<I", 65536)) > 0) == (n == 65536)
        if n == 65536:
            l_seq, = struct.unpack_from("<I", r, 20)
            assert struct.unpack_from("<II", r, 36 + len("long0") + 1)[0] == l_seq << 4 | 4 and l_seq == 300


def test_bam_check_refuses(harness, tmp_path):
    for name, s in BS.refused_sets():
        p = tmp_path / (name + ".bin")
        p.write_bytes(SS.serialize([s]))
        assert _run(harness, "check", p) == ["rc %d" % (0 if name in ("good", "name254") else BS.EINVAL), "sets 1"], name


# ---------------------------------------------------------------- framing
SIZES = (0, 1, 0xff00 - 1, 0xff00, 0xff00 + 1, 3 * 0xff00 + 77)


def test_frame_equals_host_wrap_and_gzip(harness, tmp_path):
    rng = np.random.default_rng(9)
    for n in SIZES:
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        src, dst = tmp_path / "d.bin", tmp_path / "d.bgzf"
        src.write_bytes(data)
        _run(harness, "wrap", src, dst)
        got = dst.read_bytes()
        assert got == _bam.frame(data) and len(got) == n + 31 * ((n + 0xff00 - 1) // 0xff00), n
        assert (gzip.decompress(got) if n else got) == data, n
    assert gzip.decompress(_bam.EOF) == b"" and len(_bam.EOF) == 28


def test_lane_crc_equals_zlib(harness, tmp_path):
    """the framing kernel's CRC-32 -- 256 lanes with a 256-byte chunk each, the payload at the end of the lanes' message, eight combine
    levels -- run serially: every payload length around a chunk and around the block, random bytes, zeros and 0xFF"""
    rng = np.random.default_rng(10)
    for n in (1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 256 * 255 - 1, 0xff00 - 1, 0xff00, 0xff00 + 1, 3 * 0xff00 + 77):
        for fill in (None, 0, 255):
            data = rng.integers(0, 256, n, dtype=np.uint8).tobytes() if fill is None else bytes([fill]) * n
            src = tmp_path / "c.bin"
            src.write_bytes(data)
            assert _run(harness, "crc", src) == ["crc %d" % ((n + 0xff00 - 1) // 0xff00)], (n, fill)


def test_code_table(harness):
    fwd, rev = (bytes.fromhex(x) for x in _run(harness, "codes"))
    want = bytearray([15]) * 256
    for i, c in enumerate(b"=ACMGRSVTWYHKDBN"):
        want[c] = want[c | 0x20 if c != ord("=") else c] = i
    assert fwd == bytes(want) and fwd[ord("U")] == fwd[ord("u")] == 15
    comp = {a: b for a, b in zip(b"ACGTURYKMBVDH", b"TGCAAYRMKVBHD")}
    for c in range(256):
        u = c & 0xdf if chr(c).isascii() and chr(c).isalpha() else c
        assert rev[c] == (want[comp[u]] if u in comp else want[c]), c
    assert rev[ord("U")] == rev[ord("u")] == 1 and rev[ord("=")] == 0
