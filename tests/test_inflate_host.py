"""The BGZF inflate stage on the host (mappy-rs_amd/csrc/mm355_inflate.h: the functions the kernel's lanes call, run serially; mm355_bgzfwalk.h;
the BAM record loop of mm355_bamread.h), built with g++ under AddressSanitizer and UBSan into a stand-alone program
(tests/host_harness/inflate_host.cpp).  The oracle is Python's zlib: every member of every producer inflates to its payload; every
constructed refusal is refused for its own reason; over 20 000 single-bit flips and truncations the decoder's verdict is zlib's, and the
payload is identical where both accept.  GPU side: tests/test_gpu_inflate.py."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import zlib

import pytest

import _capi
import _inflate as I

# why inf_member_host refuses each constructed member (the enum of mm355_inflate.h)
BTYPE, STORED, HEADER, OVER, INCOMPLETE, NO_EOB, REPEAT, SYMBOL, DIST, OUT_LONG, OUT_SHORT, INPUT, CRC = range(1, 14)
REASON = {"btype_11": BTYPE, "stored_len_nlen": STORED, "oversubscribed_literal": OVER, "oversubscribed_distance": OVER, "oversubscribed_code_length": OVER,
          "incomplete_literal": INCOMPLETE, "incomplete_distance": INCOMPLETE, "incomplete_single_code_of_two_bits": INCOMPLETE, "incomplete_code_length": INCOMPLETE,
          "no_end_of_block_code": NO_EOB, "repeat_without_previous": REPEAT, "run_past_hlit_hdist": REPEAT, "length_symbol_286": SYMBOL, "length_symbol_287": SYMBOL,
          "distance_symbol_30": SYMBOL, "distance_symbol_31": SYMBOL, "distance_before_the_first_byte": DIST, "match_at_position_0": DIST,
          "output_passes_isize": OUT_LONG, "match_passes_isize": OUT_LONG, "output_short_of_isize": OUT_SHORT, "crc_mismatch": CRC,
          "input_ends_in_a_symbol": INPUT, "input_ends_before_the_last_block": INPUT, "no_input": INPUT, "stored_runs_out": INPUT, "hlit_above_286": HEADER}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inflate_host") / "inflate_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(_capi.HERE, "host_harness", "inflate_host.cpp"), "-o", exe, "-lz", "-lpthread"])
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


def _cases(exe, d, cases):
    """(cdata, crc, isize) each through the program: [(status, payload or None)]"""
    src, dst = d / "cases.bin", d / "cases.out"
    with open(src, "wb") as f:
        for c, crc, isize in cases:
            f.write(struct.pack("<III", len(c), isize, crc) + c)
    st = [int(x) for x in _run(exe, "cases", src, dst)]
    assert len(st) == len(cases)
    out, at, res = dst.read_bytes(), 0, []
    for (c, crc, isize), s in zip(cases, st):
        res.append((s, out[at:at + isize] if s == 0 else None))
        at += isize if s == 0 else 0
    assert at == len(out)
    return res


def test_every_valid_member_inflates_to_its_payload(harness, built, tmp_path):
    ms = I.zlib_members() + I.own_members() + I.built_members()
    assert len(ms) > 500 and {n.split("/")[1] for n, _, _ in ms if n.startswith("zlib/")} == {c[0] for c in I.CODINGS} | {"sync"}
    # what the producers must have emitted for the list to mean anything: several blocks in a member, a distance of 32768, an ISIZE of 65536
    assert any(len(p) == 65536 for _, _, p in ms) and any(p == b"" for _, _, p in ms)
    got = _cases(harness, tmp_path, [I.parts(m) for _, m, _ in ms])
    for (name, m, p), (s, out) in zip(ms, got):
        assert s == 0 and out == p, (name, s)


def test_every_constructed_refusal_is_refused_for_its_reason(harness, tmp_path):
    rf = I.refusals()
    assert {n.split("/")[1] for n, _, _ in rf} == set(REASON)
    got = _cases(harness, tmp_path, [I.parts(m) for _, m, _ in rf])
    for (name, _, _), (s, _) in zip(rf, got):
        assert s == REASON[name.split("/")[1]], (name, s)


def test_mutations_get_zlibs_verdict(harness, built, tmp_path):
    """20 000 single-bit flips and truncations, fixed seed, none left out: the verdict is Python's on every one, the payload identical on
    acceptance; and zlib accepts a mutation only where the bit is one nobody reads (the payload is then the unmutated one: the trailer stayed)"""
    muts = I.mutations(20000)
    cases = [c for c, _ in muts]
    want = [I.verdict(*c) for c in cases]
    got = _cases(harness, tmp_path, cases)
    n_acc = 0
    for k, (w, (s, out)) in enumerate(zip(want, got)):
        assert (s == 0) == (w is not None), (k, s)
        assert out == w, k
        assert w is None or w == muts[k][1], k           # zlib itself: accepted means nothing changed
        n_acc += w is not None
    print("accepted", n_acc, "of", len(cases))
    assert 0 < n_acc < len(cases) // 4           # ignored bits exist (the padding in front of a stored block's LEN and behind the last code, the
                                                 # length bits of unused code-length symbols), and they are a minority of any stream's bits


def test_walk(harness, built, tmp_path):
    ms = I.built_members()[:3] + I.zlib_members()[:3]
    stream, payload = I.mixed_stream(ms)
    f = tmp_path / "s.bgzf"
    f.write_bytes(stream)
    lines = _run(harness, "walk", f, 1, 1)
    assert lines[0] == "rc 0 used %d out %d" % (len(stream), len(payload))
    at = o = 0
    for (name, m, p), ln in zip(ms[:3] + [("eof", I.EOF, b"")] + ms[3:] + [("eof", I.EOF, b"")], lines[1:]):
        c, crc, isize = I.parts(m)
        assert tuple(map(int, ln.split())) == (at + len(m) - 8 - len(c), len(c), isize, crc, o), name    # (a subfield in front of BC moves cdata)
        at += len(m)
        o += len(p)
    assert len(lines) == 1 + len(ms) + 2
    # a missing EOF block is tolerated
    f.write_bytes(stream[:-len(I.EOF)])
    assert _run(harness, "walk", f, 1, 1)[0] == "rc 0 used %d out %d" % (len(stream) - len(I.EOF), len(payload))
    # the buffer ends inside the last member: a piece (the rest goes in front of the next) or, at the end of the file, an error
    cut = len(stream) - len(I.EOF) - 5
    f.write_bytes(stream[:cut])
    whole = cut + 5 - len(ms[-1][1])
    assert _run(harness, "walk", f, 1, 0)[0] == "rc 0 used %d out %d" % (whole, len(payload) - len(ms[-1][2]))
    assert _run(harness, "walk", f, 1, 1)[0].startswith("rc -4 ")
    for k in (1, 3, 11, 13, 17):                 # ... anywhere inside the header too
        f.write_bytes(stream[:len(ms[0][1]) + k])
        assert _run(harness, "walk", f, 1, 0)[0] == "rc 0 used %d out %d" % (len(ms[0][1]), len(ms[0][2])), k
    # plain gzip and text are "not BGZF" (1) when they come first, an error behind a member
    for other in (gzip.compress(b"hello"), b">chr1\nACGT\n", b"\x1f\x8b", b""):
        f.write_bytes(other)
        assert _run(harness, "walk", f, 1, 1)[0].startswith("rc %d " % (1 if other else 0)), other
        f.write_bytes(ms[0][1] + other + b"x" * 30)
        assert _run(harness, "walk", f, 1, 1)[0].startswith("rc -4 "), other
    # a BC subfield that claims less than header and trailer, a subfield that leaves the extra field, an ISIZE above 65536
    m = bytearray(ms[3][1])
    bad1 = bytes(m[:16]) + struct.pack("<H", 20) + bytes(m[18:])
    bad2 = bytes(m[:14]) + struct.pack("<H", 40) + bytes(m[16:])
    bad3 = bytes(m[:-4]) + struct.pack("<I", 65537)
    for bad in (bad1, bad2, bad3):
        f.write_bytes(ms[0][1] + bad)
        assert _run(harness, "walk", f, 1, 1)[0].startswith("rc -4 ")
    # max_out: no more members than fit, but one at least
    f.write_bytes(stream)
    assert len(_run(harness, "walk", f, 1, 1, 1)) == 2
    n2 = len(ms[0][2]) + len(ms[1][2])
    assert len(_run(harness, "walk", f, 1, 1, n2)) == 3
    # the whole file through walk and decoder
    o = tmp_path / "s.out"
    assert _run(harness, "unwrap", f, o) == ["members %d bytes %d" % (len(ms) + 2, len(payload))] and o.read_bytes() == payload
    f.write_bytes(ms[0][1] + I.refusals()[0][1] + I.EOF)
    assert _run(harness, "unwrap", f, o) == ["rc -4"]


def _bam_lines(harness, tmp_path, data, chunk=7):
    f = tmp_path / "in.bam.raw"
    f.write_bytes(data)
    return _run(harness, "bam", f, chunk)


def test_bam_record_loop(harness, tmp_path):
    recs = I.fastq_records(12)
    assert len(recs[0][1]) % 2 == 1                      # an odd l_seq
    want = ["%s %s %s" % (n.decode(), s.decode(), q.decode()) for n, s, q in recs]
    for chunk in (1, 7, 1 << 20):
        assert _bam_lines(harness, tmp_path, I.ubam_bytes(recs), chunk) == want + ["rc 0"]
    # no quality (0xff), secondary and supplementary records skipped, a reverse-strand record turned back; an aligned BAM's header and CIGARs
    head = I.bam_header(b"@SQ\tSN:chr1\tLN:1000\n", [(b"chr1", 1000), (b"chrUn_x", 77)])
    n, s, q = recs[3]
    body = (I.bam_record(b"a", b"ACGTN", None) + I.bam_record(b"sec", b"AC", b"II", flag=0x100) + I.bam_record(n, s, q, flag=0x10, n_cigar=3) +
            I.bam_record(b"sup", b"ACG", b"III", flag=0x800 | 0x10) + I.bam_record(b"r", b"ACGGTN", b"ABCDEF", flag=0x10) + I.bam_record(b"e", b"", b""))
    assert _bam_lines(harness, tmp_path, head + body) == ["a ACGTN *", "%s %s %s" % (n.decode(), s.decode(), q.decode()), "r ACGGTN ABCDEF", "e  *", "rc 0"]
    assert _bam_lines(harness, tmp_path, I.bam_header()) == ["rc 0"]
    # every malformed record is refused, after the records in front of it
    good = I.bam_record(b"ok", b"ACGT", b"IIII")
    bad = {"block_size_below_32": struct.pack("<I", 31) + b"\0" * 31,
           "block_size_above_the_stream": I.bam_record(b"x", b"ACGT", b"IIII", block_size=5000),
           "l_read_name_0": I.bam_record(b"x", b"ACGT", b"IIII", l_name=0),
           "fields_exceed_block_size": I.bam_record(b"x", b"ACGT", b"IIII", l_seq=9),
           "l_seq_huge": I.bam_record(b"x", b"ACGT", b"IIII", l_seq=0xfffffff0),
           "cigar_exceeds_block_size": I.bam_record(b"x", b"ACGT", b"IIII")[:16] + struct.pack("<H", 60000) + I.bam_record(b"x", b"ACGT", b"IIII")[18:],
           "ends_in_the_fixed_fields": good[:17], "ends_in_block_size": good[:2], "ends_in_seq": good[:-5]}
    for name, b in bad.items():
        assert _bam_lines(harness, tmp_path, I.bam_header() + good + b, 5) == ["ok ACGT IIII", "rc -4"], name
    for k in (3, 6, 20, 30):                                 # a stream that ends inside the header
        assert _bam_lines(harness, tmp_path, head[:k]) == ["rc -4"], k
    assert _bam_lines(harness, tmp_path, b"BAM\1" + struct.pack("<i", -1)) == ["rc -4"]


def _read_all(L, ffi, path, qual=True, max_reads=5, opener=None):
    fx = C.c_void_p()
    rc = opener(fx) if opener else (L.mm355_fastx_open_qual if qual else L.mm355_fastx_open)(os.fsencode(str(path)), C.byref(fx))
    if rc:
        return rc
    out = []
    try:
        while True:
            rp = C.POINTER(ffi.Reads)()
            rc = L.mm355_fastx_next(fx, max_reads, 1 << 30, C.byref(rp))
            if rc:
                return rc
            if not rp:
                return out
            r = rp.contents
            qs = L.mm355_reads_quals(rp)
            for i in range(r.n):
                ln = r.lens[i]
                out.append((r.names[i], C.string_at(r.seqs[i], ln), C.string_at(qs[i], ln) if qs and qs[i] else None))
            L.mm355_reads_free(rp)
    finally:
        L.mm355_fastx_close(fx)


def test_library_reads_bam_and_bgzip_through_the_host_reader(built, tmp_path):
    """in process, no GPU: mm355_fastx_open_qual on a .bam and on a bgzip FASTQ gives the names, bases and qualities of the plain FASTQ;
    bgzf_unwrap inverts bgzf_wrap; a corrupt member raises"""
    import mappy_rs
    from mappy_rs import _ffi
    L = _ffi.lib()
    recs = I.fastq_records(40)
    text = I.fastq_text(recs)
    plain, bgz, bam, trunc = tmp_path / "r.fq", tmp_path / "r.fq.gz", tmp_path / "r.bam", tmp_path / "t.bam"
    plain.write_bytes(text)
    bgz.write_bytes(I.bgzf_file(text, 997))
    bam.write_bytes(I.bgzf_file(I.ubam_bytes(recs), 1501))
    want = [(n, s, q) for n, s, q in recs]
    assert _read_all(L, _ffi, plain) == want
    assert _read_all(L, _ffi, bgz) == want
    assert _read_all(L, _ffi, bam) == want
    assert _read_all(L, _ffi, bam, qual=False) == [(n, s, None) for n, s, q in recs]
    trunc.write_bytes(I.bgzf_file(I.ubam_bytes(recs)[:-9], 1501))
    assert _read_all(L, _ffi, trunc) == _ffi.MM355_EIO
    for name, data in list(I.D.payloads().items())[::3]:
        assert mappy_rs.bgzf_unwrap(mappy_rs.bgzf_wrap(data, compress=True)) == data, name
        assert mappy_rs.bgzf_unwrap(mappy_rs.bgzf_wrap(data)) == data, name
    stream, payload = I.mixed_stream(I.built_members() + I.zlib_members()[::17])
    assert mappy_rs.bgzf_unwrap(stream) == payload and mappy_rs.bgzf_unwrap(b"") == b""
    with pytest.raises(_ffi.Mm355Error) as e:
        mappy_rs.bgzf_unwrap(gzip.compress(b"plain gzip"))
    assert e.value.code == _ffi.MM355_EINVAL
    k = len(I.built_members()[0][1]) - 6                 # a bit of the first member's CRC-32
    for bad in (stream[:-40], stream[:k] + bytes([stream[k] ^ 4]) + stream[k + 1:], I.built_members()[0][1] + I.refusals()[5][1]):
        with pytest.raises(_ffi.Mm355Error) as e:
            mappy_rs.bgzf_unwrap(bad)
        assert e.value.code == _ffi.MM355_EIO
    assert "bgzf_unwrap" in mappy_rs.__all__
