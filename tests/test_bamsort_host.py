"""Coordinate-sorted BAM on the host: the key, the serial sort, the check of a caller's stream and the merge's copy loop of
mappy-rs_amd/csrc/mm355_bamsort.h, built with g++ under AddressSanitizer and UBSan into a stand-alone program
(tests/host_harness/bamsort_host.cpp), against the model of tests/_bamsort.py; and, in process through the library, the headers that say
SO:coordinate and mm355_bam_sort on the host.  GPU side: tests/test_gpu_bamsort.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import _bam
import _bamsort as BS
import _capi
import synthdata as S

EINVAL = -2


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bamsort_host") / "bamsort_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(_capi.HERE, "host_harness", "bamsort_host.cpp"), "-o", exe, "-lpthread"])
    return exe


def _run(exe, mode, blob, tmp_path, tag):
    src, dst = tmp_path / (tag + ".bin"), tmp_path / (tag + ".out")
    src.write_bytes(blob)
    r = subprocess.run([exe, mode, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.split(), dst.read_bytes()


# ---------------------------------------------------------------- the key
def test_key_on_hand_written_records(harness, tmp_path):
    """records spelled out in hex: block_size, refID, pos, l_read_name mapq bin, n_cigar_op flag, l_seq, next_refID, next_pos, tlen, name"""
    tail = "00000000" "ffffffff" "ffffffff" "00000000" "6100"            # l_seq 0, no mate, tlen 0, "a"
    def rec(refid, pos, flag):
        return bytes.fromhex("22000000" + refid + pos + "02" "00" "4812" + "0000" + flag + tail)
    cases = [
        (rec("00000000", "00000000", "0000"), 0 << 32 | 1 << 1 | 0),
        (rec("00000000", "00000000", "1000"), 0 << 32 | 1 << 1 | 1),
        (rec("05000000", "00000000", "1001"), 5 << 32 | 1 << 1 | 1),                 # flag 0x110: secondary on the reverse strand
        (rec("05000000", "feffff7f", "0000"), 5 << 32 | (2**31 - 1) << 1 | 0),       # pos 2^31 - 2: the low word is 0xfffffffe
        (rec("05000000", "feffff7f", "1000"), 5 << 32 | 0xfffffffe | 1),
        (rec("ffffffff", "ffffffff", "0400"), 0xffffffff << 32),                     # the unmapped record: pos -1, low word 0
        (rec("ffffffff", "00000000", "0400"), 0xffffffff << 32 | 2),
        (rec("00000000", "ffffffff", "0400"), 0),                                    # unmapped flag on a placed record: the flag's bit 4 alone counts
    ]
    assert all(len(r) == 38 and BS.key_of(r) == k for r, k in cases)
    out, got = _run(harness, "key", b"".join(struct.pack("<i", len(r)) + r for r, _ in cases), tmp_path, "key")
    assert out == ["key", str(len(cases))] and list(struct.unpack("<%dQ" % len(cases), got)) == [k for _, k in cases]
    ks = [k for _, k in cases]
    assert ks[0] < ks[1] < ks[2] < ks[3] < ks[4] < ks[5] < ks[6]                      # contig, position, strand; no contig last


# ---------------------------------------------------------------- the serial sort
def _sort_blob(streams):
    """(the harness reads n_bytes bytes of a stream: a count that disagrees with the data gets the data cut or padded to it)"""
    return b"".join(struct.pack("<qqq", n_rec, n_bytes, len(off)) + np.asarray(off, np.int64).tobytes() + data[:max(n_bytes, 0)].ljust(max(n_bytes, 0), b"\0")
                    for data, off, n_rec, n_bytes in streams)


def _sorted_results(got, streams):
    """per stream None (refused) or (keys, offsets, bytes)"""
    out, at = [], 0
    for data, off, n_rec, n_bytes in streams:
        rc, = struct.unpack_from("<i", got, at)
        at += 4
        assert rc in (0, EINVAL)
        if rc:
            out.append(None)
            continue
        keys = list(struct.unpack_from("<%dQ" % n_rec, got, at)); at += 8 * n_rec
        noff = list(struct.unpack_from("<%dq" % (n_rec + 1), got, at)); at += 8 * (n_rec + 1)
        out.append((keys, noff, got[at:at + n_bytes])); at += n_bytes
    assert at == len(got)
    return out


def test_host_sort_is_pythons_stable_sort(harness, tmp_path):
    rng = np.random.default_rng(41)
    streams, want = [], []
    for n in (0, 1, 2, 257, 1500):
        for name, fields in BS.patterns(n, rng).items():
            recs = BS.records_for(fields, rng, big=n == 257)
            data, off = BS.stream(recs)
            streams.append((data, off, n, len(data)))
            srt, keys = BS.model(recs)
            want.append((keys, list(BS.stream(srt)[1]), b"".join(srt)))
            if name == "equal":
                assert srt == recs
            if name == "descending" and n > 1:
                assert srt == recs[::-1]
    out, got = _run(harness, "sort", _sort_blob(streams), tmp_path, "sort")
    assert out == ["sort", str(len(streams))]
    res = _sorted_results(got, streams)
    for k, (g, w) in enumerate(zip(res, want)):
        assert g == w, k
        assert g[0] == sorted(g[0])


def _refused_streams():
    rng = np.random.default_rng(43)
    recs = BS.records_for(BS.patterns(6, rng)["random3"], rng)
    data, off = BS.stream(recs)
    n, nb = len(recs), len(data)
    def with_off(i, v):
        o = off.copy(); o[i] = v
        return o
    short = BS.record(0, 1, 0)[:36]
    short = struct.pack("<I", 32) + short[4:]                                # 36 bytes whose block_size agrees: shorter than any record
    lying = bytearray(data); lying[int(off[2])] ^= 1                         # a block_size that is not the piece's length
    cases = {
        "first offset not 0": (data, with_off(0, 1), n, nb),
        "last offset short of the bytes": (data, off, n, nb + 1),
        "last offset past the bytes": (data, off, n, nb - 1),
        "offsets descend": (data, with_off(3, int(off[2]) - 1), n, nb),
        "offsets repeat": (data, with_off(3, int(off[2])), n, nb),
        "negative offset": (data, with_off(1, -5), n, nb),
        "a piece of 36 bytes": (short, np.array([0, 36], np.int64), 1, 36),
        "block_size disagrees": (bytes(lying), off, n, nb),
        "block_size of the whole stream in record 0": (struct.pack("<I", nb - 4) + data[4:], off, n, nb),
        "negative count": (data, off, -1, nb),
        "negative bytes": (b"", np.array([0], np.int64), 0, -1),
        "bytes without records": (data, np.array([0], np.int64), 0, nb),
    }
    return cases, (data, off, n, nb)


def test_each_refusal_of_the_stream_check(harness, tmp_path):
    cases, good = _refused_streams()
    streams = [good] + list(cases.values()) + [(b"", np.array([0], np.int64), 0, 0)]
    out, got = _run(harness, "sort", _sort_blob(streams), tmp_path, "refuse")
    res = _sorted_results(got, streams)
    assert res[0] is not None and res[-1] == ([], [0], b"")
    assert [r is None for r in res[1:-1]] == [True] * len(cases), [n for n, r in zip(cases, res[1:-1]) if r is not None]


# ---------------------------------------------------------------- the merge's copy loop
def test_gather_checks_every_piece_before_it_copies(harness, tmp_path):
    rng = np.random.default_rng(47)
    base = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
    cases = [                                           # (src_off, len, out_cap) -> accepted?
        ([0, 990, 500], [10, 10, 0], 20, True),         # a piece that touches base_len, a total that touches out_cap
        ([1000], [0], 0, True),                         # an empty piece at the very end
        ([0, 991], [10, 10], 20, False),                # one byte past base_len
        ([1001], [0], 0, False),
        ([0, 10], [10, 11], 20, False),                 # one byte past out_cap
        ([5, -1], [5, 1], 20, False), ([5, 6], [5, -1], 20, False),
        ([0], [2**62], 2**62, False), ([2**62], [2**62], 20, False),          # sums that would wrap
        ([990, 0, 990, 3], [10, 1000, 10, 7], 1027, True),                    # overlapping pieces are the caller's business
        ([], [], 0, True),
    ]
    blob = b""
    for src, ln, cap, _ in cases:
        blob += struct.pack("<qqq", len(base), min(cap, 4096), len(src)) + np.array(src, np.int64).tobytes() + np.array(ln, np.int64).tobytes() + base
    out, got = _run(harness, "gather", blob, tmp_path, "gather")
    assert out == ["gather", str(len(cases))]
    at = 0
    for k, (src, ln, cap, ok) in enumerate(cases):
        rc, tot = struct.unpack_from("<iq", got, at)
        at += 12
        assert (rc == 0) == ok and rc in (0, EINVAL), k
        if ok:
            want = b"".join(base[s:s + l] for s, l in zip(src, ln))
            assert tot == len(want) and got[at:at + tot] == want, k
            at += tot
        else:
            assert tot == 0
    assert at == len(got)


# ---------------------------------------------------------------- in process: the headers, and the stage on the host
@pytest.fixture(scope="module")
def aligner(built, tmp_path_factory):
    import mappy_rs
    fa = str(tmp_path_factory.mktemp("bamsort") / "two.fa")
    S.write_fasta(fa, S.make_genome(7, [4000, 3000]), ["chrA", "chrB"])
    return mappy_rs.Aligner(fa, preset="map-ont")


def test_headers_say_coordinate(aligner):
    import gzip
    al = aligner
    plain, srt = al.sam_header(), al.sam_header(sort=True)
    assert plain.startswith(b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n") and al.sam_header(sort=False) == plain and al.sam_header(b"") == plain
    assert srt.split(b"\n", 1) == [b"@HD\tVN:1.6\tSO:coordinate", plain.split(b"\n", 1)[1]]
    rg = b"@RG\tID:x\n"
    assert al.sam_header(rg, sort=True) == srt.replace(b"@PG", rg + b"@PG")
    for compress in (False, True):
        assert al.bam_header(compress, sort=False) == al.bam_header(compress) == al.bam_header(compress=compress)
        data = gzip.decompress(al.bam_header(compress, rg, sort=True))
        text = al.sam_header(rg, sort=True)
        assert data[:4] == b"BAM\1" and data[8:8 + len(text)] == text and struct.unpack_from("<I", data, 4)[0] == len(text)
        assert gzip.decompress(al.bam_header(compress, rg))[8 + len(al.sam_header(rg)):] == data[8 + len(text):]      # the contigs behind either text
    with pytest.raises(TypeError):
        al.sam_header(b"", True)                        # keyword-only
    with pytest.raises(TypeError):
        al.bam_header(False, b"", True)


def _stage(L, ctx, data, off, n_rec, where, n_bytes=None):
    """mm355_bam_sort -> (rec, keys, offsets, on_device), or the return code alone"""
    from mappy_rs import _ffi
    rp = C.POINTER(_ffi.Run)()
    off = np.ascontiguousarray(off, np.int64)
    rc = L.mm355_bam_sort(ctx, data, len(data) if n_bytes is None else n_bytes, off.ctypes.data, n_rec, where, C.byref(rp))
    if rc:
        assert not rp
        return rc
    try:
        r = rp.contents
        n = int(r.n_rec)
        assert r.n_bytes == len(data)
        return (C.string_at(r.rec, r.n_bytes), [int(r.key[i]) for i in range(n)], [int(r.rec_off[i]) for i in range(n + 1)], int(r.on_device))
    finally:
        L.mm355_free_run(rp)


def test_stage_on_the_host_through_the_library(built):
    from mappy_rs import _ffi
    L = _ffi.lib()
    rng = np.random.default_rng(53)
    for n in (0, 1, 2, 300):
        for name, fields in BS.patterns(n, rng).items():
            recs = BS.records_for(fields, rng, big=n == 300)
            data, off = BS.stream(recs)
            srt, keys = BS.model(recs)
            for where in (_ffi.PAF_HOST, _ffi.PAF_AUTO):           # (AUTO is the host: no context needed)
                assert _stage(L, None, data, off, n, where) == (b"".join(srt), keys, list(BS.stream(srt)[1]), 0), (n, name)
    cases, (data, off, n, nb) = _refused_streams()
    for name, (d, o, k, b) in cases.items():
        assert _stage(L, None, d, o, k, _ffi.PAF_HOST, n_bytes=b) == EINVAL, name
    assert _stage(L, None, data, off, n, 3) == EINVAL and _stage(L, None, data, off, n, -1) == EINVAL
    assert _stage(L, None, data, off, n, _ffi.PAF_DEVICE) == EINVAL          # the device needs a context
    assert _stage(L, None, data, off, n, _ffi.PAF_HOST)[0] == b"".join(BS.model(_bam.cut(data))[0])
