"""Synthetic coordinate-sorted BAM files for the index's tests (tests/test_bai_host.py, tests/test_gpu_bai.py): records with a CIGAR built
with struct, BGZF blocks of chosen payload sizes made with zlib, and the files whose records reach every branch of the builder."""
import struct
import zlib

import numpy as np

import _bam
import _bamsort as BS

M, I, D, N, S, H, P, EQ, X = range(9)


def rec(ref, pos, flag, words, name=b"r", size=None, rng=None):
    """a record (block_size included): the CIGAR words as given, `bin` left 0 (the index recomputes it), l_seq 0, and a Z tag that brings
    the record to `size` bytes"""
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) + 1, 0, 0, len(words), flag, 0, -1, -1, 0) + name + b"\0" + struct.pack("<%dI" % len(words), *words)
    if size is not None:
        pad = size - 4 - len(body) - 4
        assert pad >= 0, (size, len(body))
        fill = bytes(rng.integers(1, 256, pad, dtype=np.uint8)) if rng is not None else b"a" * pad
        body += b"xxZ" + fill + b"\0"
    return struct.pack("<I", len(body)) + body


def header(refs):
    text = b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in refs)
    return b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs)) + b"".join(
        struct.pack("<I", len(n) + 1) + n + b"\0" + struct.pack("<I", l) for n, l in refs)


def block(payload, level):
    z = zlib.compressobj(level, zlib.DEFLATED, -15)
    c = z.compress(payload) + z.flush()
    return (bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", len(c) + 25) + c + struct.pack("<II", zlib.crc32(payload), len(payload)))


def cuts_of(recs, mode):
    """payload sizes for the records' stream.  "plain": 0xff00 each; "odd": 40000 each with an empty block after the second; "records": a
    block ends wherever a record ends (records longer than a block are cut at 0xff00)"""
    total = sum(len(r) for r in recs)
    if mode == "plain":
        return [min(0xff00, total - a) for a in range(0, total, 0xff00)]
    if mode == "odd":
        out = [min(40000, total - a) for a in range(0, total, 40000)]
        return out[:2] + [0] + out[2:]
    out = []
    for r in recs:
        n = len(r)
        while n > 0xff00:
            out.append(0xff00); n -= 0xff00
        out.append(n)
    return out


def bam_file(refs, recs, mode="plain", level=0):
    """-> (the file's bytes, first_block_at, the sizes of the records' blocks)"""
    hd = _bam.frame(header(refs))
    data = b"".join(recs)
    blocks, at = [], 0
    for n in cuts_of(recs, mode):
        blocks.append(block(data[at:at + n], level))
        at += n
    assert at == len(data)
    return hd + b"".join(blocks) + _bam.EOF, len(hd), [len(b) for b in blocks]


def tables(recs):
    """what the builder takes: keys, spans, lengths (the span from the model)"""
    import _bai
    return (np.array([BS.key_of(r) for r in recs], np.uint64), np.array([_bai.span_of(r) for r in recs], np.int64), np.array([len(r) for r in recs], np.int64))


def sort_recs(recs):
    return BS.model(recs)[0]


REFS = [(b"chrA", 1 << 29), (b"chrEmpty", 5000), (b"chrB", 3000000)]


def files(rng):
    """name -> (refs, records in coordinate order, block mode, deflate level)"""
    out = {}
    # small: everything is within 64 KB of the file, so every bin cascades into bin 0 and its chunks merge; sparse positions back-fill windows
    small = []
    for i in range(400):
        ref = (0, 2)[i % 2]
        pos = int(rng.integers(0, 2900000))
        words = [int(rng.integers(1, 400)) << 4 | int(rng.integers(0, 9)) for _ in range(int(rng.integers(0, 6)))]
        flag = (0, 16, 0x100, 4)[int(rng.integers(0, 4))]
        small.append(rec(ref, pos, flag, words, b"s%d" % i, 80 + i % 90))
    small.append(rec(0, (1 << 29) - 50, 0, [50 << 4 | M], b"last_base"))                      # end == 2^29 exactly
    small += [rec(-1, -1, 4, [], b"u%d" % i, 60) for i in range(7)]
    out["small"] = (REFS, sort_recs(small), "records", 0)
    # big: a level-5 bin of 180 KB that stays, between two chunks of its parent that stay apart; far windows that cascade and merge
    big = [rec(0, 16000, 0, [1000 << 4 | M], b"A", 200),
           *[rec(0, 16384 + 100 * i, 0, [100 << 4 | M], b"Y%d" % i, 30000, rng) for i in range(6)],
           rec(0, 32000, 16, [1000 << 4 | M], b"B", 200),
           rec(0, 5000000, 0, [20 << 4 | M], b"far1", 100), rec(0, 5020000, 0, [20 << 4 | EQ, 5 << 4 | D, 3 << 4 | X], b"far2", 100),
           rec(0, 300000000, 0, [70000 << 4 | N, 10 << 4 | M], b"intron", 100),                # spans five windows
           *[rec(2, 1000 + 3000 * i, (0, 16)[i & 1], [2500 << 4 | M, 40 << 4 | S], b"c%d" % i, 150 + i, rng) for i in range(600)],
           *[rec(2, 2999000, 4, [30 << 4 | M], b"placed_unmapped%d" % i, 90) for i in range(3)],
           *[rec(-1, -1, 4, [], b"u%d" % i, 60) for i in range(5)]]
    out["big_stored"] = (REFS, sort_recs(big), "odd", 0)
    out["big_deflated"] = (REFS, sort_recs(big), "plain", 6)
    out["big_record_cuts"] = (REFS, sort_recs(big), "records", 1)
    out["unplaced_only"] = (REFS, [rec(-1, -1, 4, [], b"u%d" % i, 60 + i) for i in range(40)], "plain", 6)
    out["no_records"] = (REFS, [], "plain", 0)
    out["no_contigs"] = ([], [rec(-1, -1, 4, [], b"u", 50)], "plain", 0)
    return out
