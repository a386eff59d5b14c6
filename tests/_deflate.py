"""What the deflate tests share (tests/test_deflate_host.py, tests/test_gpu_deflate.py): the payloads at which each part of the coder of
mappy-rs_amd/csrc/mm355_deflate.h can go wrong, a BGZF stream cut into its blocks by BSIZE and checked against Python's zlib, and the cost of
an optimal Huffman code of a payload's bytes."""
import gzip
import heapq
import random
import struct
import zlib

import numpy as np

import _bam
import _bam_sets as BS

P = _bam.PAYLOAD
HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + 258 * 7     # block header, every code-length code length, 257 + 1 lengths of 7 bits: 1880
_CACHE = {}


def _shuffled(data, seed):
    v = list(data)
    random.Random(seed).shuffle(v)
    return bytes(v)


def _period(rng, n):
    return (rng.integers(0, 256, n, dtype=np.uint8).tobytes() * 3)[:P]


def record_stream():
    """the unframed records of constructed result sets, a few blocks"""
    return b"".join(r for s in BS.random_sets(4711, 60) for r in BS.expected(s)[0])


def payloads():
    """name -> bytes, made once.  Lengths below, at and above the minimum match and the longest match, each side of a block and several
    blocks; one byte value; all values in equal numbers (in order: matches everywhere; shuffled: none); Fibonacci counts over 22 values
    (46 367 bytes: an unlimited Huffman tree is 21 deep); random bytes; a random 1000-byte string repeated; periods of the longest legal
    distance and one beyond; a record stream"""
    if _CACHE:
        return _CACHE
    rng = np.random.default_rng(20)
    for n in (0, 1, 2, 3, 4, 257, 258, 259, P - 1, P, P + 1, 3 * P + 77):
        _CACHE["random_%d" % n] = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        _CACHE["zeros_%d" % n] = bytes(n)
        _CACHE["text_%d" % n] = (b":12*ag=ACGTTGCA+acgt-tt:7NM\x03ms\x2c" * (n // 27 + 1))[:n]
    _CACHE["ff_%d" % P] = b"\xff" * P
    _CACHE["ff_259"] = b"\xff" * 259
    _CACHE["equal_in_order"] = bytes(range(256)) * 255
    _CACHE["equal_shuffled"] = _shuffled(_CACHE["equal_in_order"], 5)
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    _CACHE["fibonacci"] = _shuffled(b"".join(bytes([40 + i]) * c for i, c in enumerate(fib)), 6)
    assert len(_CACHE["fibonacci"]) == 46367
    # with the end-of-block symbol's count of 1 beside the two 1s of that payload, the merges tie and a Huffman tree of it may be 12 or 22
    # deep, as the coder breaks the ties.  Counts 1 2 3 5 ... over 21 values (46 366 bytes) and the end-of-block 1 are the strict Fibonacci
    # row: every next count exceeds the sum of all before it by one, so every Huffman tree of it is a chain 21 deep and the limit must act
    _CACHE["fibonacci_deep"] = _shuffled(b"".join(bytes([40 + i]) * c for i, c in enumerate(fib[1:])), 7)
    assert len(_CACHE["fibonacci_deep"]) == 46366
    _CACHE["repeat_1000"] = (rng.integers(0, 256, 1000, dtype=np.uint8).tobytes() * 66)[:P]
    _CACHE["period_32768"] = _period(rng, 32768)
    _CACHE["period_32769"] = _period(rng, 32769)
    _CACHE["records"] = record_stream()
    assert len(_CACHE["records"]) > 2 * P
    return _CACHE


def mixed_blocks():
    """five blocks that alternate text-like and random and a tail of one byte: deflated and stored blocks mix, and no block begins at a
    multiple of anything"""
    rng = np.random.default_rng(21)
    text = (b"cs:Z::" + b"".join(b":%d*%c%c" % (rng.integers(1, 400), b"acgt"[rng.integers(4)], b"acgt"[rng.integers(4)]) for _ in range(12000)))
    out = b""
    for k in range(5):
        out += text[k * 1000:k * 1000 + P] if k % 2 == 0 else rng.integers(0, 256, P, dtype=np.uint8).tobytes()
    assert len(out) == 5 * P
    return out + b"\x07"


def blocks(bgzf):
    """a BGZF stream cut by BSIZE"""
    out, at = [], 0
    while at < len(bgzf):
        assert bgzf[at:at + 16] == bytes.fromhex("1f8b08040000000000ff060042430200"), at
        n = struct.unpack_from("<H", bgzf, at + 16)[0] + 1
        assert at + n <= len(bgzf)
        out.append(bgzf[at:at + n])
        at += n
    return out


def check(bgzf, data):
    """every block of `bgzf` inflates to its payload of `data` with the right CRC-32, ISIZE and BSIZE, none is longer than its stored form, and
    gzip reads the whole; returns per block whether it is stored"""
    bl = blocks(bgzf)
    assert len(bl) == (len(data) + P - 1) // P
    stored = []
    for k, b in enumerate(bl):
        p = data[k * P:(k + 1) * P]
        assert zlib.decompress(b[18:-8], -15) == p, k
        assert struct.unpack("<II", b[-8:]) == (zlib.crc32(p), len(p)), k
        assert len(b) <= len(p) + 31, (k, len(b), len(p))
        stored.append(b == _bam.frame(p))
        assert stored[-1] or ((b[18] & 7) == 5 and len(b) < len(p) + 31), k       # BFINAL, BTYPE 10; a deflated block is shorter
    assert (gzip.decompress(bgzf) if data else bgzf) == data
    return stored


def huffman(payload):
    """(bits, depth) of an optimal Huffman code of the payload's bytes and one end-of-block symbol"""
    count = {}
    for c in payload:
        count[c] = count.get(c, 0) + 1
    count[256] = 1
    heap = [(n, s, (s,)) for s, n in sorted(count.items())]
    depth = dict.fromkeys(count, 0)
    heapq.heapify(heap)
    tie = 1000
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        tie += 1
        heapq.heappush(heap, (a[0] + b[0], tie, a[2] + b[2]))
    if len(count) == 1:
        depth[256] = 1
    return sum(count[s] * depth[s] for s in count), max(depth.values())
