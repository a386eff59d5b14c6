"""The coordinate order of BAM records, stated independently of the library for the sort's tests (tests/test_bamsort_host.py,
tests/test_gpu_bamsort.py): the key of include/mm355.h, records of a wanted size built with struct, the key patterns the tests cross with the
sizes, and the model -- Python's sorted() on (key, index), which is the stable sort."""
import struct

import numpy as np

BIG = (4095, 4096, 4097, 8193, 70000)          # around the permute kernel's tile, two tiles and a byte, more than a BGZF payload
MAX_POS = 2**31 - 2


def key_of(rec):
    refid, pos = struct.unpack_from("<ii", rec, 4)
    flag, = struct.unpack_from("<H", rec, 18)
    return (refid & 0xffffffff) << 32 | ((pos + 1) & 0xffffffff) << 1 & 0xffffffff | (flag >> 4 & 1)


def record(refid, pos, flag, name=b"", size=None, rng=None):
    """a record (block_size included) with these fields and a name of len(name) bytes plus its NUL; size: the record's bytes, reached with SEQ,
    QUAL and, where the rest is 1 mod 3, a four-byte tag (36 + len(name) + 1 is the smallest; a rest of exactly 1 cannot be filled)"""
    least = 37 + len(name)
    rest = 0 if size is None else size - least
    assert rest >= 0 and rest != 1, (size, least)
    aux = b""
    if rest % 3 == 1:
        aux, rest = b"xxAq", rest - 4
    l_seq = rest // 3 * 2 + (1 if rest % 3 == 2 else 0)
    assert (l_seq + 1) // 2 + l_seq == rest
    fill = bytes(rest) if rng is None else rng.integers(0, 256, rest, dtype=np.uint8).tobytes()
    body = struct.pack("<iiBBHHHIiii", refid, pos, len(name) + 1, 0, 4680, 0, flag, l_seq, -1, -1, 0) + name + b"\0" + fill + aux
    return struct.pack("<I", len(body)) + body


def stream(recs):
    """(the records back to back, their n + 1 offsets as int64)"""
    return b"".join(recs), np.cumsum([0] + [len(r) for r in recs], dtype=np.int64)


def model(recs):
    """(the records in coordinate order, ties in input order; their keys)"""
    keys = [key_of(r) for r in recs]
    order = sorted(range(len(recs)), key=lambda i: (keys[i], i))
    return [recs[i] for i in order], [keys[i] for i in order]


def patterns(n, rng):
    """name -> n (refID, pos, flag) triples"""
    return {
        "equal": [(1, 100, 0)] * n,                                                       # the stability case: output == input
        "descending": [(2, 3 * (n - i), 16 * (i & 1)) for i in range(n)],               # every record moves
        "ascending": [(0, 2 * i, 0) for i in range(n)],
        "random3": [(int(rng.integers(0, 3)), int(rng.integers(0, max(2, n // 8))), 16 * int(rng.integers(0, 2))) for _ in range(n)],
        "strands": [(0, 7, (16, 0, 0x110, 0x100)[i & 3]) for i in range(n)],                # forward and reverse at one position
        "unmapped": [(-1, -1, 4) if i & 1 else (1, 50 - i % 50, 0) for i in range(n)],
        "extremes": [(i % 2, MAX_POS if i % 3 == 0 else 0, 16 * (i % 5 == 0)) for i in range(n)],
    }


def records_for(fields, rng, big=False):
    """a record per triple: names of 0 .. 17 bytes in turn, so that records begin and end at every residue mod 16, sizes from the smallest
    up; big: the records at a few fixed places get the sizes of BIG"""
    recs = []
    n = len(fields)
    where = {(n * (2 * k + 1)) // (2 * len(BIG)): s for k, s in enumerate(BIG)} if big else {}
    for i, (refid, pos, flag) in enumerate(fields):
        name = b"n" * (i % 18)
        size = where.get(i)
        if size is None and i % 3:
            size = 37 + len(name) + (0, 2, 3, 30 + i % 40)[i % 4]
        if size is not None and (size - 37 - len(name)) == 1:
            name += b"m"
        recs.append(record(refid, pos, flag, name, size, rng))
    return recs
