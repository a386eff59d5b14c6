"""BAM aux blocks, stated independently of the library for the tests of the copied tags (tests/test_bamaux_host.py, tests/test_gpu_bamaux.py):
the bounded walk and the two-group split of include/mm355.h restated, a builder of blocks from (tag, type, value) tuples, with_aux, which
splices a block into a record of tests/_bam.py::record_of, and expected, the records of a result set of tests/_bam_sets.py with the tags
every record class carries."""
import struct

import numpy as np

import _bam
import _bam_sets as BS

SIZE = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}
FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f", "d": "d"}
B_SUBTYPES = "cCsSiIf"
MOD = (b"MM", b"ML", b"MN", b"Mm", b"Ml")                # index the bases of the read as sequenced
OWN = tuple(x.encode() for x in "NM ms AS nn tp cm s1 s2 de dv zd SA cs MD rl CG".split())   # the writer's own
LENGTHS = (0, 4, 15, 16, 17, 4095, 4096, 4097, 8193)     # around a 16-byte piece and around the bulk kernel's tile of 4096 bytes


def tag(name, typ, value):
    """one tag: value is a 1-byte bytes for A, a number for the scalar types, bytes without the NUL for Z / H, (subtype, list) for B"""
    head = name.encode() if isinstance(name, str) else name
    assert len(head) == 2
    if typ == "A":
        return head + b"A" + value
    if typ in FMT:
        return head + typ.encode() + struct.pack("<" + FMT[typ], value)
    if typ in "ZH":
        return head + typ.encode() + value + b"\0"
    sub, vals = value
    assert typ == "B" and sub in B_SUBTYPES
    return head + b"B" + sub.encode() + struct.pack("<I", len(vals)) + struct.pack("<%d%s" % (len(vals), FMT[sub]), *vals)


def block(tags):
    return b"".join(tag(*t) for t in tags)


def walk(aux):
    """the tags of the block as a list of bytes, or None for a block the walk refuses"""
    out, at, n = [], 0, len(aux)
    while at < n:
        if n - at < 3:
            return None
        t = chr(aux[at + 2])
        if t in SIZE:
            ln = 3 + SIZE[t]
        elif t in "ZH":
            nul = aux.find(b"\0", at + 3)
            if nul < 0:
                return None
            ln = nul + 1 - at
        elif t == "B":
            if n - at < 8 or chr(aux[at + 3]) not in B_SUBTYPES:
                return None
            ln = 8 + struct.unpack_from("<I", aux, at + 4)[0] * SIZE[chr(aux[at + 3])]     # (Python's integers do not wrap)
        else:
            return None
        if ln > n - at:
            return None
        out.append(aux[at:at + ln])
        at += ln
    return out


def keep_ok(keep):
    return keep == "*" or (len(keep) > 0 and len(keep) % 2 == 0)


def split(aux, keep="*"):
    """(kept bytes, mod_off), or None where mm355_bam_aux_split answers MM355_EINVAL"""
    tags = walk(aux)
    if tags is None or not keep_ok(keep):
        return None
    names = None if keep == "*" else {keep[i:i + 2].encode("latin-1") for i in range(0, len(keep), 2)}
    kept = [t for t in tags if t[:2] not in OWN and (names is None or t[:2] in names)]
    first = b"".join(t for t in kept if t[:2] not in MOD)
    return first + b"".join(t for t in kept if t[:2] in MOD), len(first)


def filler(n, rng=None):
    """a well-formed block of exactly n bytes whose tags are none of OWN and none of MOD: nothing, one A tag (n == 4), or one B:C tag
    (n >= 8)"""
    if n == 0:
        return b""
    assert n >= 4 and n not in (5, 6, 7)
    if n == 4:
        return tag("xa", "A", b"!")
    body = n - 8
    vals = (rng.integers(0, 256, body) if rng is not None else np.arange(body) % 251).astype(np.uint8).tolist()
    out = tag("xb", "B", ("C", vals))
    assert len(out) == n
    return out


def two_groups(n, rng, first=None):
    """a split block of exactly n bytes as (kept, mod_off): `first` bytes of filler (default: about half), then an ML:B:C tag"""
    if n < 12:
        return filler(n, rng), n
    first = (4 if n < 24 else n // 2) if first is None else first
    ml = tag("ML", "B", ("C", rng.integers(0, 256, n - first - 8).tolist()))
    return filler(first, rng) + ml, first


def mod_pair(n_bases, rng):
    """an MM:Z / ML:B:C pair as a basecaller writes it, of about n_bases / 2 bytes each"""
    n = max(1, n_bases // 4)
    mm = b"C+m?," + b",".join(b"%d" % x for x in rng.integers(0, 10, n)) + b";"
    return tag("MM", "Z", mm) + tag("ML", "B", ("C", rng.integers(0, 256, max(1, n_bases // 2)).tolist()))


def _tags_at(rec):
    l_name, n_cigar, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    return 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq


def with_aux(rec, aux):
    """the record (block_size included) with the block `aux` behind its own tags -- in front of a trailing CG -- and block_size fixed"""
    own = walk(rec[_tags_at(rec):])
    assert own is not None
    at = len(rec) - (len(own[-1]) if own and own[-1][:2] == b"CG" else 0)
    body = rec[4:at] + aux + rec[at:]
    return struct.pack("<I", len(body)) + body


def aux_of_record(rec, kept, mod_off, softclip):
    """what a record of this class carries of a read's split block: all of it where SEQ is the whole read, otherwise the first group"""
    flag = struct.unpack_from("<H", rec, 18)[0]
    return kept if flag & 0x900 == 0 or softclip else kept[:mod_off]


def expected(s, auxes, sam_flags=None):
    """(records, line_off) of the set as _bam_sets.expected gives them, every record with its read's tags; auxes: per read None or the
    (kept, mod_off) pair the formatter is given"""
    fl = s["sam_flags"] if sam_flags is None else sam_flags
    recs, off = BS.expected(s, sam_flags)
    starts = np.concatenate([[0], np.cumsum([len(r) for r in recs], dtype=np.int64)])[:-1]
    out, new_off, read = [], [0], 0
    for r, at in zip(recs, starts):
        while at >= off[read + 1]:
            read += 1
            new_off.append(sum(map(len, out)))
        a = auxes[read]
        out.append(r if a is None else with_aux(r, aux_of_record(r, a[0], a[1], bool(fl & 1))))
    while len(new_off) < len(off):
        new_off.append(sum(map(len, out)))
    return out, new_off


def serialize_aux(sets_auxes):
    """the aux side file of `bamaux_host sets` / `check`: per set, per read, four int32 -- aux_len, aux_mod, the bytes that follow, 1 for
    aux[i] == NULL -- and the bytes.  An entry is None, a (kept, mod_off) pair, or for the check a (len, mod, bytes or None) triple whose
    lengths need not be true"""
    out = []
    for auxes in sets_auxes:
        for a in auxes:
            ln, mod, data = (0, 0, None) if a is None else a if len(a) == 3 else (len(a[0]), a[1], a[0])
            out.append(struct.pack("<iiii", ln, mod, len(data or b""), int(data is None)) + (data or b""))
    return b"".join(out)


def aux_arrays(auxes):
    """per-read (kept, mod_off) or None -> the ctypes aux, aux_len, aux_mod arguments and what keeps them alive"""
    import ctypes as C
    n = max(1, len(auxes))
    bufs = [None if a is None else C.create_string_buffer(a[0], max(1, len(a[0]))) for a in auxes]
    ptr = (C.c_void_p * n)(*[None if b is None else C.addressof(b) for b in bufs])
    ln = (C.c_int32 * n)(*[0 if a is None else len(a[0]) for a in auxes])
    md = (C.c_int32 * n)(*[0 if a is None else a[1] for a in auxes])
    return ptr, ln, md, bufs
