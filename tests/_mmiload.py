"""What the .mmi loader tests share (the host walk of mm355_mmiwalk.h, the device loader of mm355_idxload.hip): the input files -- the
oracle's own dumps of the repeat-rich reference at the four settings, an MM_I_NO_SEQ file -- the layout of a file computed from
_mmi.parse_mmi, and the files that must be refused."""
import ctypes as C

import _mmi


def oracle_dump(fa, k, w, flag, path):
    """the oracle indexes the FASTA and writes its own .mmi (khash order inside a bucket) -> the file's bytes"""
    from oracle import oracle as O
    L = O.lib()
    io, mo = O.IdxOpt(), O.MapOpt()
    L.mmo_set_opt(None, C.byref(io), C.byref(mo))
    io.k, io.w, io.flag = k, w, flag
    idx = L.mmo_idx_load(str(fa).encode(), C.byref(io))
    assert idx
    try:
        assert L.mmo_idx_dump(idx, str(path).encode()) == 0
    finally:
        L.mmo_idx_destroy(idx)
    with open(path, "rb") as f:
        return f.read()


def no_seq(data):
    """the same index as an MM_I_NO_SEQ file: the flag set, the S section cut off"""
    m = _mmi.parse_mmi(data)
    raw = bytearray(data)
    raw[20:24] = (m["flag"] | 2).to_bytes(4, "little")
    return bytes(raw[:len(raw) - len(m["S"])])


def layout(data):
    """offsets computed on the Python side: dict off_buckets, off_S, buckets [(off, n, size)] (off of the bucket's int32 n), p_base and
    pair_base (exclusive prefix sums, one entry more than buckets), n_pos, n_distinct"""
    m = _mmi.parse_mmi(data)
    o = 24 + len(m["contig_raw"])
    lay = dict(m=m, off_buckets=o, buckets=[], p_base=[0], pair_base=[0])
    for p, pairs in m["buckets"]:
        lay["buckets"].append((o, len(p), len(pairs)))
        lay["p_base"].append(lay["p_base"][-1] + len(p)); lay["pair_base"].append(lay["pair_base"][-1] + len(pairs))
        o += 8 + 8 * len(p) + 16 * len(pairs)
    lay["off_S"] = o
    lay["n_pos"], lay["n_distinct"] = lay["p_base"][-1], lay["pair_base"][-1]
    assert o + len(m["S"]) == len(data)
    return lay


def bad_files(data):
    """[(what, bytes)]: the truncations and patches of a good file (with an S section and a bucket that has both p[] and pairs) that every
    loader must refuse as a bad file"""
    lay = layout(data)
    off, n, size = next(b for b in lay["buckets"] if b[1] >= 2 and b[2] >= 2)
    neg = bytearray(data); neg[off:off + 4] = (-1).to_bytes(4, "little", signed=True)
    b29 = bytearray(data); b29[12:16] = (29).to_bytes(4, "little")
    b28 = bytearray(data); b28[12:16] = (28).to_bytes(4, "little")       # within the header's ranges at k >= 14: 2^28 buckets the file cannot hold
    assert len(lay["m"]["S"]) > 8 and lay["m"]["contigs"][0][0] and lay["m"]["k"] >= 14
    return [
        ("cut inside the fixed header", data[:14]),
        ("cut inside a name", data[:24 + 3]),
        ("cut at a bucket header", data[:off + 2]),
        ("cut in the middle of a p[]", data[:off + 4 + 8 * (n // 2) + 3]),
        ("cut in the middle of the pairs", data[:off + 8 + 8 * n + 16 * (size // 2) + 8]),
        ("cut inside S", data[:lay["off_S"] + 6]),
        ("one byte short", data[:-1]),
        ("n = -1 in a bucket", bytes(neg)),
        ("b = 29 in the header", bytes(b29)),
        ("b = 28 in the header of a small file", bytes(b28)),
    ]
