"""Result sets for the PAF writer's tests (tests/test_paf_host.py on the CPU, tests/test_gpu_paf.py on the device): random mm355_hits_t
contents with tags rows, built the way tests/test_tags_host.py::records builds its records, the text mappy_rs.paf_line makes of them, the
ctypes record mm355_paf_format takes and the byte stream tests/host_harness/paf_host.cpp reads."""
import ctypes as C

import numpy as np

EEMPTY = -6
CIGAR_COUNTS = (0, 1, 63, 64, 65, 129, 4097)
CONTIGS = ["c", "chr2", "n" * 255]                      # names of 1 and 255 bytes
_CHARS = np.frombuffer(b"acgtn:*+-~0123456789ACGT^", np.uint8)


def _dtypes():
    import mappy_rs
    return mappy_rs._HIT_DTYPE, mappy_rs._TAG_DTYPE


def make_set(rows, tags, has_cigar, hit_off, status, qlens, qnames, contigs, cigar=(), sbuf=b""):
    """rows / tags: dicts per hit (as tests/test_tags_host.py::records takes them)"""
    hd, td = _dtypes()
    ha, ta = np.zeros(len(rows), hd), np.zeros(len(rows), td)
    for i, r in enumerate(rows):
        ha[i]["cs_len"] = ha[i]["md_len"] = -1
        for k, v in r.items():
            ha[i][k] = v
    for i, r in enumerate(tags):
        for k, v in r.items():
            ta[i][k] = v
    return dict(hits=ha, tags=ta, has_cigar=bool(has_cigar), hit_off=np.asarray(hit_off, np.int64), status=np.asarray(status, np.int32),
                qlens=np.asarray(qlens, np.int32), qnames=list(qnames), contigs=list(contigs), cigar=np.asarray(cigar, np.uint32), sbuf=bytes(sbuf))


def handmade_sets():
    """the four hand-made records of tests/test_tags_host.py (its rows, its tags, its names)"""
    from test_tags_host import CHAIN_ROW, CIGAR_ROW, CIG
    two = ["chr1", "chr2"]
    f32 = np.float32
    # (that test gives its inversion rows one CIGAR word and leaves n_cigar at 7: the numpy slice stops at the arena's end.  The C-ABI
    # refuses a row that points past its arena, so the rows say 1 here: the same line, cg:Z:657M)
    row = dict(CIGAR_ROW, is_primary=1, mapq=13, cs_len=-1, match_len=657, NM=0, n_cigar=1)
    return [
        make_set([CHAIN_ROW], [dict(score=1690, div=f32(0.0312), rep_len=37, flags=2)], False, [0, 1], [0], [5000], ["read1"], two),
        make_set([CHAIN_ROW, dict(CHAIN_ROW, is_primary=0), CHAIN_ROW],
                 [dict(score=1700, div=0.0, rep_len=0, flags=0), dict(score=900, div=-1.0, rep_len=0), dict(score=5, div=1.5, rep_len=0)],
                 False, [0, 3], [0], [5000], ["r"], two),
        make_set([CIGAR_ROW], [dict(score=598, div=f32(0.04), rep_len=120, n_ambi=1, n_gap=8, n_gapo=3, flags=0)], True, [0, 1], [0], [700], ["q7"],
                 two, cigar=CIG, sbuf=b":200+ac:3\0"),
        make_set([row, dict(row, is_primary=0), row],
                 [dict(score=0, div=-1.0, rep_len=9, flags=1), dict(score=0, div=-1.0, rep_len=9, flags=1),
                  dict(score=300, div=f32(0.01), rep_len=9, flags=2 | 1 << 2)], True, [0, 3], [0], [700], ["q"], two, cigar=[657 << 4]),
    ]


def _i32(rng, wide):
    """mostly small values, sometimes the ends of the range"""
    if wide and rng.random() < 0.1:
        return int(rng.choice([0, -1, 2**31 - 1, -2**31, 10**9, -10**9, 999999999, 9, 10]))
    return int(rng.integers(0, 10 ** int(rng.integers(1, 7))))


def random_set(rng, contigs=CONTIGS, n_cigar_ops=None, max_reads=4):
    """one random result set.  n_cigar_ops: operations of its first hit's CIGAR (None: a small random number)"""
    has_cigar = bool(rng.integers(0, 2)) or n_cigar_ops is not None
    n_reads = int(rng.integers(1, max_reads + 1))
    rows, tags, cigar, hit_off, status, qlens, qnames = [], [], [], [0], [], [], []
    sbuf = bytearray()
    for i in range(n_reads):
        kind = rng.random()
        if n_cigar_ops is not None and i == 0:
            kind = 0.5 + kind / 2                                   # the read that carries the forced CIGAR has hits
        n_hits = 0 if kind < 0.2 else int(rng.integers(1, 4))       # (an empty read -- kind < 0.08 -- never has any)
        status.append(EEMPTY if kind < 0.08 else 0)
        qlens.append(0 if kind < 0.08 else _i32(rng, False) + 1)
        qnames.append(None if rng.random() < 0.15 else str(rng.choice(["r%d" % i, "x", "q" * 255, "read %d comment" % i, "tab\there", "a b c"])))
        rep_len = _i32(rng, False)
        for j in range(n_hits):
            blen = _i32(rng, False) + 1
            mlen = int(rng.integers(0, blen + 1))
            n_gap = int(rng.integers(0, blen // 2 + 1)) if has_cigar else 0
            n_gapo = int(rng.integers(0, n_gap + 1))
            r = dict(query_start=_i32(rng, True), query_end=_i32(rng, True), strand=int(rng.choice([1, -1])), rid=int(rng.integers(0, len(contigs))),
                     target_len=_i32(rng, True), target_start=_i32(rng, True), target_end=_i32(rng, True), match_len=mlen, block_len=blen,
                     mapq=int(rng.choice([0, 60, 255, 2**32 - 1, int(rng.integers(0, 61))])), is_primary=int(rng.integers(0, 2)),
                     NM=_i32(rng, True), score0=_i32(rng, True), cnt=_i32(rng, True), subsc=_i32(rng, True), dp_max=_i32(rng, True),
                     dp_score=_i32(rng, True), dp_max2=_i32(rng, True), n_sub=_i32(rng, False))
            if has_cigar:
                nc = n_cigar_ops if (n_cigar_ops is not None and i == 0 and j == 0) else int(rng.choice([0, 1, 2, 3, 7, 20]))
                ops = np.arange(nc) % 9 if nc >= 9 else rng.integers(0, 9, nc)            # all nine operation codes
                digits = rng.integers(1, 10, nc)
                lens = np.minimum((10.0 ** digits * rng.random(nc)).astype(np.int64), 2**28 - 1)
                if nc:
                    lens[rng.integers(0, nc)] = int(rng.choice([0, 9, 10, 2**28 - 1, 99999999, 100000000]))
                r.update(n_cigar=nc, cigar_off=len(cigar))
                cigar += (lens << 4 | ops).astype(np.int64).tolist()
                for key in ("cs", "md"):
                    if rng.random() < 0.6:
                        ln = int(rng.choice([0, 1, 5, 64, 65, 300]))
                        r[key + "_off"], r[key + "_len"] = len(sbuf), ln
                        sbuf += _CHARS[rng.integers(0, len(_CHARS), ln)].tobytes() + b"\0"
            rows.append(r)
            tags.append(dict(score=_i32(rng, True), div=np.float32(rng.choice([-1.0, 0.0, 1.5, 1.0, rng.random(), rng.random() * 0.1])),
                             rep_len=rep_len, n_ambi=int(rng.integers(0, 5)) if has_cigar else 0, n_gap=n_gap, n_gapo=n_gapo,
                             flags=int(rng.integers(0, 16))))
        hit_off.append(len(rows))
    return make_set(rows, tags, has_cigar, hit_off, status, qlens, qnames, contigs, cigar=cigar, sbuf=sbuf)


def random_sets(seed, n, contigs=CONTIGS):
    """n random sets; every CIGAR length of CIGAR_COUNTS occurs several times, both modes, reads without hits, empty reads, unnamed reads"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        forced = CIGAR_COUNTS[k % 40] if k % 40 < len(CIGAR_COUNTS) else None
        out.append(random_set(rng, contigs, forced))
    return out


def hits_struct(s):
    """the set as the ctypes record mm355_paf_format takes -> (Hits, qnames char**, qlens int32*, keepalive)"""
    from mappy_rs import _ffi
    n, nr = len(s["hits"]), len(s["qlens"])
    hbuf = C.create_string_buffer(s["hits"].view("u1").tobytes(), max(1, n * s["hits"].itemsize))
    tbuf = C.create_string_buffer(s["tags"].view("u1").tobytes(), max(1, n * s["tags"].itemsize))
    cg = (C.c_uint32 * max(1, len(s["cigar"])))(*s["cigar"].tolist())
    sb = C.create_string_buffer(s["sbuf"], max(1, len(s["sbuf"])))
    off = (C.c_int64 * (nr + 1))(*s["hit_off"].tolist())
    st = (C.c_int32 * max(1, nr))(*s["status"].tolist())
    h = _ffi.Hits(n_reads=nr, hit_off=off, status=st, hits=C.cast(hbuf, C.POINTER(_ffi.Hit)), cigar=cg, str=C.cast(sb, C.POINTER(C.c_char)),
                  n_hits=n, n_cigar=len(s["cigar"]), n_str=len(s["sbuf"]), tags=C.cast(tbuf, C.POINTER(_ffi.Tags)))
    qn = (C.c_char_p * max(1, nr))(*[None if q is None else q.encode() for q in s["qnames"]])
    ql = (C.c_int32 * max(1, nr))(*s["qlens"].tolist())
    return h, qn, ql, (hbuf, tbuf, cg, sb, off, st)


def printed_name(q):
    """the query name as the line prints it"""
    return "*" if q is None else q.replace("\t", " ").split(" ")[0]


def expected(s):
    """(text, line_off) of the set: paf_line over the Mapping records of the same arrays, a line per hit in row order"""
    import mappy_rs
    h, _, _, keep = hits_struct(s)
    nr = len(s["qlens"])
    recs = mappy_rs._batch_to_mappings(C.pointer(h), nr, s["contigs"], chain_only=not s["has_cigar"])
    text, line_off = [], [0]
    for i in range(nr):
        if isinstance(recs[i], list):
            text += [mappy_rs.paf_line(m, printed_name(s["qnames"][i]), int(s["qlens"][i])) + "\n" for m in recs[i]]
        line_off.append(sum(map(len, text)))
    return "".join(text).encode(), line_off


def serialize(sets):
    """the byte stream `paf_host sets` reads"""
    out = []
    for s in sets:
        cb = b"".join(c.encode() + b"\0" for c in s["contigs"])
        qb = b"".join(q.encode() + b"\0" for q in s["qnames"] if q is not None)
        nr = len(s["qlens"])
        out.append(np.array([nr, len(s["hits"]), len(s["cigar"]), len(s["sbuf"]), int(s["has_cigar"]), len(s["contigs"]), len(cb), len(qb)],
                            np.int64).tobytes())
        out += [s["hit_off"].tobytes(), s["status"].tobytes(), s["qlens"].tobytes(), bytes(int(q is not None) for q in s["qnames"]),
                s["hits"].view("u1").tobytes(), s["tags"].view("u1").tobytes(), s["cigar"].tobytes(), s["sbuf"], cb, qb]
    return b"".join(out)
