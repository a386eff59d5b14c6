"""Result sets for the SAM writer's tests (tests/test_sam_host.py on the CPU, tests/test_gpu_sam.py on the device): random mm355_hits_t
contents with tags rows whose coordinates are consistent with the read's length (a SAM line slices the read by them), the reads and quality
strings themselves, the text mappy_rs.sam_lines makes of them, the ctypes arguments mm355_sam_format takes and the byte stream
tests/host_harness/sam_host.cpp reads.  A set is a tests/_paf_sets.py set with four more keys: seqs, quals, rep_len, sam_flags."""
import ctypes as C

import numpy as np

import _paf_sets as PS

EEMPTY = PS.EEMPTY
CONTIGS = PS.CONTIGS
SOFTCLIP, HIT_ONLY = 1, 2
TILE = 4096                                             # SAM_TILE of mm355_sam.hip: output bytes of one copy block
LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
_BASES = np.frombuffer(b"ACGTACGTACGTNacgtnRYKMBVDHSWUurykmbvdhswX*", np.uint8)
_QUALS = np.arange(33, 127, dtype=np.uint8)
_CHARS = np.frombuffer(b"acgtn:*+-~0123456789ACGT^", np.uint8)


def make_set(rows, tags, hit_off, status, qnames, seqs, quals, rep_len, sam_flags=0, contigs=CONTIGS, cigar=(), sbuf=b""):
    s = PS.make_set(rows, tags, True, hit_off, status, [len(x) for x in seqs], qnames, contigs, cigar=cigar, sbuf=sbuf)
    s.update(seqs=list(seqs), quals=list(quals), rep_len=np.asarray(rep_len, np.int32), sam_flags=int(sam_flags))
    return s


def random_read(rng, qlen, with_qual=True):
    seq = _BASES[rng.integers(0, len(_BASES), qlen)].tobytes().decode()
    return seq, (_QUALS[rng.integers(0, len(_QUALS), qlen)].tobytes().decode() if with_qual else None)


def random_row(rng, qlen, contigs, cigar, sbuf, n_cigar=None, kind=None):
    """one row and its tags row on a read of qlen bases; kind: 0 primary with sam_pri, 1 supplementary, 2 secondary, None: any"""
    qs = int(rng.integers(0, qlen + 1)) if rng.random() < 0.8 else 0
    qe = int(rng.integers(qs, qlen + 1)) if rng.random() < 0.8 else qlen
    ts = int(rng.choice([0, 9, 2**31 - 1, int(rng.integers(0, 10**6))])) if rng.random() < 0.3 else int(rng.integers(0, 10**6))
    tl = int(rng.choice([qe - qs, max(0, qe - qs - int(rng.integers(0, 50))), qe - qs + int(rng.integers(0, 50))]))
    te = min(ts + tl, 2**31 - 1)
    blen = int(rng.integers(1, 10 ** int(rng.integers(1, 7))))
    n_gap = int(rng.integers(0, blen // 2 + 1))
    kind = int(rng.integers(0, 3)) if kind is None else kind
    nc = int(rng.choice([0, 1, 2, 3, 7, 20])) if n_cigar is None else n_cigar
    ops = np.arange(nc) % 9 if nc >= 9 else rng.integers(0, 9, nc)
    lens = np.minimum((10.0 ** rng.integers(1, 10, nc) * rng.random(nc)).astype(np.int64), 2**28 - 1)
    r = dict(query_start=qs, query_end=qe, strand=int(rng.choice([1, -1])), rid=int(rng.integers(0, len(contigs))), target_len=PS._i32(rng, True),
             target_start=ts, target_end=te, match_len=int(rng.integers(0, blen + 1)), block_len=blen,
             mapq=int(rng.choice([0, 60, 255, 2**32 - 1, int(rng.integers(0, 61))])), is_primary=int(kind != 2), NM=PS._i32(rng, True),
             score0=PS._i32(rng, True), cnt=PS._i32(rng, True), subsc=PS._i32(rng, True), dp_max=PS._i32(rng, True), dp_score=PS._i32(rng, True),
             n_cigar=nc, cigar_off=len(cigar))
    cigar += (lens << 4 | ops).astype(np.int64).tolist()
    for key in ("cs", "md"):
        if rng.random() < 0.5:
            ln = int(rng.choice([0, 1, 5, 64, 65, 300]))
            r[key + "_off"], r[key + "_len"] = len(sbuf), ln
            sbuf += _CHARS[rng.integers(0, len(_CHARS), ln)].tobytes() + b"\0"
    flags = int(rng.integers(0, 16)) & ~2 | (2 if kind == 0 or (kind == 2 and rng.random() < 0.5) else 0)
    t = dict(score=PS._i32(rng, True), div=-1.0, rep_len=0, n_ambi=int(rng.integers(0, 5)), n_gap=n_gap, n_gapo=int(rng.integers(0, n_gap + 1)), flags=flags)
    return r, t


def random_set(rng, contigs=CONTIGS, n_cigar_ops=None, qlen0=None, max_reads=4):
    """one random set.  n_cigar_ops / qlen0: CIGAR operations of the first row / length of the first read (None: random)"""
    n_reads = int(rng.integers(1, max_reads + 1))
    rows, tags, cigar, hit_off, status, qnames, seqs, quals, rep = [], [], [], [0], [], [], [], [], []
    sbuf = bytearray()
    for i in range(n_reads):
        kind = rng.random()
        if i == 0 and (n_cigar_ops is not None or qlen0 is not None):
            kind = 0.5 + kind / 2                                    # the read that carries the forced shape has rows
        empty = kind < 0.08
        qlen = 0 if empty else qlen0 if (i == 0 and qlen0 is not None) else int(rng.choice(LENGTHS)) if rng.random() < 0.5 else int(rng.integers(1, 400))
        n_rows = 0 if kind < 0.25 else int(rng.integers(1, 6))
        seq, qual = random_read(rng, qlen, rng.random() < 0.7)
        status.append(EEMPTY if empty else 0)
        seqs.append(seq); quals.append(qual)
        qnames.append(None if rng.random() < 0.15 else str(rng.choice(["r%d" % i, "x", "q" * 255, "read %d comment" % i, "tab\there", "a b c"])))
        rl = PS._i32(rng, False)
        rep.append(rl)
        for j in range(n_rows):
            r, t = random_row(rng, qlen, contigs, cigar, sbuf, n_cigar_ops if (i == 0 and j == 0 and n_cigar_ops is not None) else None)
            t["rep_len"] = rl
            rows.append(r); tags.append(t)
        hit_off.append(len(rows))
    return make_set(rows, tags, hit_off, status, qnames, seqs, quals, rep, int(rng.integers(0, 4)), contigs, cigar, sbuf)


def random_sets(seed, n, contigs=CONTIGS):
    """n random sets: every CIGAR count of _paf_sets.CIGAR_COUNTS and every length of LENGTHS is forced on a first read several times"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        forced = PS.CIGAR_COUNTS[k % 40] if k % 40 < len(PS.CIGAR_COUNTS) else None
        qlen0 = LENGTHS[k % 40 - 10] if 10 <= k % 40 < 10 + len(LENGTHS) else None
        out.append(random_set(rng, contigs, forced, qlen0))
    return out


def sam_args(s):
    """the set as the ctypes arguments of mm355_sam_format -> (Hits, qnames, seqs, qlens, quals, rep_len, keepalive)"""
    h, qn, ql, keep = PS.hits_struct(s)
    nr = len(s["seqs"])
    sb = [x.encode("latin-1") for x in s["seqs"]]
    qb = [None if q is None else q.encode("latin-1") for q in s["quals"]]
    sp = (C.c_char_p * max(1, nr))(*sb)
    qp = (C.c_char_p * max(1, nr))(*qb)
    rl = (C.c_int32 * max(1, nr))(*s["rep_len"].tolist())
    return h, qn, sp, ql, qp, rl, (keep, sb, qb)


def expected(s, sam_flags=None):
    """(text, line_off) of the set: sam_lines over the Mapping records of the same arrays"""
    import mappy_rs
    fl = s["sam_flags"] if sam_flags is None else sam_flags
    h, _, _, keep = PS.hits_struct(s)
    nr = len(s["seqs"])
    recs = mappy_rs._batch_to_mappings(C.pointer(h), nr, s["contigs"])
    text, line_off = [], [0]
    for i in range(nr):
        if isinstance(recs[i], list) and (recs[i] or (len(s["seqs"][i]) and not fl & HIT_ONLY)):
            text += [ln + "\n" for ln in mappy_rs.sam_lines(recs[i], s["qnames"][i], s["seqs"][i], s["quals"][i], softclip=bool(fl & SOFTCLIP),
                                                            rl=int(s["rep_len"][i]))]
        line_off.append(sum(len(t.encode("latin-1")) for t in text))
    return "".join(text).encode("latin-1"), line_off


def serialize(sets, has_cigar=True, drop_seq=None):
    """the byte stream `sam_host sets` / `sam_host check` reads.  drop_seq: index of a read handed over as a null pointer (check only)"""
    out = []
    for s in sets:
        cb = b"".join(c.encode() + b"\0" for c in s["contigs"])
        qb = b"".join(q.encode() + b"\0" for q in s["qnames"] if q is not None)
        sq = b"".join(x.encode("latin-1") for x in s["seqs"])
        ql = b"".join(q.encode("latin-1") for q in s["quals"] if q is not None)
        nr = len(s["seqs"])
        out.append(np.array([nr, len(s["hits"]), len(s["cigar"]), len(s["sbuf"]), int(has_cigar), len(s["contigs"]), len(cb), len(qb), len(sq), len(ql),
                             s["sam_flags"]], np.int64).tobytes())
        out += [s["hit_off"].tobytes(), s["status"].tobytes(), s["qlens"].tobytes(), s["rep_len"].tobytes(),
                bytes(int(q is not None) for q in s["qnames"]), bytes(int(q is not None) for q in s["quals"]),
                bytes(int(i != drop_seq) for i in range(nr)),
                s["hits"].view("u1").tobytes(), s["tags"].view("u1").tobytes(), s["cigar"].tobytes(), s["sbuf"], cb, qb, sq, ql]
    return b"".join(out)
