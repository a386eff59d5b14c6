"""Result sets for the BAM writer's tests (tests/test_bam_host.py on the CPU, tests/test_gpu_bam.py on the device): the sets of
tests/_sam_sets.py made fit for BAM, and what tests/_bam.py::record_of makes of their SAM lines.  Fit for BAM means: mapq in 0..255 and
query names of at most 254 bytes (the writer refuses the rest: the sets for that are here too); `=` in the reads, which _sam_sets' alphabet
lacks; and no `*` in a read or a quality string -- a SEQ or QUAL field that is the one byte `*` is SAM's marker of a missing field, so the
line of a one-base read or slice could not say what the record holds (`.` stands in among the bases as the byte that is no code)."""
import numpy as np

import _bam
import _sam_sets as SS

EINVAL = -2


def scrub(s, rng):
    """the set `s` of _sam_sets made fit for BAM, in place"""
    s["hits"]["mapq"] %= 256
    s["qnames"] = [q if q is None or len(q) <= 254 else q[:254] for q in s["qnames"]]
    for i, seq in enumerate(s["seqs"]):
        b = np.frombuffer(seq.replace("*", ".").encode("latin-1"), np.uint8).copy()
        b[rng.random(len(b)) < 0.04] = ord("=")
        s["seqs"][i] = b.tobytes().decode("latin-1")
        if s["quals"][i] is not None:
            s["quals"][i] = s["quals"][i].replace("*", "+")
    return s


def random_sets(seed, n):
    rng = np.random.default_rng(seed + 1)
    return [scrub(s, rng) for s in SS.random_sets(seed, n)]


def expected(s, sam_flags=None):
    """(records, line_off) of the set: record_of over the lines of _sam_sets.expected; line_off counts bytes of the unframed stream"""
    text, text_off = SS.expected(s, sam_flags)
    recs = [_bam.record_of(ln, s["contigs"]) for ln in text.split(b"\n")[:-1]]
    n_before = [text[:o].count(b"\n") for o in text_off]
    sizes = np.concatenate([[0], np.cumsum([len(r) for r in recs], dtype=np.int64)])
    return recs, [int(sizes[k]) for k in n_before]


def long_cigar_set(n_words, rng, strand=1, n_reads=1):
    """a read of 300 bases whose first row has n_words CIGAR words including its two clips (the switch to the long form lies between 65535 and 65536);
    built directly as a result set: no read that long is needed"""
    rows, tags, cigar, hit_off, seqs, quals = [], [], [], [0], [], []
    for i in range(n_reads):
        seq, qual = SS.random_read(rng, 300)
        ops = (np.arange(n_words - 2) % 9).astype(np.int64)
        lens = rng.integers(0, 2000, n_words - 2)
        rows.append(dict(query_start=7, query_end=290, strand=strand, rid=1, target_len=10**9, target_start=12345, target_end=12345 + 283, match_len=200, block_len=283,
                         mapq=60, is_primary=1, n_cigar=n_words - 2, cigar_off=len(cigar)))
        tags.append(dict(score=99, flags=2))
        cigar += (lens << 4 | ops).tolist()
        hit_off.append(len(rows)); seqs.append(seq); quals.append(qual)
    rng2 = np.random.default_rng(1)
    return scrub(SS.make_set(rows, tags, hit_off, [0] * n_reads, ["long%d" % i for i in range(n_reads)], seqs, quals, [0] * n_reads, 0, cigar=cigar), rng2)


BOUNDS = (0, -1, 255, 256, 65535, 65536, -128, -129, -32768, -32769, 2**31 - 1, -2**31)


def boundary_set():
    """one read per value of BOUNDS, the value in every integer tag of its row: each side of every type boundary of htslib's smallest-type rule"""
    rows, tags, cigar = [], [], []
    for k, v in enumerate(BOUNDS):
        rows.append(dict(query_start=0, query_end=4, strand=1, rid=0, target_len=3000, target_start=k, target_end=k + 4, match_len=4, block_len=4, mapq=k, is_primary=1,
                         NM=v, dp_max=v, dp_score=v, cnt=v, subsc=v, n_cigar=1, cigar_off=k))
        tags.append(dict(score=v, rep_len=v, n_ambi=0, flags=2))
        cigar.append(4 << 4)
    n = len(BOUNDS)
    return SS.make_set(rows, tags, list(range(n + 1)), [0] * n, ["b%d" % k for k in range(n)], ["ACGT"] * n, ["IIII"] * n, [0] * n, 0, cigar=cigar)


def refused_sets():
    """(name, set) pairs, each with one thing BAM cannot hold; the first two pass: the untouched set, and a name of 254 bytes"""
    good = next(s for s in random_sets(8, 400) if len(s["hits"]) > 1 and s["hit_off"][1] > 0 and s["qnames"][0] is not None and s["hits"][0]["n_cigar"] > 0)

    def variant(f):
        s = {k: (v.copy() if isinstance(v, np.ndarray) else list(v) if isinstance(v, list) else v) for k, v in good.items()}
        f(s)
        return s

    def mapq(s): s["hits"]["mapq"][0] = 256
    def name(s): s["qnames"][0] = "n" * 255 + " comment"
    def name254(s): s["qnames"][0] = "n" * 254 + " comment"         # (passes)

    def clip5(s):                                       # a read said to be longer than 2^28 bases: the check reads lengths, never the bases
        s["qlens"][0] = 2**28 + 8
        s["hits"][0]["query_start"], s["hits"][0]["query_end"], s["hits"][0]["strand"] = 2**28, 2**28 + 4, 1

    def clip3(s):
        s["qlens"][0] = 2**28 + 8
        s["hits"][0]["query_start"], s["hits"][0]["query_end"], s["hits"][0]["strand"] = 2, 8, 1
    def sam_refusal(s): s["hits"][0]["query_start"] = s["hits"][0]["query_end"] + 1
    return [("good", good), ("name254", variant(name254))] + [(f.__name__, variant(f)) for f in (mapq, name, clip5, clip3, sam_refusal)]
