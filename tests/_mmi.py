"""What the index-dump tests share: a parser of minimap2's MMI\\2 file, the repeat-rich reference of the issue (written as FASTA, FASTQ
and gzip), the four index settings, reads over it, and thin wrappers of the C-ABI calls (build, load, dump)."""
import ctypes as C
import gzip
import random

import numpy as np

# k, w, flag: the default, a hifi-like k = w, k = 6 (b clamps to 12: at most one key per bucket) and homopolymer compression
SETTINGS = [(15, 10, 0), (19, 19, 0), (6, 3, 0), (15, 10, 1)]


def parse_mmi(data):
    """bytes of an MMI\\2 file -> dict: head (magic + w k b n_seq flag, raw), w k b n_seq flag, contigs [(name, len)], contig_raw,
    buckets [(p uint64[n], pairs uint64[size, 2])] for every one of the 1<<b buckets, S (raw bytes; b"" with MM_I_NO_SEQ)"""
    assert data[:4] == b"MMI\2"
    w, k, b, n_seq, flag = (int(x) for x in np.frombuffer(data, np.uint32, 5, 4))
    o = 24
    contigs = []
    for _ in range(n_seq):
        l = data[o]
        name = data[o + 1:o + 1 + l]
        ln = int.from_bytes(data[o + 1 + l:o + 5 + l], "little")
        contigs.append((name, ln)); o += 5 + l
    o_b = o
    buckets = []
    for _ in range(1 << b):
        n = int.from_bytes(data[o:o + 4], "little", signed=True); o += 4
        assert n >= 0
        p = np.frombuffer(data, np.uint64, n, o); o += 8 * n
        size = int.from_bytes(data[o:o + 4], "little"); o += 4
        pairs = np.frombuffer(data, np.uint64, 2 * size, o).reshape(size, 2); o += 16 * size
        buckets.append((p, pairs))
    S = b""
    if not flag & 2:
        n_S = (sum(ln for _, ln in contigs) + 7) // 8 * 4
        S = data[o:o + n_S]; o += n_S
        assert len(S) == n_S
    assert o == len(data), (o, len(data))
    return dict(head=data[:24], w=w, k=k, b=b, n_seq=n_seq, flag=flag, contigs=contigs, contig_raw=data[24:o_b], buckets=buckets, S=S)


def sorted_pairs(pairs):
    return pairs[np.argsort(pairs[:, 0], kind="stable")] if len(pairs) else pairs


def assert_canonical(m):
    """within a bucket keys ascend, and p[] holds the runs of the multi-occurrence keys in that order, back to back, each run ascending"""
    for p, pairs in m["buckets"]:
        keys = pairs[:, 0]
        assert (keys[1:] > keys[:-1]).all()
        at = 0
        for key, val in pairs:
            if int(key) & 1:
                continue
            start, cnt = int(val) >> 32, int(val) & 0xffffffff
            assert start == at and cnt >= 2
            run = p[start:start + cnt]
            assert (run[1:] > run[:-1]).all()
            at += cnt
        assert at == len(p)


def assert_same_index(ours, theirs):
    """two parsed files hold the same index: everything byte-identical but the order of the pairs inside a bucket"""
    assert ours["head"] == theirs["head"] and ours["contig_raw"] == theirs["contig_raw"] and ours["S"] == theirs["S"]
    for (p, pairs), (q, qairs) in zip(ours["buckets"], theirs["buckets"]):
        assert len(p) == len(q) and len(pairs) == len(qairs)
        assert p.tobytes() == q.tobytes()
        assert sorted_pairs(pairs).tobytes() == sorted_pairs(qairs).tobytes()


# ------------------------------------------------------------------ the repeat-rich reference
def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def repeat_rich_records():
    """[(name, sequence)]: a random 20 kb backbone holding a 50-mer x 120 tandem repeat and an N run, a contig that shares a 2 kb segment with
    it, a contig shorter than every k, and a short contig of its own"""
    rng = random.Random(355)
    unit = _rand(rng, 50)
    shared = _rand(rng, 2000)
    back = _rand(rng, 20000)
    c0 = back[:6000] + unit * 120 + back[6000:11000] + "N" * 37 + back[11000:15000] + shared + back[15000:]
    c1 = _rand(rng, 1500) + shared + _rand(rng, 2500)
    return [("backbone", c0), ("sharer", c1), ("tiny", "ACGTA"), ("plain", _rand(rng, 3000))]


def write_fasta(path, recs, width=70):
    with open(path, "w") as f:
        for name, s in recs:
            f.write(">%s some description\n" % name)
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + "\n")


def write_fastq(path, recs):
    with open(path, "w") as f:
        for name, s in recs:
            f.write("@%s\n%s\n+\n%s\n" % (name, s, "I" * len(s)))


def write_gzip(path, src):
    with open(src, "rb") as f, gzip.open(path, "wb") as g:
        g.write(f.read())


def make_reads(recs, n=64, seed=77):
    """n reads of 400-2500 bases cut from the two long contigs, ~6 % substitutions / indels, every other one reverse-complemented; the first
    eight start inside or just before the tandem repeat and run across it"""
    rng = random.Random(seed)
    comp = str.maketrans("ACGTN", "TGCAN")
    reads = []
    for i in range(n):
        src = recs[0][1] if i < 8 or i % 3 else recs[1][1]
        ln = min(rng.randrange(400, 2500), len(src) - 1)
        st = rng.randrange(5500, 6500) if i < 8 else rng.randrange(0, len(src) - ln)
        out = []
        for c in src[st:st + ln]:
            r = rng.random()
            if r < 0.03:
                out.append(rng.choice("ACGT"))
            elif r < 0.045:
                continue
            elif r < 0.06:
                out.append(c); out.append(rng.choice("ACGT"))
            else:
                out.append(c)
        s = "".join(out)
        reads.append(s.translate(comp)[::-1] if i & 1 else s)
    return reads


# ------------------------------------------------------------------ C-ABI wrappers
def idxopt(ffi, k, w, flag):
    io, mo = ffi.IdxOpt(), ffi.MapOpt()
    ffi.lib().mm355_set_opt(None, C.byref(io), C.byref(mo))
    io.k, io.w, io.flag = k, w, flag
    return io


def load(ffi, path, io, device=None):
    """mm355_index_load, or mm355_index_load_device when a device is given -> (return code, handle)"""
    h = C.c_void_p()
    if device is None:
        rc = ffi.lib().mm355_index_load(str(path).encode(), C.byref(io), 2, C.byref(h))
    else:
        rc = ffi.lib().mm355_index_load_device(str(path).encode(), C.byref(io), device, C.byref(h))
    return rc, h


def build(ffi, recs, io, device=None):
    """mm355_index_build, or mm355_index_build_device when a device is given -> handle"""
    n = len(recs)
    seqs = (C.c_char_p * n)(*[s.encode() for _, s in recs])
    lens = (C.c_int64 * n)(*[len(s) for _, s in recs])
    names = (C.c_char_p * n)(*[nm.encode() for nm, _ in recs])
    h = C.c_void_p()
    if device is None:
        ffi.check(ffi.lib().mm355_index_build(C.byref(io), n, seqs, lens, names, 2, C.byref(h)))
    else:
        ffi.check(ffi.lib().mm355_index_build_device(C.byref(io), n, seqs, lens, names, device, C.byref(h)))
    return h


def dump(ffi, h, path):
    """mm355_index_dump -> the file's bytes"""
    ffi.check(ffi.lib().mm355_index_dump(h, str(path).encode()))
    with open(path, "rb") as f:
        return f.read()
