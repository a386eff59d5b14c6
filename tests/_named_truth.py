"""Truth for query names (mm355_map_batch_named, Aligner.map(name=...)): the read hash and skip_seed's NO_DIAG / NO_DUAL branch.

(a) hash only: the oracle's mmo_map(..., qname) hashes the name itself (oracle_named).
(b) the filter: the oracle has no name branch in skip_seed and no MM_SEED_SELF clamp, so the truth is a composition of the oracle's exported
    stages with the filter stated here in numpy on the generation-order anchors (compose_named) -- the body of mmo_map, step by step.
    With the filter off it must reproduce mmo_map(qname) field for field (tests/test_named_host.py proves that before anything relies on
    it).  In CIGAR mode it is truth only for reads without SELF anchors.

The two worlds the tests share (built once per process) are here as well."""
import atexit
import ctypes as C
import functools
import os
import shutil
import tempfile

import numpy as np

from oracle import oracle as O
import synthdata as S
from _tags_truth import Reg1, Extra, f32_bits, gap_counts

NO_DIAG, NO_DUAL, CIGAR, FOR_ONLY, REV_ONLY, ALL_CHAINS, HARD_MLEVEL, NO_HASH_NAME = 1, 2, 4, 0x100000, 0x200000, 0x800000, 0x20000000, 0x400000000
SEED_SELF = 1 << 43
U32 = np.uint64(0xffffffff)

ROW_FIELDS = ("rid", "query_start", "query_end", "strand", "target_start", "target_end", "match_len", "block_len", "mapq", "is_primary",
              "score0", "cnt", "subsc", "dp_max", "dp_score", "n_cigar")
TAG_FIELDS = ("score", "div_bits", "rep_len", "n_ambi", "n_gap", "n_gapo", "inv", "sam_pri", "split")


def _lib():
    L = O.lib()
    if not getattr(L, "_named_truth_ready", False):
        vp, ip = C.c_void_p, C.POINTER(C.c_int)
        L.mmo_map.restype = C.POINTER(Reg1)
        L.mmo_map.argtypes = [C.POINTER(O.Idx), C.c_int, C.c_char_p, ip, C.POINTER(O.MapOpt), C.c_char_p]
        L.mmo_gen_regs.restype = C.POINTER(Reg1)
        L.mmo_gen_regs.argtypes = [C.c_uint32, C.c_int, C.c_int, vp, vp, C.c_int]
        L.mmo_set_parent.restype = None
        L.mmo_set_parent.argtypes = [C.c_float, C.c_int, C.c_int, C.POINTER(Reg1), C.c_int, C.c_int, C.c_float]
        L.mmo_select_sub.restype = None
        L.mmo_select_sub.argtypes = [C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, ip, C.POINTER(Reg1)]
        L.mmo_est_err.restype = None
        L.mmo_est_err.argtypes = [C.POINTER(O.Idx), C.c_int, C.c_int, C.POINTER(Reg1), vp, C.c_int32, vp]
        L.mmo_filter_strand_retained.argtypes = [C.c_int, C.POINTER(Reg1)]
        L.mmo_align_skeleton.restype = C.POINTER(Reg1)
        L.mmo_align_skeleton.argtypes = [C.POINTER(O.MapOpt), C.POINTER(O.Idx), C.c_int, C.c_char_p, ip, C.POINTER(Reg1), vp]
        L.mmo_set_sam_pri.argtypes = [C.c_int, C.POINTER(Reg1)]
        L.mmo_set_mapq.restype = None
        L.mmo_set_mapq.argtypes = [C.c_int, C.POINTER(Reg1), C.c_int, C.c_int, C.c_int, C.c_int]
        L.mmo_gen_cs.restype = vp
        L.mmo_gen_cs.argtypes = [C.POINTER(O.Idx), C.POINTER(Reg1), C.c_char_p, C.c_int]
        L._named_truth_ready = True
    return L


# ---------------------------------------------------------------- the hash (U:map.c::mm_map_frag)
def _wang32(k):
    k = (k + (~(k << 15) & 0xffffffff)) & 0xffffffff
    k ^= k >> 10
    k = (k + (k << 3)) & 0xffffffff
    k ^= k >> 6
    k = (k + (~(k << 11) & 0xffffffff)) & 0xffffffff
    k ^= k >> 16
    return k


def x31(name):
    """X31 over the bytes as C `char` (a byte >= 0x80 is sign-extended, as the oracle's x31_hash_string does)"""
    sc = [b - 256 if b >= 128 else b for b in name]
    if not sc or sc[0] == 0:
        return 0
    h = sc[0] & 0xffffffff
    for c in sc[1:]:
        h = ((h << 5) - h + c) & 0xffffffff
    return h


def read_hash(qlen, seed, name, flag=0):
    h = x31(name) if name is not None and not flag & NO_HASH_NAME else 0
    h ^= (_wang32(qlen & 0xffffffff) + _wang32(seed & 0xffffffff)) & 0xffffffff
    return _wang32(h)


# ---------------------------------------------------------------- skip_seed's name branch, on generation-order anchors
def name_filter(a, qlen, qname, tnames, tlens, flag):
    """a: [n, 2] u64 anchors in generation order (the oracle's, strand filters already applied).  Returns (keep mask, self mask).
    Names are bytes, compared as Python compares bytes: unsigned, a proper prefix first -- strcmp."""
    n = a.shape[0]
    keep = np.ones(n, bool); self_ = np.zeros(n, bool)
    if qname is None or not flag & (NO_DIAG | NO_DUAL) or n == 0:
        return keep, self_
    x, y = a[:, 0], a[:, 1]
    rev = (x >> np.uint64(63)).astype(bool)
    rid = ((x >> np.uint64(32)) & np.uint64(0x7fffffff)).astype(np.int64)
    rpos = (x & U32).astype(np.int64)
    span = ((y >> np.uint64(32)) & np.uint64(0xff)).astype(np.int64)
    ylo = (y & U32).astype(np.int64)
    qpos = np.where(rev, qlen + span - 2 - ylo, ylo)
    gt = np.array([qname > t for t in tnames], bool)[rid]           # strcmp(qname, tname) > 0
    own = np.array([qname == t and l == qlen for t, l in zip(tnames, tlens)], bool)[rid]
    if flag & NO_DIAG:
        keep &= ~(own & (rpos == qpos))
        self_ = own & ~rev & (rpos != qpos)
    if flag & NO_DUAL:
        keep &= ~gt
    return keep, self_ & keep


# ---------------------------------------------------------------- region records -> dicts
def _rows(L, orc, regs, n, rep_len, seq_b, with_cs):
    out = []
    for i in range(n):
        r = regs[i]
        d = dict(score=r.score, div_bits=f32_bits(r.div), rep_len=rep_len, n_ambi=0, n_gap=0, n_gapo=0,
                 inv=r.bits >> 11 & 1, sam_pri=r.bits >> 12 & 1, split=r.bits >> 8 & 3,
                 query_start=r.qs, query_end=r.qe, strand=-1 if r.bits >> 10 & 1 else 1, rid=r.rid, target_start=r.rs, target_end=r.re,
                 match_len=r.mlen, block_len=r.blen, mapq=r.bits & 0xff, is_primary=int(r.parent == r.id), score0=r.score0, cnt=r.cnt,
                 subsc=r.subsc, dp_max=0, dp_score=0, n_cigar=0, cigar=b"", cs=None)
        if r.p:
            p = r.p.contents
            words = np.ctypeslib.as_array(C.cast(C.addressof(p) + C.sizeof(Extra), C.POINTER(C.c_uint32)), shape=(p.n_cigar,)).copy() \
                if p.n_cigar else np.zeros(0, np.uint32)
            d["n_gap"], d["n_gapo"] = gap_counts(words)
            d.update(n_ambi=p.ambi_ts & 0x3fffffff, dp_max=p.dp_max, dp_score=p.dp_score, n_cigar=int(p.n_cigar), cigar=words.tobytes())
            if with_cs:
                s = L.mmo_gen_cs(orc.idx, C.byref(r), seq_b, 1)
                d["cs"] = C.string_at(s)
                L.free(s)
            L.free(C.cast(r.p, C.c_void_p))
        out.append(d)
    if regs:
        L.free(C.cast(regs, C.c_void_p))
    return out


def oracle_named(orc, seq, qname, with_cs=False):
    """(a) the read through mmo_map(..., qname): the oracle hashes the name (and filters nothing)"""
    if len(seq) == 0:
        return []
    L = _lib()
    b = seq.encode()
    n = C.c_int(0)
    regs = L.mmo_map(orc.idx, len(b), b, C.byref(n), C.byref(orc.mo), qname)
    return _rows(L, orc, regs, n.value, int(orc.stats().rep_len), b, with_cs)


def filtered_anchors(orc, seq, qname, flag=None):
    """generation-order anchors after skip_seed's name branch (SELF marked in bit 43), rep_len, mini_pos"""
    a, rep_len, mini_pos, _ = orc.anchors(seq, sorted_=False)
    keep, self_ = name_filter(a, len(seq), qname, [t.encode("utf-8", "surrogateescape") for t in orc.seq_names], orc.seq_lens,
                              orc.mo.flag if flag is None else flag)
    a = a.copy()
    a[self_, 1] |= np.uint64(SEED_SELF)
    return np.ascontiguousarray(a[keep]), rep_len, mini_pos, int(self_.sum())


def compose_named(orc, seq, qname, filter_on=True, with_cs=False):
    """(b) the body of mmo_map (oracle/mmo_map.c) from the oracle's exported stages, with skip_seed's name branch between the anchor
    generation and the sort.  filter_on=False: no filter -- must equal oracle_named.  Returns (rows, number of SELF anchors)."""
    L = _lib()
    mo = orc.mo
    b = seq.encode()
    qlen = len(b)
    if qlen == 0:
        return [], 0
    a, rep_len, mini_pos, n_self = filtered_anchors(orc, seq, qname, None if filter_on else 0)
    if a.shape[0]:
        L.mmo_radix_sort_128x(a.ctypes.data, a.ctypes.data + a.shape[0] * 16)
    u, ca, _ = orc.chains_final(a, qlen)
    if len(u) == 0:
        return [], n_self
    u = np.ascontiguousarray(u, np.uint64); ca = np.ascontiguousarray(ca, np.uint64); mini_pos = np.ascontiguousarray(mini_pos, np.uint64)
    k = orc.k
    regs = L.mmo_gen_regs(read_hash(qlen, mo.seed, qname, mo.flag), qlen, len(u), u.ctypes.data, ca.ctypes.data, 0)
    n = C.c_int(len(u))
    sub_diff, strand_sc = mo.a * 2 + mo.b, int(mo.max_gap * 0.8)
    if not mo.flag & ALL_CHAINS:
        L.mmo_set_parent(mo.mask_level, mo.mask_len, n.value, regs, sub_diff, int(bool(mo.flag & HARD_MLEVEL)), mo.alt_drop)
        L.mmo_select_sub(mo.pri_ratio, k * 2, mo.best_n, 1, strand_sc, C.byref(n), regs)
    L.mmo_est_err(orc.idx, qlen, n.value, regs, ca.ctypes.data, len(mini_pos), mini_pos.ctypes.data)
    n.value = L.mmo_filter_strand_retained(n.value, regs)
    if mo.flag & CIGAR:
        regs = L.mmo_align_skeleton(C.byref(mo), orc.idx, qlen, b, C.byref(n), regs, ca.ctypes.data)
        if not mo.flag & ALL_CHAINS:
            L.mmo_set_parent(mo.mask_level, mo.mask_len, n.value, regs, sub_diff, int(bool(mo.flag & HARD_MLEVEL)), mo.alt_drop)
            L.mmo_select_sub(mo.pri_ratio, k * 2, mo.best_n, 0, strand_sc, C.byref(n), regs)
            L.mmo_set_sam_pri(n.value, regs)
    L.mmo_set_mapq(n.value, regs, mo.min_chain_score, mo.a, rep_len, 0)
    return _rows(L, orc, regs, n.value, rep_len, b, with_cs), n_self


def row_tuple(d):
    return tuple(d[k] for k in ROW_FIELDS)


def tag_tuple(d):
    return tuple(d[k] for k in TAG_FIELDS)


# ---------------------------------------------------------------- the worlds
def _mut(codes, rng, err):
    return S.mutate(codes, rng, err * 0.4, err * 0.27, err * 0.33)


@functools.lru_cache(maxsize=None)
def overlap_world():
    """An all-vs-all set indexed as its own targets: 17 reads of 3 kb cut every 800 bases from a 15 kb genome (6 % error), one 8 kb read
    (more than 1024 kept seeds: crosses EX_TILE), one read with a 900-base internal repeat (off-diagonal SELF anchors).  Contig names are
    shuffled against the order along the genome and include prefixes of one another, a byte >= 0x80, the empty string and one name shared
    by two contigs.  Returns a dict: fa, targets [(name bytes, seq)], queries [(name bytes or None, seq)]."""
    rng = np.random.Generator(np.random.PCG64(20240))
    g = S.random_codes(rng, 15000)
    reads = [S.codes_to_str(_mut(g[s:s + 3000], rng, 0.06)) for s in range(0, 15000 - 3000 + 1, 800)]
    reads += [S.codes_to_str(_mut(g[13000:15000], rng, 0.06))]                 # a short tail read: 17 in all
    assert len(reads) == 17
    long_read = S.codes_to_str(_mut(g[2000:10000], rng, 0.06))
    unit = S.random_codes(rng, 900)
    rep_read = S.codes_to_str(np.concatenate([S.random_codes(rng, 500), unit, S.random_codes(rng, 300), _mut(unit, rng, 0.03), S.random_codes(rng, 400)]))
    names = [b"rd1", b"rd10", b"rd1a", b"rd\xc3\xa9", b"", b"dup", b"dup", b"zz", b"a", b"rd2", b"rd20", b"m5", b"Rd1", b"rd3", b"k", b"rd11", b"b9"]
    order = rng.permutation(17)
    targets = [(names[i], reads[order[i]]) for i in range(17)] + [(b"long8k", long_read), (b"selfrep", rep_read)]
    td = tempfile.mkdtemp(prefix="named_world_")
    atexit.register(shutil.rmtree, td, True)
    fa = os.path.join(td, "reads.fa")
    with open(fa, "wb") as fh:
        for nm, s in targets:
            fh.write(b">" + nm + b"\n" + s.encode() + b"\n")
    greatest = max(nm for nm, _ in targets)
    gi = [nm for nm, _ in targets].index(greatest)
    queries = list(targets)
    queries.insert(7, (None, reads[3]))                                         # an unnamed read in the middle of a named batch
    queries.append((b"rd10", reads[order[1]][:2500]))                           # the name of a contig, another length
    queries.append((b"rd15", reads[5]))                                         # no contig has this name; it sorts between rd11 and rd1a
    queries.append((b"rd1", reads[order[0]]))                                   # (again: the same named read twice in one batch)
    return dict(fa=fa, targets=targets, queries=queries, greatest=gi)


@functools.lru_cache(maxsize=None)
def dup_world():
    """two identical 20 kb contigs and a third; 3 kb reads from the duplicate, each mapped under four names: the primary / secondary
    assignment between the copies is decided by the hash alone"""
    rng = np.random.Generator(np.random.PCG64(777))
    c = S.random_codes(rng, 20000)
    other = S.random_codes(rng, 20000)
    td = tempfile.mkdtemp(prefix="named_dup_")
    atexit.register(shutil.rmtree, td, True)
    fa = os.path.join(td, "dup.fa")
    S.write_fasta(fa, [c, c.copy(), other], ["copyA", "copyB", "other"])
    reads = [S.codes_to_str(_mut(c[s:s + 3000], rng, 0.06)) for s in (500, 6000, 16500)]
    names = [b"r", b"read/1", b"q\xff", b"a-long-read-name-0001"]
    return dict(fa=fa, reads=reads, names=names)
