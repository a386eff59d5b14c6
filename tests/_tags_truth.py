"""Truth for the PAF tags (mm355_tags_t, Aligner(tags=True)): the oracle's own mm_reg1_t / mm_extra_t records, read through ctypes.

oracle.OracleAligner.map() goes through mmo_map_flat, which keeps only what mappy_rs::Mapping has.  The tags need the rest of the region
record -- score, div, inv, split, sam_pri, p->n_ambi -- and the read's rep_len (mmo_stats), so this module declares mmo_reg1_t / mmo_extra_t
(oracle/mmo.h) and calls mmo_map() itself.  n_gap / n_gapo are counted from the oracle's CIGAR in plain Python.  div is compared as a float
bit pattern, never with a tolerance."""
import ctypes as C
import struct

import numpy as np

from oracle import oracle as O


class Extra(C.Structure):      # mmo_extra_t without its flexible CIGAR array
    _fields_ = [("capacity", C.c_uint32), ("dp_score", C.c_int32), ("dp_max", C.c_int32), ("dp_max2", C.c_int32),
                ("ambi_ts", C.c_uint32),       # n_ambi:30, trans_strand:2
                ("n_cigar", C.c_uint32)]


class Reg1(C.Structure):       # mmo_reg1_t
    _fields_ = [(k, C.c_int32) for k in ("id", "cnt", "rid", "score", "qs", "qe", "rs", "re", "parent", "subsc", "as_", "mlen", "blen",
                                          "n_sub", "score0")] + \
               [("bits", C.c_uint32),          # mapq:8, split:2, rev:1, inv:1, sam_pri:1, ...
                ("hash", C.c_uint32), ("div", C.c_float), ("p", C.POINTER(Extra))]


assert C.sizeof(Reg1) == 80 and C.sizeof(Extra) == 24

TAG_FIELDS = ("score", "div_bits", "rep_len", "n_ambi", "n_gap", "n_gapo", "inv", "sam_pri", "split")
HIT_FIELDS = ("query_start", "query_end", "strand", "rid", "target_start", "target_end", "match_len", "block_len", "mapq", "is_primary",
              "score0", "cnt", "subsc", "dp_max", "dp_score", "n_cigar")


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def gap_counts(cigar_words):
    """(n_gap, n_gapo) of packed CIGAR words (len << 4 | op): summed lengths and number of the I / D operations"""
    n_gap = n_gapo = 0
    for w in cigar_words:
        if int(w) & 0xf in (1, 2):
            n_gap += int(w) >> 4
            n_gapo += 1
    return n_gap, n_gapo


def _lib():
    L = O.lib()
    if not getattr(L, "_tags_truth_ready", False):
        L.mmo_map.restype = C.POINTER(Reg1)
        L.mmo_map.argtypes = [C.POINTER(O.Idx), C.c_int, C.c_char_p, C.POINTER(C.c_int), C.POINTER(O.MapOpt), C.c_char_p]
        L._tags_truth_ready = True
    return L


def oracle_tags(orc, seq):
    """the read through mmo_map(): a list, one dict per region in output order, with TAG_FIELDS and HIT_FIELDS"""
    if len(seq) == 0:
        return []
    L = _lib()
    b = seq.encode()
    n = C.c_int(0)
    regs = L.mmo_map(orc.idx, len(b), b, C.byref(n), C.byref(orc.mo), None)
    rep_len = int(orc.stats().rep_len)
    out = []
    for i in range(n.value):
        r = regs[i]
        d = dict(score=r.score, div_bits=f32_bits(r.div), div=float(r.div), rep_len=rep_len, n_ambi=0, n_gap=0, n_gapo=0,
                 inv=r.bits >> 11 & 1, sam_pri=r.bits >> 12 & 1, split=r.bits >> 8 & 3,
                 query_start=r.qs, query_end=r.qe, strand=-1 if r.bits >> 10 & 1 else 1, rid=r.rid, target_start=r.rs, target_end=r.re,
                 match_len=r.mlen, block_len=r.blen, mapq=r.bits & 0xff, is_primary=int(r.parent == r.id), score0=r.score0, cnt=r.cnt,
                 subsc=r.subsc, dp_max=0, dp_score=0, n_cigar=0)
        if r.p:
            p = r.p.contents
            words = np.ctypeslib.as_array(C.cast(C.addressof(p) + C.sizeof(Extra), C.POINTER(C.c_uint32)), shape=(p.n_cigar,)) if p.n_cigar else []
            d["n_gap"], d["n_gapo"] = gap_counts(words)
            d.update(n_ambi=p.ambi_ts & 0x3fffffff, dp_max=p.dp_max, dp_score=p.dp_score, n_cigar=int(p.n_cigar))
            L.free(C.cast(r.p, C.c_void_p))
        out.append(d)
    if regs:
        L.free(C.cast(regs, C.c_void_p))
    return out


def tags_tuple(d):
    return tuple(d[k] for k in TAG_FIELDS)
