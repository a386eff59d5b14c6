"""mappy_rs -- drop-in surface of Adoni5/mappy-rs for the MI355X-native mapping path.

Mirrors the reference's PyO3 module (/root/reference/src/lib.rs:995-999: only `Aligner` is
exported; `Mapping` and the batch iterator are reachable as return values).  Same constructor
keywords (lib.rs:312), same properties (lib.rs:439-470, 651-670), same `map` / `map_batch` /
`enable_threading` semantics and the same exception types and messages (lib.rs:388-394, 435,
477-481, 777-792, 847-866, 889-896).  Where the reference dispatches reads to N OS threads that
each call minimap2's mm_map (lib.rs:541-636), this module hands whole batches to libmm355.so
(hand-written HIP kernels for gfx950) through the C-ABI of include/mm355.h.  The extension is
mandatory: importing works without a GPU (so the API can be inspected), but creating an
Aligner that maps reads requires the HIP library and a visible MI355X -- there is no CPU path.
"""
import collections
import collections.abc
import contextlib
import ctypes as C
import functools
import os
import struct
import tempfile
import threading
import time

# ROCclr multiplexes all HIP streams over GPU_MAX_HW_QUEUES hardware queues (default 4); the pipelined map_batch keeps several contexts in
# flight and measures best with 8 (bench.py sets the same).  Only effective if the HIP runtime has not been started yet.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np

from . import _batch, _ffi, _pipeline
from ._batch import AlignmentBatchResultIter

__all__ = ["Aligner", "Mapping", "paf_line", "sam_lines", "shard_by_bases", "order_by_length", "bgzf_unwrap", "bam_aux_split"]

_CIGAR_OPS = "MIDNSHP=X"

# capacity constants of the reference (lib.rs:429-430, 950)
SUB_BATCH_READS, SUB_BATCH_BASES = 9216, 96_000_000   # one GPU sub-batch of map_batch (bench.py's default shape: a 73 728-read block over eight contexts)
WORK_QUEUE_CAP = 50000
SORT_CHUNK_BYTES = 64 << 20        # map_bam_file(sort=True): the records one step of the merge gathers, deflates and writes
BAI_MAX_LEN = 1 << 29              # map_bam_file(index=True): the longest contig a .bai index can hold
# results a batch may hold before its workers wait for the consumer: the reference's results_queue (ArrayQueue of 50 000, lib.rs:430) plus its
# bounded(20000) channel (lib.rs:950) -- here one channel.  (With 20 000 alone the workers stall while map_batch is still consuming its
# iterable, which nobody reads during: -12 % on 262 144 reads.)
RESULT_CHANNEL_CAP = 70000


_HIT_FIELDS = [k for k, _t in _ffi.Hit._fields_]
_F = {k: i for i, k in enumerate(_HIT_FIELDS)}
_HIT_DTYPE, _TAG_DTYPE = _ffi._HIT_DTYPE, _ffi._TAG_DTYPE
(_QS, _QE, _ST, _RID, _TL, _TS, _TE, _ML, _BL, _MQ, _PR, _NM, _NC, _CO, _CSO, _CSL, _MDO, _MDL) = (_F[k] for k in (
    "query_start", "query_end", "strand", "rid", "target_len", "target_start", "target_end", "match_len", "block_len", "mapq",
    "is_primary", "NM", "n_cigar", "cigar_off", "cs_off", "cs_len", "md_off", "md_len"))
# a record mapped with tags=True: the row of the mm355_tags_t array stands behind the hit row in the same tuple
_T0 = len(_HIT_FIELDS)
_TAG_HIT = tuple(_F[k] for k in ("subsc", "cnt", "dp_max", "dp_score"))
# what a record keeps of its tags (view: built on access, detached: _own[15]):
# (s1, div, rl, n_ambi, n_gap, n_gapo, flags, s2, cm, ms, AS)
(_G_S1, _G_DIV, _G_RL, _G_NN, _G_GAP, _G_GAPO, _G_FL, _G_S2, _G_CM, _G_MS, _G_AS) = range(11)


class _HitBatch:
    """what the Mapping records of one mm355_hits_t share: the packed CIGAR words, the string arena, the contig names, and whether the batch
    was mapped without CIGARs (chain-only: no extension, records come from the chains)"""
    __slots__ = ("cig", "sbuf", "names", "chain_only", "tags")

    def __init__(self, cig, sbuf, names, chain_only=False, tags=False):
        self.cig, self.sbuf, self.names, self.chain_only, self.tags = cig, sbuf, names, chain_only, tags


class Mapping:
    """Result record; fields and aliases of mappy_rs::Mapping (lib.rs:109-154, 196-284).

    A record that comes out of the mapping path is a view: `_r` is the row of the C-ABI hit array (a tuple, converted in bulk), `_b`
    the arenas it points into; fields are read on access (the reference converts its Vec / Strings on access as well, lib.rs:196-284).
    Creating a record is two slot stores -- the per-hit cost under the GIL that used to cap `map_batch` below the C-ABI rate.
    Retention: an untouched view keeps its sub-batch's arenas alive (CIGAR words + cs / MD bytes of up to SUB_BATCH_READS reads, a few MB).
    The first access to `cigar`, `cs` or `MD` -- or `detach()` -- copies the record's own slices and drops that reference, so a caller that
    keeps a few records of a large `map_batch` (the reference's records own their Vec / Strings) holds a few hundred bytes each."""

    __slots__ = ("_b", "_r", "_cig", "_own")
    FIELDS = ("query_start", "query_end", "strand", "target_name", "target_len", "target_start", "target_end",
              "match_len", "block_len", "mapq", "is_primary", "cigar", "NM", "MD", "cs")

    def __init__(self, query_start, query_end, strand, target_name, target_len, target_start, target_end, match_len,
                 block_len, mapq, is_primary, cigar, NM, MD, cs):
        self._b = None
        self._r = None
        self._cig = list(cigar)
        self._own = (query_start, query_end, strand, target_name, target_len, target_start, target_end, match_len, block_len, mapq,
                     bool(is_primary), NM, MD, cs, False, None)

    @classmethod
    def _view(cls, batch, row):
        m = object.__new__(cls)
        m._b = batch
        m._r = row
        m._cig = None
        m._own = None
        return m

    query_start = property(lambda s: s._r[_QS] if s._own is None else s._own[0])
    query_end = property(lambda s: s._r[_QE] if s._own is None else s._own[1])
    strand = property(lambda s: s._r[_ST] if s._own is None else s._own[2])          # +1 / -1 (lib.rs:231-237)
    target_name = property(lambda s: s._b.names[s._r[_RID]] if s._own is None else s._own[3])
    target_len = property(lambda s: s._r[_TL] if s._own is None else s._own[4])
    target_start = property(lambda s: s._r[_TS] if s._own is None else s._own[5])
    target_end = property(lambda s: s._r[_TE] if s._own is None else s._own[6])
    match_len = property(lambda s: s._r[_ML] if s._own is None else s._own[7])
    block_len = property(lambda s: s._r[_BL] if s._own is None else s._own[8])
    mapq = property(lambda s: s._r[_MQ] if s._own is None else s._own[9])
    is_primary = property(lambda s: bool(s._r[_PR]) if s._own is None else s._own[10])
    NM = property(lambda s: s._r[_NM] if s._own is None else s._own[11])

    def detach(self):
        """make the record independent of its sub-batch: copy its fields, CIGAR and cs / MD out of the shared arenas and drop the reference"""
        if self._own is None:
            r, b = self._r, self._b
            w = b.cig[r[_CO]:r[_CO] + r[_NC]] if r[_NC] > 0 else b.cig[:0]
            self._cig = list(zip((w >> 4).tolist(), (w & 0xf).tolist()))
            md = b.sbuf[r[_MDO]:r[_MDO] + r[_MDL]].decode() if r[_MDL] >= 0 else None
            cs = b.sbuf[r[_CSO]:r[_CSO] + r[_CSL]].decode() if r[_CSL] >= 0 else None
            self._own = (r[_QS], r[_QE], r[_ST], b.names[r[_RID]], r[_TL], r[_TS], r[_TE], r[_ML], r[_BL], r[_MQ], bool(r[_PR]), r[_NM], md, cs,
                         b.chain_only, self._tags())
            self._b = self._r = None
        return self

    @property
    def MD(self):
        if self._own is None:
            self.detach()
        return self._own[12]

    @property
    def cs(self):
        if self._own is None:
            self.detach()
        return self._own[13]

    @property
    def cigar(self):
        """list of (length, op) tuples, as mappy-rs; unpacked from the packed uint32 words (length << 4 | op) on first access"""
        if self._own is None:
            self.detach()
        return self._cig

    # ---- minimap2's PAF tags (Aligner(tags=True)); every one is None on a record mapped without tags
    def _tags(self):
        if self._own is not None:
            return self._own[15]
        if not self._b.tags:
            return None
        r = self._r
        return r[_T0:_T0 + 7] + tuple(r[i] for i in _TAG_HIT)

    def _tag(self, i):
        t = self._tags()
        return None if t is None else t[i]

    def _has_cigar(self):
        return not (self._b.chain_only if self._own is None else self._own[14])

    s1 = property(lambda s: s._tag(_G_S1), doc="chaining score of the region (r->score)")
    s2 = property(lambda s: s._tag(_G_S2), doc="chaining score of the best secondary (r->subsc)")
    cm = property(lambda s: s._tag(_G_CM), doc="number of minimizers on the chain (r->cnt)")
    ms = property(lambda s: s._tag(_G_MS), doc="DP score of the max-scoring segment (r->p->dp_max)")
    AS = property(lambda s: s._tag(_G_AS), doc="DP alignment score (r->p->dp_score)")
    nn = property(lambda s: s._tag(_G_NN), doc="ambiguous bases in the alignment (r->p->n_ambi)")
    rl = property(lambda s: s._tag(_G_RL), doc="length of query regions harbouring repetitive seeds (per read)")

    @property
    def zd(self):
        """r->split: bit 0 = the region was split on its right, bit 1 = on its left (0: not split; minimap2 prints zd only then)"""
        t = self._tags()
        return None if t is None else t[_G_FL] >> _ffi.TAG_SPLIT_SHIFT & 3

    @property
    def dv(self):
        """approximate per-base divergence from the chain (mm_est_err); None with a CIGAR (minimap2 prints de instead) or when not estimated"""
        t = self._tags()
        if t is None or self._has_cigar() or not 0.0 <= t[_G_DIV] <= 1.0:
            return None
        return t[_G_DIV]

    @property
    def de(self):
        """gap-compressed per-base divergence, 1 - mlen / (blen + n_ambi - n_gap + n_gapo); None without a CIGAR"""
        t = self._tags()
        if t is None or not self._has_cigar():
            return None
        return 1.0 - float(self.match_len) / (self.block_len + t[_G_NN] - t[_G_GAP] + t[_G_GAPO])

    @property
    def tp(self):
        """'P' primary, 'S' secondary, 'I' / 'i' the same for an inversion record"""
        t = self._tags()
        if t is None:
            return None
        inv = t[_G_FL] & _ffi.TAG_INV
        return ("I" if inv else "P") if self.is_primary else ("i" if inv else "S")

    @property
    def is_supplementary(self):
        """a primary record that is not the read's first one (SAM flag 0x800: parent == id without sam_pri)"""
        t = self._tags()
        return None if t is None else bool(self.is_primary and not t[_G_FL] & _ffi.TAG_SAM_PRI)

    # mappy aliases (lib.rs:196-284)
    ctg = property(lambda s: s.target_name)
    ctg_len = property(lambda s: s.target_len)
    r_st = property(lambda s: s.target_start)
    r_en = property(lambda s: s.target_end)
    q_st = property(lambda s: s.query_start)
    q_en = property(lambda s: s.query_end)
    blen = property(lambda s: s.block_len)
    mlen = property(lambda s: s.match_len)

    @property
    def cigar_str(self):
        out = []
        for n, op in self.cigar:
            if op > 8:
                raise ValueError("Invalid CIGAR code `{op}`")
            out.append("%d%s" % (n, _CIGAR_OPS[op]))
        return "".join(out)

    def __str__(self):  # PAF-like, lib.rs:159-180; a chain-only record has no cg:Z: field (minimap2 prints none without -c)
        tp = "tp:A:P" if self.is_primary else "tp:A:S"
        chain_only = self._b.chain_only if self._own is None else self._own[14]
        cols = (self.query_start, self.query_end, "+" if self.strand > 0 else "-", self.target_name, self.target_len, self.target_start,
                self.target_end, self.match_len, self.block_len, self.mapq, tp)
        return "\t".join(str(x) for x in (cols if chain_only else cols + ("cg:Z:" + self.cigar_str,)))

    def __repr__(self):
        return "Mapping(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in Mapping.FIELDS)

    def __eq__(self, o):
        return isinstance(o, Mapping) and all(getattr(self, k) == getattr(o, k) for k in Mapping.FIELDS)

    __hash__ = None


def _batch_to_mappings(hp, n_reads, names, chain_only=False):
    """all hits of one mm355_hits_t (a pointer to it, or its _ffi.HitsView) -> list (per read) of list[Mapping] or RuntimeError.  One bulk copy
    per array (hit rows, CIGAR words, string arena); every Mapping is a view of its row (fields, cs / MD strings and the CIGAR list are produced
    on access).  chain_only: the batch was mapped without MM_F_CIGAR (no CIGAR words; the records print no cg:Z: field)."""
    v = hp if isinstance(hp, _ffi.HitsView) else _ffi.read_hits(hp, n_reads)
    off = v.off.tolist()
    empty = np.flatnonzero(v.status == _ffi.MM355_EEMPTY).tolist()
    if len(v.hits):
        rows = v.hits.tolist()
        has_tags = v.tags is not None
        if has_tags:    # the tags row of a hit goes behind its hit row
            rows = [r + t for r, t in zip(rows, v.tags.tolist())]
        B = _HitBatch(v.cigar, v.str, names, chain_only, has_tags)
        view = Mapping._view
        ms = [view(B, r) for r in rows]
        out = [ms[off[i]:off[i + 1]] for i in range(n_reads)]
    else:
        out = [[] for _ in range(n_reads)]
    for i in empty:
        out[i] = RuntimeError("Sequence is empty")
    return out


def _f4(x):
    return "0" if x == 0.0 else "%.4f" % x


def _tag_block(m, t, has_cigar):
    """the tags PAF and SAM share, in write_tags' order: NM ms AS nn with a CIGAR; tp cm s1, s2 on primaries; de or dv; zd on split regions"""
    f = []
    if has_cigar:
        f += ["NM:i:%d" % m.NM, "ms:i:%d" % t[_G_MS], "AS:i:%d" % t[_G_AS], "nn:i:%d" % t[_G_NN]]
    f += ["tp:A:" + m.tp, "cm:i:%d" % t[_G_CM], "s1:i:%d" % t[_G_S1]]
    if m.is_primary:
        f.append("s2:i:%d" % t[_G_S2])
    if has_cigar:
        f.append("de:f:" + _f4(m.de))
    elif 0.0 <= t[_G_DIV] <= 1.0:
        f.append("dv:f:" + _f4(t[_G_DIV]))
    if m.zd:
        f.append("zd:i:%d" % m.zd)
    return f


def paf_line(m, name, qlen):
    """one PAF line of the record `m` of the read `name` (length `qlen`): the twelve columns and the tags in the order of minimap2's PAF
    writer (format.c::mm_write_paf + write_tags).  Needs a record mapped with Aligner(tags=True): ValueError otherwise.

    name qlen qs qe +/- target tlen ts te mlen blen mapq, then with a CIGAR NM:i ms:i AS:i nn:i, then tp:A cm:i s1:i and, on primary records,
    s2:i; de:f with a CIGAR, otherwise dv:f when the divergence was estimated ("0" when exactly zero, else %.4f); zd:i on split regions;
    rl:i; with a CIGAR cg:Z, then cs:Z / MD:Z when the record has them.

    The layout is written from knowledge of mm_write_paf: the minimap2 sources and binary are not part of this repository, so the line has
    not been diffed against minimap2's own output.  The values behind it are checked against the oracle field by field."""
    t = m._tags()
    if t is None:
        raise ValueError("paf_line needs a record mapped with Aligner(tags=True)")
    has_cigar = m._has_cigar()
    f = [name, qlen, m.query_start, m.query_end, "+" if m.strand > 0 else "-", m.target_name, m.target_len, m.target_start, m.target_end,
         m.match_len, m.block_len, m.mapq]
    f += _tag_block(m, t, has_cigar)
    f.append("rl:i:%d" % t[_G_RL])
    if has_cigar:
        f.append("cg:Z:" + m.cigar_str)
        if m.cs is not None:
            f.append("cs:Z:" + m.cs)
        if m.MD is not None:
            f.append("MD:Z:" + m.MD)
    return "\t".join(str(x) for x in f)


# minimap2's seq_comp_table: bytes below 128, case kept; everything else (S W N among them) is its own complement
_SAM_COMP = {ord(a): ord(b) for a, b in zip("ACGTURYKMBVDHacgturykmbvdh", "TGCAAYRMKVBHDtgcaayrmkvbhd")}


def _sam_clips(m, qlen):
    """(clip5, clip3) of a record on a read of qlen bases, in the order the line prints them"""
    return (qlen - m.query_end, m.query_start) if m.strand < 0 else (m.query_start, qlen - m.query_end)


def sam_lines(ms, name, seq, qual=None, *, softclip=False, rl=None):
    """the SAM lines (str, no newline) of one read's records `ms` (mapped with Aligner(tags=True), base-level), as minimap2 -a writes them
    (format.c::mm_write_sam3, write_sam_cigar, sam_write_sq, write_tags of 2.26), one per record in order.  name: the read's name (printed
    up to its first blank; None prints `*`); seq / qual: the read and its quality string (None: `*`) as they were given to the mapping call;
    softclip: minimap2 -Y.  Empty `ms` gives the one unmapped record and needs rl, the read's rep_len.

    QNAME; FLAG = 0x10 on the reverse strand, 0x100 on a secondary, otherwise 0x800 on a supplementary; RNAME; POS = target_start + 1; MAPQ;
    CIGAR with the clipped read ends around it (H on a supplementary without softclip, otherwise S; `*` without a CIGAR); `*` 0 0; SEQ and
    QUAL: the whole read (reverse-complemented / reversed on the reverse strand) on the first primary and under softclip, `*` `*` on a
    secondary, the aligned slice on a hard-clipped supplementary; then NM ms AS nn tp cm s1 [s2] de [zd], SA:Z: on a primary when the read
    has other primaries with a CIGAR (rname,pos,strand,cigar,mapq,nm; each, the cigar as clip5 S, M, I, D, clip3 S), cs:Z: / MD:Z:, rl:i:.
    Records without tags, or chain-only records: ValueError.  Like paf_line, the layout is written from knowledge of minimap2's writer and
    has not been diffed against its output."""
    qn = "*" if name is None else name.replace("\t", " ").split(" ")[0]
    qlen = len(seq)
    if not ms:
        if rl is None:
            raise ValueError("the unmapped record needs `rl`, the read's rep_len")
        return ["\t".join([qn, "4", "*", "0", "0", "*", "*", "0", "0", seq, "*" if qual is None else qual, "rl:i:%d" % rl])]
    for m in ms:
        if m._tags() is None or not m._has_cigar():
            raise ValueError("sam_lines needs records mapped with Aligner(tags=True) and base-level alignment")
    out = []
    for m in ms:
        t = m._tags()
        rev = m.strand < 0
        flag = (0x10 if rev else 0) | (0x100 if not m.is_primary else 0 if t[_G_FL] & _ffi.TAG_SAM_PRI else 0x800)
        clip5, clip3 = _sam_clips(m, qlen)
        if len(m.cigar):
            letter = "H" if flag & 0x800 and not softclip else "S"
            cig = ("%d%s" % (clip5, letter) if clip5 else "") + m.cigar_str + ("%d%s" % (clip3, letter) if clip3 else "")
        else:
            cig = "*"
        if flag & 0x900 == 0 or softclip:
            s, q = seq, qual
        elif flag & 0x100:
            s, q = None, None
        else:
            s, q = seq[m.query_start:m.query_end], None if qual is None else qual[m.query_start:m.query_end]
        if s is None:
            s = q = "*"
        else:
            if rev:
                s, q = s[::-1].translate(_SAM_COMP), None if q is None else q[::-1]
            q = "*" if q is None else q
        f = [qn, flag, m.target_name, m.target_start + 1, m.mapq, cig, "*", 0, 0, s, q]
        f += _tag_block(m, t, True)
        if m.is_primary:
            sa = []
            for o in ms:
                if o is m or not o.is_primary or not len(o.cigar):
                    continue
                c5, c3 = _sam_clips(o, qlen)
                ql, tl = o.query_end - o.query_start, o.target_end - o.target_start
                l_m, l_i, l_d = (ql, 0, tl - ql) if ql < tl else (tl, ql - tl, 0)
                oc = "".join("%d%s" % (n, c) for n, c in ((c5, "S"), (l_m, "M"), (l_i, "I"), (l_d, "D"), (c3, "S")) if n)
                sa.append("%s,%d,%s,%s,%d,%d;" % (o.target_name, o.target_start + 1, "-" if o.strand < 0 else "+", oc, o.mapq,
                                                  o.block_len - o.match_len + o._tags()[_G_NN]))
            if sa:
                f.append("SA:Z:" + "".join(sa))
        if m.cs is not None:
            f.append("cs:Z:" + m.cs)
        if m.MD is not None:
            f.append("MD:Z:" + m.MD)
        f.append("rl:i:%d" % t[_G_RL])
        out.append("\t".join(str(x) for x in f))
    return out


# the empty BGZF block that ends a BAM file
BAM_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bam_aux_split(aux, keep="*"):
    """(kept, mod_off): the tags of the BAM aux block `aux` (bytes) that `keep` names -- "*" for all, or two-letter names back to back --
    in the two groups the BAM writer takes: first every kept tag but MM ML MN Mm Ml, then, from mod_off, those (mm355_bam_aux_split; the
    tags the writer emits itself are always dropped).  ValueError: a malformed block or `keep`."""
    aux = bytes(aux)
    out = C.create_string_buffer(max(1, len(aux)))
    n_out, mod = C.c_int32(), C.c_int32()
    if len(aux) > 2**31 - 1 or _ffi.lib().mm355_bam_aux_split(aux, len(aux), keep.encode("latin-1"), out, C.byref(n_out), C.byref(mod)) != 0:
        raise ValueError("malformed BAM aux block, or malformed `keep`")
    return out.raw[:n_out.value], mod.value


def _keep_of(copy_tags):
    """map_bam_file's copy_tags as mm355_fastx_keep_aux takes it: None for none, "*" for all, or the names back to back"""
    if copy_tags is None or copy_tags is False:
        return None
    if copy_tags is True:
        return b"*"
    try:
        names = list(copy_tags) if not isinstance(copy_tags, (str, bytes)) else None
    except TypeError:
        names = None
    if not names or not all(isinstance(t, str) and len(t) == 2 and t.isascii() and t.isprintable() for t in names):
        raise ValueError("`copy_tags` must be False, True, or an iterable of two-letter tag names")
    return "".join(names).encode()


def bgzf_wrap(data, *, compress=False):
    """`data` (bytes) in stored BGZF blocks of at most 0xff00 bytes of payload each (mm355_bgzf_wrap on the host); b"" gives b"".
    compress=True: every block deflated where that is shorter (mm355_bgzf_deflate at level 1, on the host)"""
    L = _ffi.lib()
    tp = C.POINTER(_ffi.Text)()
    if compress:
        _ffi.check(L.mm355_bgzf_deflate(None, data, len(data), _ffi.PAF_HOST, 1, C.byref(tp)))
    else:
        _ffi.check(L.mm355_bgzf_wrap(None, data, len(data), _ffi.PAF_HOST, C.byref(tp)))
    try:
        return bytes(_ffi.text_view(tp))
    finally:
        L.mm355_free_text(tp)


def bgzf_unwrap(data):
    """the host inverse of bgzf_wrap: the payloads of the BGZF members of `data` (bytes), back to back (mm355_bgzf_inflate on the host);
    b"" gives b"".  Data that does not begin with a BGZF member, a malformed member and one the decoder refuses (a corrupt deflate stream,
    a CRC-32 or ISIZE that is not the trailer's) raise"""
    L = _ffi.lib()
    tp = C.POINTER(_ffi.Text)()
    _ffi.check(L.mm355_bgzf_inflate(None, data, len(data), _ffi.PAF_HOST, C.byref(tp)))
    try:
        return bytes(_ffi.text_view(tp))
    finally:
        L.mm355_free_text(tp)


def shard_by_bases(lengths, n_shards):
    """a batch is cut into `n_shards` CONTIGUOUS shards balanced by cumulative bases (not by read count): a read belongs to
    the shard that contains the midpoint of its span on the cumulative-bases axis.  Returns n_shards+1 boundaries b with shard
    s = items[b[s]:b[s+1]]; every item belongs to exactly one shard."""
    n_shards = max(1, int(n_shards))
    lengths = np.asarray(lengths, dtype=np.int64)
    n = len(lengths)
    if n == 0:
        return [0] * (n_shards + 1)
    cum = np.cumsum(lengths)
    total = max(1, int(cum[-1]))
    mid2 = 2 * cum - lengths                      # twice the midpoint, exact in integers
    shard = np.minimum(n_shards - 1, (mid2 * n_shards) // (2 * total))
    return [int(np.searchsorted(shard, s, side="left")) for s in range(n_shards)] + [n]


def order_by_length(lengths):
    """indices of the reads, longest first (stable).  The per-read kernels of a sub-batch cost the latency of its longest read, so a
    dispatcher that has a window of pending reads cuts its sub-batches from this order: sub-batches of similar reads, the few very long
    ones together"""
    return np.argsort(-np.asarray(lengths, dtype=np.int64), kind="stable").tolist()


def _cs_flag(cs):
    """the flag bits of a `cs=` argument: False (no cs), True or "short" (minimap2 --cs, `:123*ag+tt-c`), "long" (--cs=long, `=ACGT*ag+tt-c`:
    the matched bases spelled out, what tools that rebuild both sequences of an alignment need).  Anything else: ValueError."""
    if cs is None or (isinstance(cs, (bool, int)) and cs in (0, 1)):
        return _ffi.OUT_CS if cs else 0
    if isinstance(cs, str) and cs == "short":
        return _ffi.OUT_CS
    if isinstance(cs, str) and cs == "long":
        return _ffi.OUT_CS_LONG
    raise ValueError("`cs` must be False, True, 'short' or 'long'")


# one entry point of the C-ABI that maps reads and writes records: the function; whether it takes qualities and sam_flags (SAM, BAM); whether it
# takes the three aux arguments; what stands between `where` and the result; the result's type (_ffi.Text, or _ffi.Run for a sorted call)
_Entry = collections.namedtuple("_Entry", "fn sam aux tail out")


def _check_reads(seqs, names, quals=None):
    """the reads of a one-call writer, checked: (seqs as a list, names as a list or None, None or (the qualities as a char* array, what it
    points into))"""
    seqs = list(seqs)
    for s in seqs:
        if not isinstance(s, str):
            raise TypeError("argument 'seq': 'bytes' object cannot be converted to 'PyString'" if isinstance(s, bytes)
                            else "argument 'seq' must be str")
    if names is not None:
        names = list(names)
        if len(names) != len(seqs) or not all(nm is None or isinstance(nm, str) for nm in names):
            raise ValueError("`names` must hold a string or None for every read")
    if quals is None:
        return seqs, names, None
    quals = list(quals)
    if len(quals) != len(seqs) or not all(q is None or (isinstance(q, str) and len(q) == len(s) and q.isascii()) for q, s in zip(quals, seqs)):
        raise ValueError("`quals` must hold None or an ASCII string of the read's length for every read")
    if not all(q is None or s.isascii() for q, s in zip(quals, seqs)):
        raise ValueError("a read that has a quality string must be ASCII: its quality is matched to it byte by byte")
    qkeep = [None if q is None else q.encode() for q in quals]
    return seqs, names, ((C.c_char_p * len(qkeep))(*qkeep), qkeep)


# what map_bam_file adds to a map_file call (map_bam_file's docstring)
_FileOpts = collections.namedtuple("_FileOpts", "sam_flags compress read_on_gpu keep_aux sort tmp_dir index tmp_compress",
                                   defaults=(0, False, False, None, False, None, False, False))

# what a worker of _map_file hands on for one sub-batch: the result record (mm355_text_t or mm355_run_t), its reads, bases and bytes of kept tags
_SubBatch = collections.namedtuple("_SubBatch", "tp n_reads n_bases n_aux")

# the sorted run of one sub-batch as the merge needs it: the records' keys and lengths in key order, where the run's bytes begin in the spool,
# the records' spans (index=True; else empty), and the offsets of its BGZF members in its bytes (a packed run; else None)
_Run = collections.namedtuple("_Run", "keys lens place spans blk_off")


class _TextSink:
    """where the results of an unsorted file go: the texts, written in input order"""

    def __init__(self, out):
        self.out, self.n_lines, self.n_dev, self.ms_format, self.n_out = out, 0, 0, 0.0, 0

    def take(self, k, tp):
        t = tp.contents
        self.n_lines += int(t.n_lines); self.n_dev += int(t.on_device); self.ms_format += float(t.ms_format); self.n_out += int(t.n_text)
        self.out.write(_ffi.text_view(tp))


class _RunSpool:
    """where the results of a sorted file go: every run's bytes (its records; the BGZF members of a packed run) appended to the temporary
    file as the runs complete, and per run the tables the merge needs (24 bytes per record, 32 with spans)"""

    def __init__(self, tmp, index, packed):
        self.tmp, self.index, self.packed = tmp, index, packed
        self.runs, self.n_tmp, self.n_raw = {}, 0, 0      # per sub-batch; the spool's bytes; packed: the bytes of the records its members hold
        self.n_lines, self.n_dev, self.ms_format = 0, 0, 0.0

    def take(self, k, tp):
        t = tp.contents
        n = int(t.n_rec)
        self.n_lines += n; self.n_dev += int(t.on_device); self.ms_format += float(t.ms_sort)
        keys = np.ctypeslib.as_array(t.key, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
        lens = np.diff(np.ctypeslib.as_array(t.rec_off, shape=(n + 1,))) if n else np.zeros(0, np.int64)
        spans = np.ctypeslib.as_array(t.span, shape=(n,)).copy() if self.index and n else np.zeros(0, np.int64)
        blk_off = None
        if self.packed:
            blk_off = np.ctypeslib.as_array(t.blk_off, shape=(int(t.n_blk) + 1,)).copy()
            self.n_raw += int(t.rec_off[n])
        self.runs[k] = _Run(keys, lens, self.n_tmp, spans, blk_off)
        if t.n_bytes:
            self.tmp.write(memoryview((C.c_char * int(t.n_bytes)).from_address(C.addressof(t.rec.contents))))
        self.n_tmp += int(t.n_bytes)


class _GatherStep:
    """a step of the merge of plain runs: the records gathered from the spool (mm355_bam_gather) into a host buffer behind the bytes the
    last step left over, and the whole payloads framed (level 0, on the host: no context) or deflated (mm355_bgzf_deflate on the device)"""

    def __init__(self, L, level):
        self.L, self.level, self.where = L, level, _ffi.PAF_DEVICE if level else _ffi.PAF_HOST

    def begin(self, runs, order, spool):
        self.spool, self.carry = spool, np.zeros(0, np.uint8)
        self.src = np.ascontiguousarray(np.concatenate([r.place + np.cumsum(r.lens, dtype=np.int64) - r.lens for r in runs])[order])

    def blocks(self, ctx, i, lens, last):
        L, carry, j, n_new = self.L, self.carry, i + len(lens), int(lens.sum())
        buf = np.empty(len(carry) + n_new, np.uint8)
        buf[:len(carry)] = carry
        _ffi.check(L.mm355_bam_gather(self.spool.ctypes.data, len(self.spool), self.src[i:j].ctypes.data, lens.ctypes.data, j - i, buf.ctypes.data + len(carry), n_new))
        # whole payloads now; what is left opens the next step's buffer (the last step writes everything)
        n_now = len(buf) if last else len(buf) // 0xff00 * 0xff00
        self.carry = buf[n_now:].copy()
        if not n_now:
            return None
        tp = C.POINTER(_ffi.Text)()
        _ffi.check(L.mm355_bgzf_deflate(ctx, C.cast(buf.ctypes.data, C.c_char_p), n_now, self.where, self.level, C.byref(tp)))
        return tp


class _PackedStep:
    """a step of the merge of packed runs (map_bam_file(tmp_compress=True)).  A step is a contiguous range of the merged order, so it takes
    from every run a contiguous range of that run's records: record counts per run (a bincount) and a running count of what earlier
    steps took give the raw range [lo, hi) each run contributes, the members [lo // 0xff00, ceil(hi / 0xff00)) hold it, and one
    mm355_bam_merge_step call turns the slices and the records' places into the step's blocks, the leftover bytes staying with the call.
    The file writers run it on the device whatever the level; the host `where` is the C-ABI's and the tests'."""

    def __init__(self, L, level, where=_ffi.PAF_DEVICE):
        self.L, self.level, self.where = L, level, where

    def begin(self, runs, order, spool):
        n_runs = len(runs)
        counts = np.array([len(r.keys) for r in runs], np.int64)
        self.spool = spool
        self.run_of = np.repeat(np.arange(n_runs, dtype=np.int64), counts)[order]
        self.raw_all = np.concatenate([np.concatenate(([0], np.cumsum(r.lens, dtype=np.int64))) for r in runs])     # per run its n + 1 raw offsets
        self.raw_first = np.cumsum(counts + 1) - (counts + 1)
        self.at = np.ascontiguousarray(np.concatenate([np.cumsum(r.lens, dtype=np.int64) - r.lens for r in runs])[order])   # a record's place in its run's unframed stream
        self.blk_all = np.concatenate([r.blk_off for r in runs]).astype(np.int64, copy=False)                      # per run its n_blk + 1 member offsets
        blk_n = np.array([len(r.blk_off) for r in runs], np.int64)
        self.blk_first = np.cumsum(blk_n) - blk_n
        self.place = np.array([r.place for r in runs], np.int64)
        self.carry, self.n_carry = np.empty(0xff00, np.uint8), C.c_int64(0)
        self.taken = np.zeros(n_runs, np.int64)          # the records of every run that earlier steps took
        self.slice_of_run = np.empty(n_runs, np.int32)

    def blocks(self, ctx, i, lens, last):
        P, j, carry = 0xff00, i + len(lens), self.carry
        took = np.bincount(self.run_of[i:j], minlength=len(self.taken))
        sel = np.flatnonzero(took)
        first = self.raw_first[sel] + self.taken[sel]
        lo, hi = self.raw_all[first], self.raw_all[first + took[sel]]
        m_lo, m_hi = lo // P, (hi + P - 1) // P
        b_lo, b_hi = self.blk_all[self.blk_first[sel] + m_lo], self.blk_all[self.blk_first[sel] + m_hi]
        slice_at, slice_bytes, slice_raw_at = np.ascontiguousarray(self.place[sel] + b_lo), np.ascontiguousarray(b_hi - b_lo), np.ascontiguousarray(m_lo * P)
        self.slice_of_run[sel] = np.arange(len(sel), dtype=np.int32)
        rec_slice = np.ascontiguousarray(self.slice_of_run[self.run_of[i:j]])
        self.taken += took
        tp = C.POINTER(_ffi.Text)()
        _ffi.check(self.L.mm355_bam_merge_step(ctx, self.spool.ctypes.data, len(self.spool), slice_at.ctypes.data, slice_bytes.ctypes.data, slice_raw_at.ctypes.data, len(sel),
                                               rec_slice.ctypes.data, self.at[i:j].ctypes.data, lens.ctypes.data, j - i, carry.ctypes.data, self.n_carry.value,
                                               1 if last else 0, self.where, self.level, C.byref(tp), carry.ctypes.data, C.byref(self.n_carry)))
        return tp


def _merge(L, runs, spool, out, step, bai=None, contexts=None):
    """the merge phase of map_bam_file(sort=True).  runs: the _Run of every sub-batch, in input order, the records of a run in key order;
    spool: their bytes, one array (the memory-mapped temporary file).  The stable argsort of the concatenated keys is the k-way merge -- and
    the stable sort of the unsorted file, because ties inside a run are in input order already.  The merged order is cut into steps of
    SORT_CHUNK_BYTES; `step` (_GatherStep, _PackedStep) makes the BGZF blocks of each, carrying what does not fill a block into the next, and
    they are written to `out`.  Array operations and one or two library calls per step: no Python work per record.
    bai: the .bai builder -- it gets the ordered keys, spans and lengths once, and every step's blocks as they are written.
    contexts: (acquire, release) of the pool; one is taken for the steps where `step` runs on the device, none otherwise.
    Returns (the bytes written, the seconds spent in the builder's calls)"""
    keys = np.concatenate([r.keys for r in runs]) if runs else np.zeros(0, np.uint64)
    if len(keys) == 0:
        return 0, 0.0
    order = np.argsort(keys, kind="stable")
    lens = np.ascontiguousarray(np.concatenate([r.lens for r in runs]).astype(np.int64, copy=False)[order])
    n_out, t_index = 0, 0.0
    if bai is not None:
        t_ix = time.perf_counter()
        keys, spans = np.ascontiguousarray(keys[order]), np.ascontiguousarray(np.concatenate([r.spans for r in runs])[order])
        _ffi.check(L.mm355_bai_records(bai, keys.ctypes.data, spans.ctypes.data, lens.ctypes.data, len(lens)))
        t_index += time.perf_counter() - t_ix
    end_at = np.cumsum(lens)                         # the sorted stream's offset behind every record
    step.begin(runs, order, spool)
    dev_ctx = contexts[0](0) if step.where == _ffi.PAF_DEVICE else None
    try:
        i, n = 0, len(lens)
        while i < n:
            base = int(end_at[i - 1]) if i else 0
            j = max(i + 1, int(np.searchsorted(end_at, base + SORT_CHUNK_BYTES, side="right")))
            tp = step.blocks(dev_ctx[1] if dev_ctx else None, i, lens[i:j], j == n)
            i = j
            if tp is None:
                continue
            try:
                if tp.contents.n_text:
                    n_out += int(tp.contents.n_text)
                    out.write(_ffi.text_view(tp))
                    if bai is not None:
                        t_ix = time.perf_counter()
                        _ffi.check(L.mm355_bai_blocks(bai, C.addressof(tp.contents.text.contents), int(tp.contents.n_text)))
                        t_index += time.perf_counter() - t_ix
            finally:
                L.mm355_free_text(tp)
    finally:
        if dev_ctx is not None:
            contexts[1](dev_ctx)
    return n_out, t_index


class Aligner:
    """mappy-compatible aligner (lib.rs:288-671) whose mapping path runs on MI355X GPUs.

    `device` / `devices` are the only additions to the reference's constructor: the GPU (or list of GPUs of one node) that map
    this Aligner's reads.  With several devices the index is replicated into each one's HBM (mm355_upload) and `map_batch` deals
    its sub-batches to the contexts of all of them -- the GPU analogue of the reference's N worker threads over one shared index
    (lib.rs:541-636).  Reads are independent: no collective.

    `build_on_gpu=True` (keyword-only) builds the index of a FASTA / FASTQ on devices[0] instead of on the host (mm355_index_load_device);
    `save_index(path)` writes any index as an .mmi, so that a reference is indexed once and loaded from then on.
    `load_on_gpu=True` (keyword-only) loads an .mmi straight into the HBM of devices[0] (mm355_index_load_mmi_device): no host table is made.
    A file that is not an .mmi takes the usual route, so `build_on_gpu=True, load_on_gpu=True` keeps the index on the GPU whatever the file is."""

    def __init__(self, fn_idx_in=None, preset=None, k=None, w=None, min_cnt=None, min_chain_score=None,
                 min_dp_score=None, bw=None, best_n=None, n_threads=3, fn_idx_out=None, max_frag_len=None,
                 extra_flags=None, seq=None, scoring=None, device=0, devices=None, *, cigar=True, tags=False, name_key=None,
                 build_on_gpu=False, load_on_gpu=False):
        L = _ffi.lib()
        self._L = L
        self._idx = C.c_void_p()
        self._ctx = C.c_void_p()
        self._wctx = {}                      # device -> free contexts of the map_batch pipeline workers (one per host thread)
        self._name_cache = None
        self._devices = [int(d) for d in devices] if devices is not None else [int(device)]
        if not self._devices:
            raise ValueError("`devices` must name at least one GPU")
        self._device = self._devices[0]
        self._n_threads = 0
        self._lock = threading.Lock()
        # tags=True: every mapping call asks for the mm355_tags_t rows (MM355_OUT_TAGS): the records carry minimap2's PAF tags (s1, dv, de, rl ...)
        self._tag_flag = _ffi.OUT_TAGS if tags else 0
        # name_key: map_batch passes item[name_key] as the read's query name (mappy's map(seq, name=...)); a missing key or None = unnamed
        self._name_key = name_key
        io, mo = _ffi.IdxOpt(), _ffi.MapOpt()
        L.mm355_set_opt(None, C.byref(io), C.byref(mo))
        if preset is not None:
            rc = L.mm355_set_opt(str(preset).encode(), C.byref(io), C.byref(mo))
            # The reference ignores mm_set_opt's return value (lib.rs:336): an unknown name leaves the defaults in place, silently, and so
            # does this mirror (MM355_EINVAL).  A preset minimap2 knows but this path does not implement (sr, splice ...) must not be
            # mapped with other parameters behind the caller's back: refuse.
            if rc == _ffi.MM355_EUNSUP:
                raise NotImplementedError("preset %r is not implemented by the MI355X mapping path (long-read presets only: map-ont, "
                                          "map-hifi, map-pb, asm5/asm10/asm20, ava-ont, ava-pb)" % (preset,))
        if cigar:
            mo.flag |= 4                   # MM_F_CIGAR, lib.rs:339; cigar=False: chain-only mapping (minimap2 without -c), no extension
        io.batch_size |= 0x7fffffffffffffff  # lib.rs:340
        if k is not None: io.k = k
        if w is not None: io.w = w
        if min_cnt is not None: mo.min_cnt = min_cnt
        if min_chain_score is not None: mo.min_chain_score = min_chain_score
        if min_dp_score is not None: mo.min_dp_max = min_dp_score
        if bw is not None: mo.bw = bw
        if best_n is not None: mo.best_n = best_n
        if max_frag_len is not None: mo.max_frag_len = max_frag_len
        if extra_flags is not None: mo.flag |= extra_flags
        if scoring is not None and len(scoring) >= 4:
            mo.a, mo.b, mo.q, mo.e = (int(x) for x in scoring[:4])
            mo.q2, mo.e2 = mo.q, mo.e
            if len(scoring) >= 6:
                mo.q2, mo.e2 = int(scoring[4]), int(scoring[5])
                if len(scoring) >= 7:
                    mo.sc_ambi = int(scoring[6])
        self._io, self._mo = io, mo
        if seq is not None:
            raise NotImplementedError("Not Implemented")
        if fn_idx_out is not None:
            raise NotImplementedError("Not Implemented")
        if fn_idx_in is None:
            raise RuntimeError("Did not create or open an index")
        path = str(fn_idx_in).encode()
        rc = _ffi.MM355_EINVAL
        if load_on_gpu:                    # an .mmi goes into the HBM of devices[0] in pieces; MM355_EINVAL = not an .mmi: the routes below
            rc = L.mm355_index_load_mmi_device(path, self._device, C.byref(self._idx))
        if rc == _ffi.MM355_EINVAL and build_on_gpu:   # a FASTA / FASTQ is sketched, sorted and tabled on devices[0]; an .mmi loads as below
            rc = L.mm355_index_load_device(path, C.byref(io), self._device, C.byref(self._idx))
        elif rc == _ffi.MM355_EINVAL:
            rc = L.mm355_index_load(path, C.byref(io), int(n_threads), C.byref(self._idx))
        if rc != 0 or not self._idx:
            raise RuntimeError("Did not create or open an index")
        L.mm355_mapopt_update(C.byref(mo), self._idx)
        if len(self._devices) > 1:         # replicate now, so that the first map_batch does not pay for it
            arr = (C.c_int32 * len(self._devices))(*self._devices)
            rc = L.mm355_upload(self._idx, arr, len(self._devices))
            if rc != 0:
                raise RuntimeError("mm355: " + L.mm355_strerror(rc).decode())

    # ---- properties (lib.rs:439-470, 651-670)
    def _info(self):
        k, w, b, fl, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint32()
        self._L.mm355_index_info(self._idx, C.byref(k), C.byref(w), C.byref(b), C.byref(fl), C.byref(n))
        return k.value, w.value, b.value, fl.value, n.value

    def __bool__(self):
        return bool(self._idx)

    @property
    def k(self): return self._info()[0]

    @property
    def w(self): return self._info()[1]

    @property
    def n_seq(self): return self._info()[4]

    @property
    def seq_names(self):
        if not self._idx:
            raise RuntimeError("Index hasn't loaded")
        return [self._L.mm355_index_seq_name(self._idx, i).decode() for i in range(self.n_seq)]

    def seq(self, name, start=0, end=0x7fffffff):
        """lib.rs:464-470 with the rules of lib.rs:706-766: None on any error (incl. "No sequence in this index", lib.rs:710-714)."""
        L = self._L
        if not self._idx:
            return None
        if (self._mo.flag & 4) and (self._info()[3] & 2):      # MM_F_CIGAR && MM_I_NO_SEQ
            return None
        rid = L.mm355_index_name2id(self._idx, name.encode())
        if rid < 0:
            return None
        ln = L.mm355_index_seq_len(self._idx, rid)
        if start >= ln or start >= end:
            return None
        if end < 0 or end > ln:
            end = ln
        buf = (C.c_uint8 * (end - start))()
        n = L.mm355_index_getseq(self._idx, rid, start, end, buf)
        if n < 0:
            return None
        return bytes(buf[:n]).translate(bytes.maketrans(b"\x00\x01\x02\x03\x04", b"ACGTN")).decode()

    def save_index(self, path):
        """writes the index as a minimap2 .mmi (mm355_index_dump; the reference's `fn_idx_out`, lib.rs:391-394, as a method): any index, also
        one built with build_on_gpu=True.  Aligner(path), minimap2 and mappy load the file."""
        rc = self._L.mm355_index_dump(self._idx, os.fsencode(path))
        if rc != 0:
            raise RuntimeError("mm355: " + self._L.mm355_strerror(rc).decode())

    # ---- device context
    def _context(self):
        if not self._ctx:
            rc = self._L.mm355_ctx_create(self._idx, self._device, C.byref(self._ctx))
            if rc != 0:
                raise RuntimeError("mm355: " + self._L.mm355_strerror(rc).decode())
        return self._ctx

    def _map_many(self, seqs, flags, ctx=None, names=None):
        """one mm355_map_batch call; returns list of list[Mapping].  ctx: a pipeline worker's own context (no lock needed).
        names: query names (str or None per read); None or all None = the unnamed call"""
        L = self._L
        packed, narr = _ffi.pack_reads(seqs), _ffi.pack_names(names)
        own = ctx is None               # the Aligner's own context is shared: under the lock
        with self._lock if own else contextlib.nullcontext():
            rc, hp = _ffi.call_map(L, self._context() if own else ctx, self._mo, packed, flags, narr)
        _ffi.check(rc)
        return _batch_to_mappings(_ffi.take_hits(L, hp, len(seqs)), len(seqs), self._names(), chain_only=not self._mo.flag & 4)

    def _names(self):
        if self._name_cache is None:
            self._name_cache = [nm.decode() if nm is not None else None for nm in (self._L.mm355_index_seq_name(self._idx, i) for i in range(self.n_seq))]
        return self._name_cache

    def _ctx_acquire(self, slot):
        """a free worker context on GPU devices[slot % n_devices] (created on demand; contexts are pooled per device and never shared
        between two running workers, also not between two overlapping map_batch calls)"""
        dev = self._devices[slot % len(self._devices)]
        with self._lock:
            free = self._wctx.setdefault(dev, [])
            if free:
                return dev, free.pop()
        ctx = C.c_void_p()
        _ffi.check(self._L.mm355_ctx_create(self._idx, dev, C.byref(ctx)))
        return dev, ctx

    def _ctx_release(self, dev_ctx):
        with self._lock:
            self._wctx.setdefault(dev_ctx[0], []).append(dev_ctx[1])

    # ---- single read (lib.rs:473-514)
    def map(self, seq, seq2=None, cs=False, MD=False, *, name=None):
        """name: the read's query name (mappy's `name`): it enters the hash that orders regions of equal score, and with the ava-ont / ava-pb
        presets (MM_F_NO_DIAG / MM_F_NO_DUAL) it filters self hits and the second report of every pair.  None = an unnamed read."""
        if seq2 is not None:
            raise NotImplementedError("Using `seq2` is not implemented")
        if not isinstance(seq, str):
            raise TypeError("argument 'seq': 'bytes' object cannot be converted to 'PyString'" if isinstance(seq, bytes)
                            else "argument 'seq' must be str")
        cs_flag = _cs_flag(cs)
        if (cs_flag or MD) and not self._mo.flag & 4:
            raise ValueError("cs / MD need base-level alignment: this Aligner was created with cigar=False")
        if name is not None and not isinstance(name, str):
            raise ValueError("`name` must be a string")
        flags = cs_flag | (_ffi.OUT_MD if MD else 0) | self._tag_flag
        r = self._map_many([seq], flags, names=None if name is None else [name])[0]
        if isinstance(r, Exception):
            raise r
        return r

    def map_no_op(self, _seq, seq2=None, _cs=False, _MD=False):
        """canned record of lib.rs:675-693 (binding-overhead probe)"""
        if seq2 is not None:
            raise NotImplementedError("Using `seq2` is not implemented")
        return [Mapping(0, 1000, 1, "Hello", 101010, 10, 1010, 1000, 1000, 60, True, [], 0, None, "Cigar string")]

    # ---- batch path (lib.rs:541-648, 771-906)
    def enable_threading(self, n_threads):
        """In the reference this spawns N mm_map worker threads; here it arms the GPU batch path: map_batch drives up to
        min(n_threads, 8) host threads per GPU, each with its own context (HIP streams + buffers)."""
        self._n_threads = int(n_threads)

    def map_batch(self, seqs, back_off=True, *, cs=True):
        """lib.rs:639-648, 771-906.  The iterable is consumed completely before the iterator is returned (lib.rs:845-903), but -- as in the
        reference, whose workers pop the queue while `_map_batch` is still pushing -- mapping starts as soon as the first sub-batch of reads
        has been taken from it, and results stream out of the returned iterator in completion order while later sub-batches are still on the
        GPU (lib.rs:793-839: collector thread -> bounded channel -> `__next__`)."""
        cs_flag = _cs_flag(cs)           # cs (keyword-only): True = the reference's hard-wired short form (lib.rs:589); "short", "long", False as in map()
        if cs_flag == _ffi.OUT_CS_LONG and not self._mo.flag & 4:
            raise ValueError("cs / MD need base-level alignment: this Aligner was created with cigar=False")
        if self._n_threads == 0:
            raise RuntimeError("Multi threading not enabled on this instance. Please call `.enable_threading()`")
        # accepted iterables: list / tuple / iterator / generator / sequence -- not dict, not str (lib.rs:782-792, 910-920)
        if isinstance(seqs, (dict, str, bytes)) or not (isinstance(seqs, (list, tuple, collections.abc.Sequence)) or
                                                        isinstance(seqs, collections.abc.Iterator)):
            raise TypeError("Unsupported batch type, pass a list, iter, generator or tuple")
        max_workers = max(1, min(self._n_threads, 8)) * len(self._devices)
        try:
            n_known = len(seqs)
        except TypeError:
            n_known = None
        # sub-batch size: at most SUB_BATCH_READS; small inputs are cut finer so that every worker gets about two sub-batches (16384 reads:
        # 1024 per sub-batch maps 20 % faster than 4096).  Unknown length (iterators): ramp up, so that the first results leave early.
        sb_reads = SUB_BATCH_READS
        sb_fixed = None if n_known is None else min(sb_reads, max(1024, -(-n_known // (2 * max_workers))))

        def size_of(k):
            return sb_fixed if sb_fixed is not None else min(sb_reads, 512 << min(4, k // max_workers))
        name_key = self._name_key

        def names_of(items):
            """query names of a sub-batch (None without name_key or when no item has one); a name that is not str: ValueError, like `seq`"""
            if name_key is None:
                return None
            names = [it.get(name_key) for it in items]
            if all(nm is None for nm in names):
                return None
            if not all(nm is None or isinstance(nm, str) for nm in names):
                raise ValueError("`%s` must be a string" % (name_key,))
            return names
        out_flags = (cs_flag if self._mo.flag & 4 else 0) | self._tag_flag        # chain-only: no cs string to produce
        self._names()                       # fill the name cache before the workers read it
        # the caps are module globals read per call (tests and tools set them); the cut and the engine of mappy_rs/_batch.py get them as arguments
        run = _batch.BatchRun(functools.partial(self._map_sub, out_flags), self._ctx_acquire, self._ctx_release, max_workers,
                              WORK_QUEUE_CAP, RESULT_CHANNEL_CAP, back_off)
        try:
            for reads, items in _batch.sub_batches(seqs, size_of, SUB_BATCH_BASES, WORK_QUEUE_CAP, back_off):
                run.submit(reads, items, names_of(items))     # (names_of raises in the caller's thread, before the sub-batch is queued)
        except BaseException:
            run.abort()                     # nothing is yielded: the workers stop after their current sub-batch
            raise
        return run.finish()

    def _map_sub(self, flags, dev_ctx, reads, names):
        """one sub-batch of map_batch on a worker's (device, context); cs=true, MD=false: lib.rs:589-590"""
        return self._map_many(reads, flags, dev_ctx[1]) if names is None else self._map_many(reads, flags, dev_ctx[1], names=names)

    # ---- PAF text (mm355_map_batch_paf): the lines of mappy_rs.paf_line, formatted by the library -- on the device for large batches
    def _paf_flags(self, cs, MD):
        cs_flag = _cs_flag(cs)
        if (cs_flag or MD) and not self._mo.flag & 4:
            raise ValueError("cs / MD need base-level alignment: this Aligner was created with cigar=False")
        return cs_flag | (_ffi.OUT_MD if MD else 0) | _ffi.OUT_TAGS

    def map_paf(self, seqs, names=None, cs=False, MD=False, *, where=_ffi.PAF_AUTO):
        """the PAF lines of `seqs` (a list of str) as bytes, in input order: one mm355_map_batch_paf call, no Mapping objects.  Each line is
        paf_line() of the record map() would return, tagged whatever `tags=` was; names[i] (str or None) is the read's query name as in
        map(seq, name=...), printed up to its first blank; an unnamed read prints `*`.  An empty sequence writes nothing.
        where (keyword-only): _ffi.PAF_AUTO (the library picks the formatter by the hit count), PAF_HOST or PAF_DEVICE; which one wrote the
        text of the last call is kept in `paf_on_device`."""
        flags = self._paf_flags(cs, MD)
        return self._map_records(seqs, names, None, flags, 0, where, _Entry(self._L.mm355_map_batch_paf, False, False, (), _ffi.Text))

    paf_on_device = None              # whether the device formatter wrote the text of the last map_paf / map_sam call

    # ---- SAM text (mm355_map_batch_sam): the lines of mappy_rs.sam_lines, formatted by the library
    def sam_header(self, rg=b"", *, sort=False):
        """the SAM header of this index as bytes: @HD (unsorted, grouped by query), one @SQ per contig in index order, @PG of this library;
        rg: @RG lines (bytes, newline-terminated) to stand between the @SQ lines and @PG.  sort=True: @HD says SO:coordinate (the header of
        a file map_bam_file(sort=True) writes)"""
        L = self._L
        sq = "".join("@SQ\tSN:%s\tLN:%d\n" % (nm, L.mm355_index_seq_len(self._idx, i)) for i, nm in enumerate(self._names()))
        hd = "@HD\tVN:1.6\tSO:coordinate\n" if sort else "@HD\tVN:1.6\tSO:unsorted\tGO:query\n"
        return (hd + sq).encode() + bytes(rg) + b"@PG\tID:mappy_rs\tPN:mappy_rs\n"

    def _sam_flags(self, cs, MD):
        if not self._mo.flag & 4:
            raise ValueError("SAM needs base-level alignment: this Aligner was created with cigar=False")
        return _cs_flag(cs) | (_ffi.OUT_MD if MD else 0)

    def map_sam(self, seqs, names=None, quals=None, cs=False, MD=False, *, softclip=False, hit_only=False, where=_ffi.PAF_AUTO):
        """the SAM lines of `seqs` (a list of str) as bytes, without a header (sam_header()), in input order: one mm355_map_batch_sam call, no
        Mapping objects.  The lines of a read are sam_lines() of the records map() would return with tags; a read without hits writes one
        unmapped record unless hit_only (minimap2 --sam-hit-only); an empty sequence writes nothing.  names as in map_paf; quals[i] is None or
        a str as long as the read; softclip: minimap2 -Y.  where and `paf_on_device`: as for map_paf."""
        sam_flags = (_ffi.SAM_SOFTCLIP if softclip else 0) | (_ffi.SAM_HIT_ONLY if hit_only else 0)
        return self._map_records(seqs, names, quals, self._sam_flags(cs, MD), sam_flags, where, _Entry(self._L.mm355_map_batch_sam, True, False, (), _ffi.Text))

    def _bam_entry(self, level, aux, sort, index=False, packed=False):
        """the entry point of a BAM call, chosen once from what the call asks for: sorted calls return a run (with spans for the index, packed
        for a compressed spool) and always take the aux arguments; an unsorted call takes them only where there are tags"""
        L = self._L
        if sort and packed:
            return _Entry(L.mm355_map_batch_bam_run_packed, True, True, (1 if index else 0,), _ffi.Run)
        if sort:
            return _Entry(L.mm355_map_batch_bam_run_span if index else L.mm355_map_batch_bam_run, True, True, (), _ffi.Run)
        if aux:
            return _Entry(L.mm355_map_batch_bam_aux, True, True, (level,), _ffi.Text)
        if level:
            return _Entry(L.mm355_map_batch_bam_deflate, True, False, (1,), _ffi.Text)
        return _Entry(L.mm355_map_batch_bam, True, False, (), _ffi.Text)

    def _call_entry(self, e, ctx, reads, quals, aux, flags, sam_flags, where):
        """one call of the entry point `e` on `ctx`: reads = (n, seqs, lens, names) and aux = (blocks, lengths, mod_off) as the C-ABI takes
        them; returns (rc, the pointer to the result record)"""
        tp = C.POINTER(e.out)()
        a = (ctx, C.byref(self._mo)) + tuple(reads) + ((quals,) if e.sam else ()) + (tuple(aux) if e.aux else ()) + (flags,) + ((sam_flags,) if e.sam else ())
        return e.fn(*a, int(where), *e.tail, C.byref(tp)), tp

    def _take_text(self, rc, tp, note=True):
        """the end of a one-call writer: rc checked, which formatter wrote the text kept in `paf_on_device` (note), the text as bytes, the record freed"""
        if rc != 0:
            raise RuntimeError(self._L.mm355_strerror(rc).decode())
        try:
            if note:
                self.paf_on_device = bool(tp.contents.on_device)
            return bytes(_ffi.text_view(tp))
        finally:
            self._L.mm355_free_text(tp)

    def _map_records(self, seqs, names, quals, flags, sam_flags, where, entry, aux=(None, None, None), run_level=0):
        """map_paf / map_sam / map_bam: the arguments checked, one call of `entry` on the aligner's own context, the text as bytes.
        An entry that returns a run (map_bam(sort=True)): its records go through mm355_bgzf_deflate at run_level"""
        seqs, names, qarr = _check_reads(seqs, names, quals)
        L, note = self._L, entry.out is _ffi.Text
        packed, narr = _ffi.pack_reads(seqs), _ffi.pack_names(names)
        with self._lock:
            rc, tp = self._call_entry(entry, self._context(), (len(seqs), packed.arr, packed.lens, narr), qarr and qarr[0], aux, flags, sam_flags, where)
            if rc == 0 and not note:        # a run: deflated where the records were sorted; stored blocks are the host's (mm355_bgzf_wrap's rule)
                rp, tp = tp, C.POINTER(_ffi.Text)()
                r = rp.contents
                self.paf_on_device = bool(r.on_device)
                rc = L.mm355_bgzf_deflate(self._context(), C.cast(r.rec, C.c_char_p), r.n_bytes, _ffi.PAF_DEVICE if run_level and r.on_device else _ffi.PAF_HOST,
                                          run_level, C.byref(tp))
                L.mm355_free_run(rp)
        return self._take_text(rc, tp, note)

    # ---- BAM records (mm355_map_batch_bam): the BAM encoding of map_sam's lines in stored BGZF blocks, formed by the library
    def map_bam(self, seqs, names=None, quals=None, cs=False, MD=False, *, softclip=False, hit_only=False, where=_ffi.PAF_AUTO, compress=False, aux=None, sort=False):
        """the BAM records of `seqs` as bytes: whole BGZF blocks (stored, not compressed) without the header (bam_header()) and without the
        EOF block (BAM_EOF), in input order; one mm355_map_batch_bam call.  A record is the BAM encoding of the line map_sam writes for the
        same arguments (include/mm355.h states it field by field); the results of consecutive calls, one behind the other, continue the
        stream.  Besides what map_sam refuses: a read name of more than 254 bytes (RuntimeError).  Arguments and `paf_on_device` as for map_sam.
        compress=True: the blocks deflated (mm355_map_batch_bam_deflate at level 1; on the device by a kernel, a workgroup per block): the same
        records behind gzip.decompress, blocks of their real size.
        aux: a list with bytes or None for every read -- the BAM aux tags the read brought along (MM / ML, RG, ...).  Each entry goes through
        mm355_bam_aux_split with "*"; a record that holds the whole read carries all of them behind its own tags, a hard-clipped
        supplementary or a secondary only those that do not index the read's bases (include/mm355.h).  ValueError: a malformed entry,
        with the read's index.
        sort=True: the same records in coordinate order (samtools' key: contig, position, forward before reverse, unmapped last; records of
        equal key in input order) -- one mm355_map_batch_bam_run call, which sorts the records where they were formed, then
        mm355_bgzf_deflate of the sorted stream.  The blocks of THIS call's records: a file of several calls is map_bam_file(sort=True)'s."""
        aux3 = (None, None, None)
        if aux is not None:
            seqs, aux = list(seqs), list(aux)
            if len(aux) != len(seqs) or not all(a is None or isinstance(a, (bytes, bytearray)) for a in aux):
                raise ValueError("`aux` must hold bytes or None for every read")
            n = len(aux)
            keep, lens, mods = [None] * n, (C.c_int32 * n)(), (C.c_int32 * n)()
            for i, a in enumerate(aux):
                if a is None:
                    continue
                try:
                    keep[i], mods[i] = bam_aux_split(a)
                except ValueError:
                    raise ValueError("`aux[%d]` is no well-formed BAM aux block" % i) from None
                lens[i] = len(keep[i])
            aux3 = ((C.c_void_p * n)(*[None if k is None else C.cast(C.c_char_p(k), C.c_void_p).value for k in keep]), lens, mods)
        level = 1 if compress else 0
        sam_flags = (_ffi.SAM_SOFTCLIP if softclip else 0) | (_ffi.SAM_HIT_ONLY if hit_only else 0)
        return self._map_records(seqs, names, quals, self._sam_flags(cs, MD), sam_flags, where, self._bam_entry(level, aux is not None, sort), aux3, run_level=level)

    def bam_header(self, compress=False, rg=b"", *, sort=False):
        """the BAM header of this index as BGZF blocks (compress=True: deflated): the magic, sam_header(rg) as the text, the contigs with their
        lengths.  sort=True: the text is sam_header(rg, sort=True)"""
        text, L = self.sam_header(rg, sort=bool(sort)), self._L
        refs = []
        for i, nm in enumerate(self._names()):
            b = nm.encode()
            refs.append(struct.pack("<I", len(b) + 1) + b + b"\0" + struct.pack("<I", L.mm355_index_seq_len(self._idx, i)))
        return bgzf_wrap(b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs)) + b"".join(refs), compress=bool(compress))

    def map_bam_file(self, reads_path, out_path, cs=False, MD=False, n_threads=None, sub_batch_reads=SUB_BATCH_READS, *, where=_ffi.PAF_AUTO,
                     softclip=False, hit_only=False, compress=False, read_on_gpu=False, copy_tags=False, sort=False, tmp_dir=None, index=False,
                     tmp_compress=False):
        """maps a FASTA / FASTQ file of reads to an uncompressed BAM file (what `samtools view -u` writes; ready for `samtools sort` /
        `index` without a SAM parse): bam_header(), the records of map_bam per sub-batch in input order, BAM_EOF.  The reader, the workers,
        the bound on memory, the ".part" file and its rename, what a failure leaves behind and the returned dict are map_file's; n_lines
        counts records.  A record takes about 1.5 bytes per base with qualities (a SAM line 2) and as much from a FASTA (0xFF per base where
        SAM prints one `*`): the gain is the consumer's, which parses nothing.
        compress=True: a compressed BAM file (what `samtools view -b` writes): bam_header(compress=True), the records of
        map_bam(compress=True) per sub-batch, BAM_EOF; the returned dict also has n_bytes_out, the size of the file.
        read_on_gpu, and a BAM as the reads file: as for map_file.
        copy_tags: False / None drops the aux tags of a BAM reads file; True carries every tag of a read into its records (MM / ML, the
        modified-base calls of a basecaller's BAM, among them); an iterable of two-letter names carries only those (anything else:
        ValueError).  Which record gets which tags: include/mm355.h (a record that holds the whole read gets all, a hard-clipped
        supplementary or a secondary those that do not index bases; the tags the writer emits itself are never copied).  The header then
        has the input's @RG lines between @SQ and @PG, and the returned dict n_aux_bytes: the bytes of kept tags the reader handed on.
        With a reads file that is no BAM the keyword copies nothing.  Works with either reader.
        sort=True: a coordinate-sorted BAM file (what `samtools sort` writes; @HD says SO:coordinate): exactly the stable sort of the file
        the call writes without the keyword, by samtools' key (contig in header order, position, forward before reverse, records without a
        contig last; records of equal key stay in input order), whatever sub_batch_reads, the worker count, the reader or the formatter.
        Two phases.  Runs: every sub-batch is mapped and its records sorted where they were formed (mm355_map_batch_bam_run: on the device
        a radix sort of the keys and a tiled permutation in HBM); the records of each run are appended, uncompressed, to one temporary file
        in `tmp_dir` (default: the directory of out_path), which is unlinked as soon as it is open, and 24 bytes per record (key, length,
        place) stay in memory.  Merge: one stable argsort of all keys, then in steps of SORT_CHUNK_BYTES the records are gathered from the
        memory-mapped temporary file (mm355_bam_gather), framed or deflated (mm355_bgzf_deflate: on the device when compress) and written;
        what does not fill a block is carried into the next step, so the file is bam_header(sort=True), the BGZF blocks of the whole
        sorted stream, BAM_EOF -- the same bytes for any step or sub-batch size.  The temporary file is as large as the uncompressed
        records, about 1.5 bytes per base (tmp_compress=True, below, spools compressed runs instead); memory grows with
        the number of records, not with their bytes.  The returned dict also has
        n_runs, seconds_merge and n_tmp_bytes, and ms_format sums the runs' sort steps.  A failure in either phase removes the ".part"
        file and leaves what was at out_path.  Composes with every other keyword.  map_file (SAM, PAF) has no `sort`.
        index=True (with sort=True only: ValueError otherwise): also writes the .bai index to out_path + ".bai", from numbers the writer has
        in hand -- no second pass over the BAM.  The workers call mm355_map_batch_bam_run_span: on the device k_rec_span sums every
        record's CIGAR on the sorted stream in HBM, and 8 bytes per record come back with the key (32 bytes per record stay in memory
        instead of 24).  The merge gives the ordered keys, spans and lengths to the builder once (mm355_bai_records) and, after every
        step's mm355_bgzf_deflate, the blocks just written (mm355_bai_blocks); mm355_bai_finish makes the file's bytes (include/mm355.h
        states the index rule).  The index goes to out_path + ".bai.part" and is renamed after the BAM's rename; a failure in any phase
        leaves no ".part" file and what was at both paths.  A .bai holds coordinates up to 2^29: a longer contig raises ValueError, naming
        it, before anything is opened or mapped.  The returned dict also has n_index_bytes and seconds_index (the builder's calls and the
        write).  Without the keyword nothing changes: no byte, call, kernel argument or dict key.
        tmp_compress=True (with sort=True only: ValueError otherwise): the same file and the same .bai, byte for byte, from COMPRESSED runs
        -- no record lies uncompressed outside HBM.  The workers call mm355_map_batch_bam_run_packed: the sorted stream of a sub-batch is
        deflated where it lies, and only its BGZF members, keys, offsets and spans come to the host; the temporary file holds members.
        The merge keeps its one stable argsort; a step takes from every run a contiguous range of records, hence of members, and one
        mm355_bam_merge_step call inflates those members on the device, gathers the records behind the bytes the last step left over
        (k_rec_gather), and frames or deflates every whole payload -- on the device whatever `compress` is.  The returned dict's
        n_tmp_bytes is the temporary file's real size, and it gains n_tmp_raw_bytes, the bytes of the records it holds.  Not the default:
        README, "Compressed runs", has the measurements."""
        if tmp_compress and not sort:
            raise ValueError("`tmp_compress=True` needs `sort=True`: only a sorted BAM file is written from runs")
        if index and not sort:
            raise ValueError("`index=True` needs `sort=True`: an unsorted BAM file has no .bai index")
        if index:
            for i, nm in enumerate(self._names()):
                if self._L.mm355_index_seq_len(self._idx, i) > BAI_MAX_LEN:
                    raise ValueError("contig %s is longer than 2^29 bases: a .bai index cannot hold it" % nm)
        sam_flags = (_ffi.SAM_SOFTCLIP if softclip else 0) | (_ffi.SAM_HIT_ONLY if hit_only else 0)
        o = _FileOpts(sam_flags, bool(compress), bool(read_on_gpu), _keep_of(copy_tags), bool(sort), tmp_dir, bool(index), bool(tmp_compress))
        return self._map_file("bam", reads_path, out_path, self._sam_flags(cs, MD), n_threads, sub_batch_reads, where, o)

    def map_file(self, reads_path, out_path, cs=False, MD=False, n_threads=None, sub_batch_reads=SUB_BATCH_READS, *, where=_ffi.PAF_AUTO, format="paf",
                 read_on_gpu=False):
        """maps a FASTA / FASTQ file of reads (plain or gzip) to a PAF file, lines in input order -- minimap2's command line from a read set to
        its overlaps or alignments.  A reader thread cuts sub-batches of `sub_batch_reads` reads (and at most SUB_BATCH_BASES bases) with the
        library's streaming reader; up to min(n_threads, 8) workers per GPU (n_threads=None: enable_threading's value, or 1), each with a
        context of the pool, map and format them (mm355_map_batch_paf, GIL released); this thread writes the texts in input order.  At most
        2 x workers sub-batches exist at any time, as reads or as text: memory does not grow with the file.  No Python work per read or hit.
        The text is written to `out_path` + ".part" and renamed when it is complete: a failure stops the rest, removes the partly written
        file and is raised, and a file that was at `out_path` before is still there.  `where` (keyword-only): as for map_paf.
        Returns {n_reads, n_bases, n_lines, n_sub_batches, seconds} (and ms_format, n_on_device: the formatting step summed over the
        sub-batches, and how many of them the device formatted).
        format (keyword-only): "paf", or "sam": the header of sam_header(), then the lines of map_sam (mm355_map_batch_sam; the reader keeps
        FASTQ qualities, a FASTA read prints `*`; reads without hits write their unmapped record).  A SAM sub-batch's text is about 2.2 x its
        bases (a PAF one's a few hundred bytes per hit), and 2 x workers of them exist at a time.  Any other value: ValueError, before a
        file is opened.
        The reads file may also be a BAM (unaligned, as basecallers write it, or aligned): its records are the reads -- secondary and
        supplementary ones skipped, reverse-strand ones turned back, aux tags dropped (include/mm355.h).
        read_on_gpu (keyword-only): True opens the reads with mm355_fastx_open_device on the aligner's first device -- a BGZF file (bgzip
        FASTQ / FASTA, or a BAM) is inflated there, a workgroup per block, and only cut into records on the host.  Any other file (plain
        text, plain gzip) is opened as without the keyword.  The returned dict then has reader_on_device (bool): which of the two happened."""
        if format not in ("paf", "sam"):
            raise ValueError("`format` must be \"paf\" or \"sam\"")
        flags = self._sam_flags(cs, MD) if format == "sam" else self._paf_flags(cs, MD)
        return self._map_file(format, reads_path, out_path, flags, n_threads, sub_batch_reads, where, _FileOpts(read_on_gpu=bool(read_on_gpu)))

    def _open_reads(self, reads_path, sam, o):
        """the library's streaming reader on a reads file: (the handle; whether the device inflates the file; the @RG lines of a BAM whose
        tags are kept, else b"").  sam: the reader keeps qualities"""
        L = self._L
        fx = C.c_void_p()
        rc = _ffi.MM355_EINVAL
        if o.read_on_gpu:
            rc = L.mm355_fastx_open_device(os.fsencode(reads_path), 1 if sam else 0, self._devices[0], C.byref(fx))
        reader_on_device = rc == 0
        if rc == _ffi.MM355_EINVAL:               # not asked for, or not a BGZF file: the host reader
            rc = (L.mm355_fastx_open_qual if sam else L.mm355_fastx_open)(os.fsencode(reads_path), C.byref(fx))
        if rc == 0 and o.keep_aux is not None:    # the tags to keep
            rc = L.mm355_fastx_keep_aux(fx, o.keep_aux)
            if rc != 0:
                L.mm355_fastx_close(fx)
        if rc != 0:
            raise RuntimeError("%s: %s" % (reads_path, L.mm355_strerror(rc).decode()))
        n_rg = C.c_int64()
        rg = L.mm355_fastx_bam_rg(fx, C.byref(n_rg)) if o.keep_aux is not None else None
        return fx, reader_on_device, C.string_at(rg, n_rg.value) if rg else b""

    def _file_work(self, kind, flags, where, o):
        """what a worker of _map_file does with one sub-batch of reads, built once per file: work(ctx, reads) -> _SubBatch.  Inside it the
        library call is one callable, (ctx, reads) -> (rc, result, bytes of kept tags), on the entry point the file's keywords choose"""
        L, sam = self._L, kind != "paf"
        entry = (self._bam_entry(1 if o.compress else 0, o.keep_aux is not None, o.sort, o.index, o.tmp_compress) if kind == "bam" else
                 _Entry(L.mm355_map_batch_sam, True, False, (), _ffi.Text) if sam else _Entry(L.mm355_map_batch_paf, False, False, (), _ffi.Text))

        def call(ctx, rp):
            r = rp.contents
            aux, n_aux = (None, None, None), 0
            if o.keep_aux is not None:
                alen, amod = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
                ap = L.mm355_reads_aux(rp, C.byref(alen), C.byref(amod))
                if ap:
                    n_aux = int(np.ctypeslib.as_array(alen, shape=(int(r.n),)).sum(dtype=np.int64))
                aux = (ap, alen, amod)
            rc, tp = self._call_entry(entry, ctx, (int(r.n), r.seqs, r.lens, r.names), L.mm355_reads_quals(rp) if sam else None, aux, flags, o.sam_flags, where)
            return rc, tp, n_aux

        def work(ctx, rp):
            r = rp.contents
            n_bases = int(np.ctypeslib.as_array(r.lens, shape=(int(r.n),)).sum(dtype=np.int64))
            rc, tp, n_aux = call(ctx[1], rp)
            if rc != 0:
                raise RuntimeError(L.mm355_strerror(rc).decode())
            return _SubBatch(tp, int(r.n), n_bases, n_aux)
        return work, lambda d: (L.mm355_free_run if o.sort else L.mm355_free_text)(d.tp)

    def _merge_spool(self, sink, out, level, bai):
        """the merge phase on what the run sink holds (the workers' contexts are back in the pool: the merge takes one): (bytes written,
        seconds in the .bai builder)"""
        sink.tmp.flush()
        spool = np.memmap(sink.tmp, dtype=np.uint8, mode="r", shape=(sink.n_tmp,)) if sink.n_tmp else np.zeros(0, np.uint8)
        step = _PackedStep(self._L, level) if sink.packed else _GatherStep(self._L, level)
        return _merge(self._L, [sink.runs[k] for k in sorted(sink.runs)], spool, out, step, bai, (self._ctx_acquire, self._ctx_release))

    def _write_bai(self, bai, bai_part):
        """the finished index to bai_part: (its bytes, the seconds that took)"""
        t_ix = time.perf_counter()
        tp = C.POINTER(_ffi.Text)()
        _ffi.check(self._L.mm355_bai_finish(bai, C.byref(tp)))
        try:
            with open(bai_part, "wb") as f:
                f.write(_ffi.text_view(tp))
            return int(tp.contents.n_text), time.perf_counter() - t_ix
        finally:
            self._L.mm355_free_text(tp)

    def _map_file(self, kind, reads_path, out_path, flags, n_threads, sub_batch_reads, where, o=_FileOpts()):
        """map_file (kind "paf" / "sam") and map_bam_file ("bam", with its keywords in `o`).  The reader, the workers and the bound on
        memory are _pipeline.Pipeline's; here: the arguments, the reads file, the sink -- texts written in input order, or (sort) runs
        spooled to a temporary file as they complete and merged afterwards (_merge; index: it feeds the .bai builder; tmp_compress:
        packed runs, merged on the device) -- the ".part" files with their rename or removal, and the returned dict"""
        L = self._L
        nt = self._n_threads if n_threads is None else int(n_threads)
        n_workers = max(1, min(nt, 8)) * len(self._devices)
        sub_batch_reads = int(sub_batch_reads)
        if sub_batch_reads < 1:
            raise ValueError("`sub_batch_reads` must be at least 1")
        t0 = time.perf_counter()
        fx, reader_on_device, rg = self._open_reads(reads_path, kind != "paf", o)
        suffix = (lambda x: x.encode()) if isinstance(os.fspath(out_path), bytes) else (lambda x: x)
        part, bai_path = os.fspath(out_path) + suffix(".part"), os.fspath(out_path) + suffix(".bai")
        bai_part = bai_path + suffix(".part")
        tmp, bai = None, C.c_void_p()
        n_index, seconds_index, seconds_merge = 0, 0.0, 0.0
        try:
            header = self.sam_header() if kind == "sam" else self.bam_header(o.compress, rg, sort=o.sort) if kind == "bam" else b""
            trailer = BAM_EOF if kind == "bam" else b""

            def next_item():
                rp = C.POINTER(_ffi.Reads)()
                rc = L.mm355_fastx_next(fx, sub_batch_reads, SUB_BATCH_BASES, C.byref(rp))
                if rc != 0:
                    raise RuntimeError("%s: %s" % (reads_path, L.mm355_strerror(rc).decode()))
                return rp if rp else None
            work, free_result = self._file_work(kind, flags, int(where), o)
            out = open(part, "wb")          # (an unwritable path raises here: nothing has run, no file is left)
            try:
                self._names()
                if o.index:
                    _ffi.check(L.mm355_bai_open(len(self._names()), len(header), C.byref(bai)))
                out.write(header)
                if o.sort:                  # (unlinked as soon as it is open: no exit path leaves it behind)
                    tmp = tempfile.TemporaryFile(dir=os.fspath(o.tmp_dir) if o.tmp_dir is not None else os.path.dirname(os.path.abspath(os.fspath(out_path))))
                sink = _RunSpool(tmp, o.index, o.tmp_compress) if o.sort else _TextSink(out)
                n_reads = n_bases = n_aux = 0
                with _pipeline.Pipeline(next_item, work, L.mm355_reads_free, free_result, self._ctx_acquire, self._ctx_release, n_workers, ordered=not o.sort) as pipe:
                    for k, d in pipe:
                        sink.take(k, d.tp)
                        n_reads += d.n_reads; n_bases += d.n_bases; n_aux += d.n_aux
                n_out = len(header) + len(trailer)
                if o.sort:
                    t_merge = time.perf_counter()
                    n_merged, seconds_index = self._merge_spool(sink, out, 1 if o.compress else 0, bai if o.index else None)
                    n_out += n_merged
                    seconds_merge = time.perf_counter() - t_merge
                else:
                    n_out += sink.n_out
                out.write(trailer)
                out.close()
                if o.index:                 # the whole index exists as a file before either name changes
                    n_index, t_ix = self._write_bai(bai, bai_part)
                    seconds_index += t_ix
                os.replace(part, out_path)
                if o.index:
                    os.replace(bai_part, bai_path)
            except BaseException:
                out.close()
                for p in (part, bai_part) if o.index else (part,):
                    try:
                        os.remove(p)
                    except OSError:
                        pass
                raise
        finally:
            if tmp is not None:
                tmp.close()
            if bai:
                L.mm355_bai_close(bai)
            L.mm355_fastx_close(fx)
        res = {"n_reads": n_reads, "n_bases": n_bases, "n_lines": sink.n_lines, "n_sub_batches": pipe.n_items,
               "seconds": time.perf_counter() - t0, "ms_format": sink.ms_format, "n_on_device": sink.n_dev}
        if o.compress:
            res["n_bytes_out"] = n_out
        if o.read_on_gpu:
            res["reader_on_device"] = reader_on_device
        if o.keep_aux is not None:
            res["n_aux_bytes"] = n_aux
        if o.sort:
            res["n_runs"], res["seconds_merge"], res["n_tmp_bytes"] = len(sink.runs), seconds_merge, sink.n_tmp
        if o.index:
            res["n_index_bytes"], res["seconds_index"] = n_index, seconds_index
        if o.tmp_compress:
            res["n_tmp_raw_bytes"] = sink.n_raw
        return res

    def _stage_runner(self):
        """per-stage access to the same kernels (parity tests, kernel bench)"""
        return _ffi.StageRunner(self._idx, self._mo, self._device)

    def __del__(self):
        try:
            if self._ctx: self._L.mm355_ctx_destroy(self._ctx)
            for ctxs in self._wctx.values():
                for ctx in ctxs: self._L.mm355_ctx_destroy(ctx)
            if self._idx: self._L.mm355_index_free(self._idx)
        except Exception:
            pass
