"""The .bai index of a coordinate-sorted BAM file, stated independently of the library for the index's tests (tests/test_bai_host.py,
tests/test_gpu_bai.py) from the rule of include/mm355.h and SAM v1 sections 5.2 / 5.3: the span of a record from its bytes, the builder
from the bytes of a BAM file (blocks walked by BSIZE, inflated with zlib), a parser of .bai, and query(), which answers a region from the
index the way a reader does.  Shares no code with the library."""
import bisect
import struct
import zlib

REF_OPS = (0, 2, 3, 7, 8)        # M D N = X
PSEUDO = 37450
MAX_END = 1 << 29


def span_of(rec):
    """rec: a record with its block_size word -> end << 1 | unmapped bit"""
    pos, = struct.unpack_from("<i", rec, 8)
    l_name = rec[12]
    n_cigar, flag = struct.unpack_from("<HH", rec, 16)
    reflen = 0
    if not flag & 4:
        for w in struct.unpack_from("<%dI" % n_cigar, rec, 36 + l_name):
            if w & 15 in REF_OPS:
                reflen += w >> 4
    return (pos + max(1, reflen)) << 1 | (flag >> 2 & 1)


def fits(rec):
    return len(rec) >= 36 and 36 + rec[12] + 4 * struct.unpack_from("<H", rec, 16)[0] <= len(rec)


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def blocks_of(data):
    """the BGZF blocks of a file: (file offset, size, payload)"""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04"
        xlen, = struct.unpack_from("<H", data, at + 10)
        x, bsize = at + 12, None
        while x < at + 12 + xlen:
            si, slen = data[x:x + 2], struct.unpack_from("<H", data, x + 2)[0]
            if si == b"BC" and slen == 2:
                bsize, = struct.unpack_from("<H", data, x + 4)
            x += 4 + slen
        size = bsize + 1
        payload = zlib.decompress(data[at + 12 + xlen:at + size - 8], -15)
        crc, isize = struct.unpack_from("<II", data, at + size - 8)
        assert isize == len(payload) and crc == zlib.crc32(payload)
        out.append((at, size, payload))
        at += size
    assert at == len(data)
    return out


class Bam:
    """a BAM file's bytes, cut: the contigs, the records with their virtual offsets (vb, ve)"""

    def __init__(self, data):
        self.blocks = blocks_of(data)
        assert self.blocks and self.blocks[-1][2] == b""              # the EOF block
        self.stream = b"".join(b[2] for b in self.blocks)
        self.isum = [0]
        for b in self.blocks:
            self.isum.append(self.isum[-1] + len(b[2]))
        s = self.stream
        assert s[:4] == b"BAM\1"
        at = 8 + struct.unpack_from("<I", s, 4)[0]
        n_ref, = struct.unpack_from("<I", s, at)
        at += 4
        self.refs = []
        for _ in range(n_ref):
            l, = struct.unpack_from("<I", s, at)
            self.refs.append((s[at + 4:at + 4 + l - 1], struct.unpack_from("<I", s, at + 4 + l)[0]))
            at += 8 + l
        self.recs = []                                               # (ref, beg, end, unmapped, vb, ve, record)
        while at < len(s):
            n = struct.unpack_from("<I", s, at)[0] + 4
            rec = s[at:at + n]
            ref, pos = struct.unpack_from("<ii", rec, 4)
            sp = span_of(rec)
            self.recs.append((ref, pos, sp >> 1, sp & 1, self.voffset(at), self.voffset(at + n), rec))
            at += n
        assert at == len(s)
        self.vbs = [r[4] for r in self.recs]

    def voffset(self, u):
        """the first block with isum(b + 1) > u; for the stream's length: the block behind the last one that holds bytes (the EOF block)"""
        b = bisect.bisect_right(self.isum, u) - 1
        if b >= len(self.blocks):
            b = max(k for k, blk in enumerate(self.blocks) if blk[2]) + 1
        return self.blocks[b][0] << 16 | (u - self.isum[b])

    def decode(self, vb, ve):
        """the records from vb up to ve"""
        return self.recs[bisect.bisect_left(self.vbs, vb):bisect.bisect_left(self.vbs, ve)]


def build(bam, census=None):
    """the .bai of a Bam; census: a dict that receives what the finishing did"""
    cen = census if census is not None else {}
    for k in ("moved", "stayed5", "cascades", "chunk_merges", "chunk_kept_apart", "backfilled"):
        cen.setdefault(k, 0)
    out = [b"BAI\1", struct.pack("<I", len(bam.refs))]
    n_no_coor = sum(1 for r in bam.recs if r[0] < 0)
    last = None
    for r in bam.recs:
        key = ((r[0] & 0xffffffff), r[1])
        assert last is None or key >= last, "the file is not sorted"
        last = key
    for ref in range(len(bam.refs)):
        recs = [r for r in bam.recs if r[0] == ref]
        if not recs:
            out.append(struct.pack("<II", 0, 0))
            continue
        bins, iv, run = {}, {}, None
        for _, beg, end, unm, vb, ve, _rec in recs:
            assert 0 <= beg < end <= MAX_END
            b = reg2bin(beg, end)
            if run == b:
                bins[b][-1][1] = ve
            else:
                bins.setdefault(b, []).append([vb, ve])
                run = b
            for w in range(beg >> 14, ((end - 1) >> 14) + 1):
                iv.setdefault(w, vb)
        n_intv = max(iv) + 1
        lin = [None] * n_intv
        for w in range(n_intv - 1, -1, -1):
            if w in iv:
                lin[w] = iv[w]
            else:
                lin[w] = lin[w + 1]
                cen["backfilled"] += 1
        moved_from = set()
        for lo, hi in ((4681, 37449), (585, 4681), (73, 585), (9, 73), (1, 9)):
            for b in sorted(k for k in bins if lo <= k < hi):
                ch = bins[b]
                if (max(c[1] for c in ch) >> 16) - (min(c[0] for c in ch) >> 16) < 0x10000:
                    bins.setdefault((b - 1) >> 3, []).extend(bins.pop(b))
                    cen["moved"] += 1
                    if any((m - 1) >> 3 == b for m in moved_from):
                        cen["cascades"] += 1
                    moved_from.add(b)
                elif lo == 4681:
                    cen["stayed5"] += 1
        out.append(struct.pack("<I", len(bins) + 1))
        for b in sorted(bins):
            ch = sorted(bins[b])
            merged = [list(ch[0])]
            for c in ch[1:]:
                if c[0] >> 16 <= merged[-1][1] >> 16:
                    merged[-1][1] = max(merged[-1][1], c[1])
                    cen["chunk_merges"] += 1
                else:
                    merged.append(list(c))
                    cen["chunk_kept_apart"] += 1
            out.append(struct.pack("<II", b, len(merged)) + b"".join(struct.pack("<QQ", *c) for c in merged))
        out.append(struct.pack("<IIQQQQ", PSEUDO, 2, recs[0][4], recs[-1][5], sum(1 for r in recs if not r[3]), sum(1 for r in recs if r[3])))
        out.append(struct.pack("<I", n_intv) + struct.pack("<%dQ" % n_intv, *lin))
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def parse(bai):
    """-> ([per ref (bins: {bin: [(beg, end)]}, ioffset list)], n_no_coor); checks the bins' order"""
    assert bai[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<I", bai, 4)
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<I", bai, at)
        at += 4
        bins, order = {}, []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<II", bai, at)
            at += 8
            bins[b] = [struct.unpack_from("<QQ", bai, at + 16 * k) for k in range(n_chunk)]
            order.append(b)
            at += 16 * n_chunk
        assert order == sorted(order) and (not order or order[-1] == PSEUDO)
        n_intv, = struct.unpack_from("<I", bai, at)
        at += 4
        refs.append((bins, list(struct.unpack_from("<%dQ" % n_intv, bai, at))))
        at += 8 * n_intv
    n_no_coor, = struct.unpack_from("<Q", bai, at)
    assert at + 8 == len(bai)
    return refs, n_no_coor


def query(bam, bai, ref, b, e):
    """the records of [b, e) on ref, found through the index alone: reg2bins, the chunks whose end lies above the linear index's offset
    for b's window, decoded from vb to ve, filtered by overlap"""
    refs, _ = parse(bai) if isinstance(bai, (bytes, bytearray)) else bai
    bins, lin = refs[ref]
    if b >= e or not lin:
        return []
    min_off = lin[b >> 14] if (b >> 14) < len(lin) else lin[-1]
    hit = {}
    for k in reg2bins(b, e):
        for vb, ve in bins.get(k, ()):
            if ve > min_off:
                for r in bam.decode(vb, ve):
                    if r[0] == ref and r[1] < e and r[2] > b:
                        hit[r[4]] = r
    return [hit[k] for k in sorted(hit)]


def brute(bam, ref, b, e):
    return [r for r in bam.recs if r[0] == ref and r[1] < e and r[2] > b] if b < e else []
