"""What the inflate tests share (tests/test_inflate_host.py, tests/test_gpu_inflate.py): BGZF members from three producers -- Python's zlib at
every level and strategy, this library's own host coder, and a small bit writer for members neither of them emits (and one member per reason
the decoder of mappy-rs_amd/csrc/mm355_inflate.h refuses) -- with Python's verdict on each, a FASTQ / unaligned-BAM pair of files, and the
mutations of the CPU run.  A member is (name, bytes of the whole member, payload or None when it must be refused)."""
import random
import struct
import zlib

import numpy as np

import _deflate as D

P = D.P
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_CACHE = {}


def member(cdata, payload, *, crc=None, isize=None, extra=b"", mtime=0, xfl=0, os_=255):
    """a BGZF member around `cdata`: `extra` is subfields in front of BC; crc / isize override the trailer"""
    xlen = len(extra) + 6
    total = 12 + xlen + len(cdata) + 8
    assert total <= 65536, total
    head = b"\x1f\x8b\x08\x04" + struct.pack("<IBBH", mtime, xfl, os_, xlen) + extra + b"BC\x02\x00" + struct.pack("<H", total - 1)
    return head + cdata + struct.pack("<II", zlib.crc32(payload) if crc is None else crc, len(payload) if isize is None else isize)


def parts(m):
    """(cdata, crc, isize) of a member, by its own XLEN"""
    xlen = struct.unpack_from("<H", m, 10)[0]
    return m[12 + xlen:-8], struct.unpack_from("<I", m, len(m) - 8)[0], struct.unpack_from("<I", m, len(m) - 4)[0]


def verdict(cdata, crc, isize):
    """Python's: the payload when zlib's raw inflate reaches the end of the stream and CRC-32 and length are the trailer's, else None"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(cdata)
    except zlib.error:
        return None
    if not d.eof or len(out) != isize or zlib.crc32(out) != crc:
        return None
    return out


def raw(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, sync_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if sync_at is None:
        return c.compress(payload) + c.flush()
    return c.compress(payload[:sync_at]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(payload[sync_at:]) + c.flush()


CODINGS = [("l0", 0, zlib.Z_DEFAULT_STRATEGY), ("l1", 1, zlib.Z_DEFAULT_STRATEGY), ("l6", 6, zlib.Z_DEFAULT_STRATEGY), ("l9", 9, zlib.Z_DEFAULT_STRATEGY),
           ("fixed", 6, zlib.Z_FIXED), ("huffman", 6, zlib.Z_HUFFMAN_ONLY), ("rle", 6, zlib.Z_RLE)]


def chunks():
    """name -> payload of at most 0xff00 bytes (the payloads of _deflate.payloads() cut there), one of 65536 bytes and the empty one"""
    out = {}
    for name, data in D.payloads().items():
        for k in range(max(1, (len(data) + P - 1) // P)):
            out["%s/%d" % (name, k)] = data[k * P:(k + 1) * P]
    rng = np.random.default_rng(31)
    q = b"".join(b"@r%d\nACGT%s\n+\n%s\n" % (i, rng.choice(list(b"ACGT"), 60).astype(np.uint8).tobytes(), bytes(rng.integers(35, 75, 64, dtype=np.uint8))) for i in range(700))
    out["isize_65536"] = q[:65536]
    assert len(out["isize_65536"]) == 65536
    out["empty"] = b""
    return out


def zlib_members():
    """every chunk at every coding that fits a member (BSIZE is 16 bits: random bytes of a full payload do not fit as a fixed-Huffman block)"""
    if "zlib" not in _CACHE:
        out = []
        for name, p in chunks().items():
            for cn, level, strat in CODINGS:
                c = raw(p, level, strat)
                if len(c) + 26 <= 65536:
                    out.append(("zlib/%s/%s" % (cn, name), member(c, p), p))
            if len(p) > 2:
                out.append(("zlib/sync/%s" % name, member(raw(p, 6, sync_at=len(p) // 2), p), p))
        _CACHE["zlib"] = out
    return _CACHE["zlib"]


def own_members():
    """the library's host coder (single-code distance sets, distance 32768, headers without run symbols); needs the built library"""
    if "own" not in _CACHE:
        import mappy_rs
        out = []
        for name, data in D.payloads().items():
            for k, b in enumerate(D.blocks(mappy_rs.bgzf_wrap(data, compress=True))):
                out.append(("own/%s/%d" % (name, k), b, data[k * P:(k + 1) * P]))
        _CACHE["own"] = out
    return _CACHE["own"]


# ---- the bit writer
class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, k):                  # k bits of v, lowest first
        assert 0 <= v < 1 << k
        self.acc |= v << self.n
        self.n += k
        return self

    def code(self, c):                    # a Huffman code (value, length): its first bit first
        v, k = c
        return self.put(int(format(v, "0%db" % k)[::-1], 2) if k else 0, k)

    def align(self):
        self.n = (self.n + 7) // 8 * 8
        return self

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def canonical(lens):
    """symbol -> (code, length) of the canonical code of RFC 1951 3.2.2 (over-subscribed sets too: the codes just wrap)"""
    out, code = {}, 0
    for k in range(1, 16):
        for s, l in enumerate(lens):
            if l == k:
                out[s] = (code & ((1 << k) - 1), k)
                code += 1
        code <<= 1
    return out


FIXED_LL = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_D = canonical([5] * 32)
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_PLAIN = [4] * 16 + [0, 0, 0]          # the lengths 0 .. 15 in four bits each: a complete code without run symbols
CL_RUNS = [5] * 16 + [2, 3, 3]           # with 16, 17 and 18


def dyn_head(b, ll, d, *, final=1, cl=None, items=None, n_ll=None, n_d=None):
    """BFINAL, BTYPE 10 and the header of a dynamic block: ll / d are the code lengths; items: the code-length symbols to send, as
    (symbol,) or (symbol, extra value) -- default every length by itself"""
    cl = CL_PLAIN if cl is None else cl
    items = [(x,) for x in list(ll) + list(d)] if items is None else items
    n_ll, n_d = len(ll) if n_ll is None else n_ll, len(d) if n_d is None else n_d
    n_cl = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl[s]))
    b.put(final, 1).put(2, 2).put(n_ll - 257, 5).put(n_d - 1, 5).put(n_cl - 4, 4)
    for s in CL_ORDER[:n_cl]:
        b.put(cl[s], 3)
    cc = canonical(cl)
    for it in items:
        b.code(cc[it[0]])
        if it[0] >= 16:
            b.put(it[1], {16: 2, 17: 3, 18: 7}[it[0]])
    return canonical(ll), canonical(d)


def _ll_for(symbols, extra=()):
    """complete literal/length lengths in which `symbols` (and 256) have a code: 8 bits each, padded to 256 codes with unused literals"""
    ll = [0] * 286
    for s in list(symbols) + [256] + list(extra):
        ll[s] = 8
    for s in range(255, -1, -1):
        if sum(1 for x in ll if x) >= 256:
            break
        if not ll[s]:
            ll[s] = 8
    assert sum(1 for x in ll if x) == 256
    return ll


def built_members():
    """hand-assembled valid members neither producer emits"""
    out = []
    text = b"no match in here, only literals!"
    # literals only; HDIST = 1 and its one length 0
    b = Bits()
    ll, _ = dyn_head(b, _ll_for(text), [0])
    for c in text:
        b.code(ll[c])
    b.code(ll[256])
    out.append(("built/literals_hdist1_len0", member(b.bytes(), text), text))
    # a match whose distance equals its position: it reaches byte 0; then one of distance 1 and length 258 that overlaps itself
    b = Bits().put(1, 1).put(1, 2)
    for c in b"abcde":
        b.code(FIXED_LL[c])
    b.code(FIXED_LL[259]).code(FIXED_D[4]).put(0, 1)           # length 5, distance 5
    b.code(FIXED_LL[285]).code(FIXED_D[0])                     # length 258, distance 1
    b.code(FIXED_LL[256])
    p = b"abcdeabcde" + b"e" * 258
    out.append(("built/distance_is_position", member(b.bytes(), p), p))
    # the same, BC behind another subfield, and a header with MTIME, XFL and OS set
    out.append(("built/bc_behind_subfield", member(b.bytes(), p, extra=b"XY\x03\x00abc", mtime=0x12345678, xfl=2, os_=3), p))
    # run symbols 16, 17 and 18, one run across the literal/distance boundary
    ll_lens = [0] * 65 + [1] + [0] * 190 + [2] + [0] * 7 + [2]  # 'A': 1 bit, 256 and 264: 2 bits (HLIT = 265)
    items = [(18, 65 - 11), (1,), (18, 138 - 11), (18, 52 - 11), (2,), (17, 7 - 3), (2,), (16, 0)]   # ... 264: 2, then "repeat 2 three times": d 0, 1, 2
    d_lens = [2, 2, 2, 2]
    items.append((2,))
    b = Bits()
    ll, d = dyn_head(b, ll_lens, d_lens, cl=CL_RUNS, items=items)
    b.code(ll[65]).code(ll[65]).code(ll[264]).put(0, 0).code(d[1]).code(ll[256])      # A A, length 10 distance 2
    p = b"A" * 12
    out.append(("built/runs_across_the_boundary", member(b.bytes(), p), p))
    # a code of 15 bits: lengths 1, 2, ..., 14, 15, 15
    ll_lens = [0] * 286
    for k, s in enumerate([256] + list(range(97, 111))):
        ll_lens[s] = k + 1
    ll_lens[111] = 15
    b = Bits()
    ll, _ = dyn_head(b, ll_lens, [0])
    p = bytes(range(97, 112)) * 3
    for c in p:
        b.code(ll[c])
    b.code(ll[256])
    out.append(("built/codes_of_15_bits", member(b.bytes(), p), p))
    # two stored blocks, the first empty (a sync flush), and bytes between the stream's end and the trailer
    b = Bits().put(0, 1).put(0, 2).align().put(0, 16).put(0xffff, 16).put(1, 1).put(0, 2).align().put(3, 16).put(0xfffc, 16)
    out.append(("built/stored_and_ignored_tail", member(b.bytes() + b"xyz" + b"\xde\xad", b"xyz"), b"xyz"))
    for name, m, p in out:
        assert verdict(*parts(m)) == p, name
    return out


def refusals():
    """one member per reason to refuse; Python's zlib refuses every one (asserted here)"""
    out = []

    def add(name, cdata, payload=b"", **kw):
        out.append(("refuse/" + name, member(cdata, payload, **kw), None))

    lit = lambda b, s: [b.code(FIXED_LL[c]) for c in s]
    add("btype_11", Bits().put(1, 1).put(3, 2).bytes())
    add("stored_len_nlen", Bits().put(1, 1).put(0, 2).align().put(3, 16).put(0xfffd, 16).bytes() + b"xyz", b"xyz")
    ok_ll = _ll_for(b"ab")
    over = list(ok_ll)
    over[0] = 7
    for name, ll_, d_, cl_ in (("oversubscribed_literal", over, [0], None), ("oversubscribed_distance", ok_ll, [1, 1, 1], None),
                               ("oversubscribed_code_length", ok_ll, [0], [3] * 9 + [4] * 7 + [0, 0, 0]),
                               ("incomplete_literal", [x if s != 1 else 0 for s, x in enumerate(ok_ll)], [0], None),
                               ("incomplete_distance", ok_ll, [2, 2], None), ("incomplete_single_code_of_two_bits", ok_ll, [2], None),
                               ("incomplete_code_length", ok_ll, [0], [4] * 15 + [0, 0, 0, 0])):
        b = Bits()
        try:
            ll, _ = dyn_head(b, ll_, d_, cl=cl_)
        except KeyError:                                   # (a length whose code-length symbol has no code: send what there is)
            raise
        b.code(ll[97]).code(ll[256])
        add(name, b.bytes(), b"a")
    no_eob = _ll_for(b"ab")
    no_eob[256], no_eob[0] = 0, 8
    b = Bits()
    ll, _ = dyn_head(b, no_eob, [0])
    b.code(ll[97])
    add("no_end_of_block_code", b.bytes() + b"\0\0", b"a")
    b = Bits()
    dyn_head(b, [8] * 257, [0], cl=CL_RUNS, items=[(16, 0)] + [(8,)] * 257)
    add("repeat_without_previous", b.bytes() + b"\0\0")
    b = Bits()
    dyn_head(b, [8] * 257, [0], cl=CL_RUNS, items=[(8,)] * 256 + [(18, 127)])
    add("run_past_hlit_hdist", b.bytes() + b"\0\0")
    for s in (286, 287):
        b = Bits().put(1, 1).put(1, 2)
        lit(b, b"abc")
        b.code(FIXED_LL[s]).code(FIXED_D[0]).code(FIXED_LL[256])
        add("length_symbol_%d" % s, b.bytes(), b"abc")
    for s in (30, 31):
        b = Bits().put(1, 1).put(1, 2)
        lit(b, b"abc")
        b.code(FIXED_LL[257]).code(FIXED_D[s]).code(FIXED_LL[256])
        add("distance_symbol_%d" % s, b.bytes(), b"abcabc")
    b = Bits().put(1, 1).put(1, 2)
    lit(b, b"abc")
    b.code(FIXED_LL[257]).code(FIXED_D[3]).code(FIXED_LL[256])      # distance 4 at position 3
    add("distance_before_the_first_byte", b.bytes(), b"abcabc")
    b = Bits().put(1, 1).put(1, 2)
    b.code(FIXED_LL[257]).code(FIXED_D[0]).code(FIXED_LL[256])      # a match at position 0
    add("match_at_position_0", b.bytes(), b"aaa")
    good = raw(b"hello, hello, hello, hello")
    add("output_passes_isize", good, b"hello, hello, hello, hello", isize=20)
    add("output_short_of_isize", good, b"hello, hello, hello, hello", isize=27)
    add("crc_mismatch", good, b"hello, hello, hello, hello", crc=zlib.crc32(b"hello") ^ 1)
    b = Bits().put(1, 1).put(1, 2)
    b.code(FIXED_LL[285]).code(FIXED_D[0])
    add("match_passes_isize", Bits().put(1, 1).put(1, 2).code(FIXED_LL[97]).code(FIXED_LL[285]).code(FIXED_D[0]).code(FIXED_LL[256]).bytes(), b"a" * 100)
    big = raw(D.payloads()["text_%d" % P], 6)
    add("input_ends_in_a_symbol", big[:len(big) // 2], D.payloads()["text_%d" % P])
    add("input_ends_before_the_last_block", raw(b"abcabcabc", 6, sync_at=4)[:-2], b"abcabcabc")
    add("no_input", b"")
    add("stored_runs_out", Bits().put(1, 1).put(0, 2).align().put(9, 16).put(0xfff6, 16).bytes() + b"xyz", b"xyz" * 3)
    add("hlit_above_286", Bits().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(15, 4).bytes() + b"\0" * 40)
    for name, m, _ in out:
        assert verdict(*parts(m)) is None, name
    return out


def mixed_stream(members_):
    """members of every producer one behind the other, the EOF block in the middle and at the end: (the stream, its payload)"""
    ms = list(members_)
    half = len(ms) // 2
    seq = ms[:half] + [("eof", EOF, b"")] + ms[half:] + [("eof", EOF, b"")]
    return b"".join(m for _, m, _ in seq), b"".join(p for _, _, p in seq)


def mutations(n, seed=7):
    """n single-bit flips and truncations of valid members' cdata (small members of every producer, so that header bits are hit often):
    ((cdata, crc, isize), the unmutated payload) each; trailers stay, so a verdict of 'accept' means the flipped bit was one nobody reads"""
    rng = random.Random(seed)
    base = [(m, p) for name, m, p in zlib_members() + own_members() + built_members() if p is not None and 0 < len(p) <= 600 and len(m) < 700]
    assert len(base) > 60
    out = []
    while len(out) < n:
        m, p = rng.choice(base)
        c, crc, isize = parts(m)
        if rng.random() < 0.15:
            out.append(((c[:rng.randrange(len(c))], crc, isize), p))
        else:
            k = rng.randrange(8 * len(c))
            out.append(((c[:k >> 3] + bytes([c[k >> 3] ^ 1 << (k & 7)]) + c[(k >> 3) + 1:], crc, isize), p))
    return out


# ---- reads files
def fastq_records(n=40, seed=3, with_n=True):
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        l = int(rng.integers(1, 700)) if i else 1
        seq = rng.choice(list(b"ACGT" + (b"N" if with_n else b"")), l).astype(np.uint8).tobytes()
        qual = bytes(rng.integers(33, 74, l, dtype=np.uint8))
        recs.append((b"read%d/x" % i, seq, qual))
    return recs


def fastq_text(recs):
    return b"".join(b"@%s some comment\n%s\n+\n%s\n" % r for r in recs)


_NIB = {c: i for i, c in enumerate(b"=ACMGRSVTWYHKDBN")}
_COMP = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")


def bam_record(name, seq, qual, flag=4, n_cigar=0, aux=b"", l_name=None, block_size=None, l_seq=None):
    """one BAM record (block_size included); qual None: 0xff bytes; flag 0x10: seq / qual are stored reverse-complemented as an aligner would"""
    if flag & 0x10:
        seq, qual = seq.translate(_COMP)[::-1], None if qual is None else qual[::-1]
    nm = name + b"\0"
    packed = bytes((_NIB[seq[i]] << 4) | (_NIB[seq[i + 1]] if i + 1 < len(seq) else 0) for i in range(0, len(seq), 2))
    q = b"\xff" * len(seq) if qual is None else bytes(c - 33 for c in qual)
    body = struct.pack("<iiBBHHHIiii", -1, -1, len(nm) if l_name is None else l_name, 0, 4680, n_cigar, flag, len(seq) if l_seq is None else l_seq, -1, -1, 0)
    body += nm + struct.pack("<%dI" % n_cigar, *[(10 << 4) | 4] * n_cigar) + packed + q + aux
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def bam_header(text=b"@HD\tVN:1.6\tSO:unsorted\n", refs=()):
    out = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs))
    for nm, ln in refs:
        out += struct.pack("<I", len(nm) + 1) + nm + b"\0" + struct.pack("<I", ln)
    return out


def ubam_bytes(recs):
    """the uninflated bytes of an unaligned BAM of the records, with aux tags that the reader drops"""
    return bam_header() + b"".join(bam_record(n, s, q, aux=b"RGZgroup\0MMZC+m,5;\0") for n, s, q in recs)


def bgzf_file(data, cut, level=6):
    """`data` in members of `cut` payload bytes (lines and records straddle them) and the EOF block"""
    return b"".join(member(raw(data[i:i + cut], level), data[i:i + cut]) for i in range(0, len(data), cut)) + EOF


def corrupt(bgzf, k):
    """the stream with one bit of member k's CRC-32 flipped (any other bit might be one nobody reads)"""
    at = 0
    for _ in range(k):
        at += struct.unpack_from("<H", bgzf, at + 16)[0] + 1
    at += struct.unpack_from("<H", bgzf, at + 16)[0] + 1 - 7
    return bgzf[:at] + bytes([bgzf[at] ^ 0x10]) + bgzf[at + 1:]
