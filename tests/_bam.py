"""The BAM record and its BGZF framing, stated independently of the library for the BAM writer's tests (tests/test_bam_host.py,
tests/test_gpu_bam.py): record_of encodes one SAM line by the rules of include/mm355.h (the SAM/BAM specification, htslib's choices where it
leaves one), frame builds stored BGZF blocks with zlib.crc32, split inflates a BGZF stream with gzip and cuts it into records."""
import gzip
import re
import struct
import zlib

PAYLOAD = 0xff00
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_CODE = bytearray([15]) * 256
for _i, _c in enumerate("=ACMGRSVTWYHKDBN"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i
_CODE = bytes(_CODE)
_OPS = b"MIDNSHP=X"
_CIGAR = re.compile(rb"(\d+)([MIDNSHP=X])")


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def _int_tag(v):
    if v >= 0:
        return b"C" + struct.pack("<B", v) if v <= 255 else b"S" + struct.pack("<H", v) if v <= 65535 else b"I" + struct.pack("<I", v)
    return b"c" + struct.pack("<b", v) if v >= -128 else b"s" + struct.pack("<h", v) if v >= -32768 else b"i" + struct.pack("<i", v)


def record_of(line, contigs):
    """the BAM record (block_size included) of one SAM line (str or bytes, no newline); contigs: the reference names in index order"""
    if isinstance(line, str):
        line = line.encode("latin-1")
    f = line.split(b"\t")
    qname, flag, rname, pos, mapq, cigar, seq, qual = f[0], int(f[1]), f[2], int(f[3]) - 1, int(f[4]), f[5], f[9], f[10]
    assert f[6:9] == [b"*", b"0", b"0"] and len(qname) <= 254 and 0 <= mapq <= 255
    refid = -1 if rname == b"*" else [c.encode() for c in contigs].index(rname)
    words = [] if cigar == b"*" else [int(n) << 4 | _OPS.index(op) for n, op in _CIGAR.findall(cigar)]
    assert cigar == b"*" or b"".join(b"%d%c" % (w >> 4, _OPS[w & 15]) for w in words) == cigar
    reflen = sum(w >> 4 for w in words if w & 15 in (0, 2, 3, 7, 8))
    l_seq = 0 if seq == b"*" else len(seq)
    packed = seq.translate(_CODE) + b"\0" if l_seq else b""
    packed = bytes(a << 4 | b for a, b in zip(packed[0:l_seq:2], packed[1:l_seq + 1:2]))
    quality = b"\xff" * l_seq if qual == b"*" else bytes((q - 33) & 0xff for q in qual)
    assert len(quality) == l_seq
    tags = []
    for t in f[11:]:
        name, typ, val = t[:2], t[3:4], t[5:]
        assert t[2:3] == t[4:5] == b":"
        if typ == b"i":
            tags.append(name + _int_tag(int(val)))
        elif typ == b"A":
            tags.append(name + b"A" + val)
        elif typ == b"f":
            tags.append(name + b"f" + struct.pack("<f", float(val)))
        else:
            assert typ == b"Z"
            tags.append(name + b"Z" + val + b"\0")
    cigar_words = words
    if len(words) > 65535:                                  # htslib's long-CIGAR form
        cigar_words = [(l_seq << 4 | 4) & 0xffffffff, (reflen << 4 | 3) & 0xffffffff]
        tags.append(b"CGBI" + struct.pack("<I", len(words)) + struct.pack("<%dI" % len(words), *words))
    body = struct.pack("<iiBBHHHIiii", refid, pos, len(qname) + 1, mapq, reg2bin(pos, pos + max(1, reflen)) & 0xffff, len(cigar_words), flag, l_seq, -1, -1, 0)
    body += qname + b"\0" + struct.pack("<%dI" % len(cigar_words), *cigar_words) + packed + quality + b"".join(tags)
    return struct.pack("<I", len(body)) + body


def frame(data):
    """`data` in stored BGZF blocks of at most PAYLOAD bytes each"""
    out = []
    for at in range(0, len(data), PAYLOAD):
        p = data[at:at + PAYLOAD]
        out.append(bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", len(p) + 30) + b"\x01" + struct.pack("<HH", len(p), len(p) ^ 0xffff)
                   + p + struct.pack("<II", zlib.crc32(p), len(p)))
    return b"".join(out)


def inflate(bgzf):
    """the payload of a BGZF stream, and a check that it is cut the way frame cuts it"""
    data = gzip.decompress(bgzf) if bgzf else b""
    assert len(bgzf) == len(data) + 31 * ((len(data) + PAYLOAD - 1) // PAYLOAD)
    return data


def cut(stream):
    """a stream of records -> the records, block_size included"""
    out, at = [], 0
    while at < len(stream):
        n = struct.unpack_from("<I", stream, at)[0] + 4
        out.append(stream[at:at + n])
        at += n
    assert at == len(stream)
    return out


def split(bgzf):
    return cut(inflate(bgzf))
