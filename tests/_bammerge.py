"""One step of the merge of compressed runs (include/mm355.h: mm355_bam_merge_step), stated independently of the library for its tests
(tests/test_bammerge_host.py, tests/test_gpu_bammerge.py): the members are inflated with Python's zlib, the records sliced out of the payloads
and concatenated behind the carry, and the result cut at 0xff00.  The spools the tests merge from are built here as well, with zlib -- a
member's producer is none of the step's business, only that member b of a run holds the raw bytes [b * 0xff00, (b + 1) * 0xff00)."""
import struct
import zlib

import numpy as np

P = 0xff00
EINVAL, EIO = -2, -4


def member(payload, level):
    """one BGZF member around `payload`; level 0: a stored deflate block (what the library writes where deflate would not shorten)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    cdata = c.compress(payload) + c.flush()
    total = 18 + len(cdata) + 8
    assert total <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", total - 1) + cdata + struct.pack("<II", zlib.crc32(payload), len(payload)))


def pack_run(raw, levels=(6,)):
    """(the members of `raw` cut every 0xff00 bytes, their n + 1 offsets); member b is written at levels[b % len(levels)]"""
    ms = [member(raw[at:at + P], levels[(at // P) % len(levels)]) for at in range(0, len(raw), P)]
    return b"".join(ms), np.cumsum([0] + [len(m) for m in ms], dtype=np.int64)


def members(blob):
    """the payloads of the BGZF members of `blob`, each inflated by zlib and held to its CRC-32 and ISIZE"""
    out, at = [], 0
    while at < len(blob):
        assert blob[at:at + 4] == b"\x1f\x8b\x08\x04" and blob[at + 12:at + 16] == b"BC\x02\x00", at
        size = struct.unpack_from("<H", blob, at + 16)[0] + 1
        p = zlib.decompress(blob[at + 18:at + size - 8], -15)
        crc, isize = struct.unpack_from("<II", blob, at + size - 8)
        assert zlib.crc32(p) == crc and len(p) == isize
        out.append(p)
        at += size
    assert at == len(blob)
    return out


class Step:
    """the arguments of one step; spool: bytes; slices: (at, bytes, raw_at) each; recs: (slice, at, len) each"""
    def __init__(self, spool, slices, recs, carry=b"", final=False, level=0):
        self.spool, self.slices, self.recs, self.carry, self.final, self.level = spool, list(slices), list(recs), carry, final, level

    def arrays(self):
        s = np.array(self.slices, np.int64).reshape(-1, 3)
        r = np.array(self.recs, np.int64).reshape(-1, 3)
        return (np.ascontiguousarray(s[:, 0]), np.ascontiguousarray(s[:, 1]), np.ascontiguousarray(s[:, 2]),
                np.ascontiguousarray(r[:, 0].astype(np.int32)), np.ascontiguousarray(r[:, 1]), np.ascontiguousarray(r[:, 2]))


def model(step):
    """(the raw bytes the step's blocks hold, the bytes it leaves over)"""
    payloads = [b"".join(members(step.spool[at:at + n])) for at, n, _ in step.slices]
    stream = step.carry + b"".join(payloads[s][at - step.slices[s][2]:at - step.slices[s][2] + n] for s, at, n in step.recs)
    assert len(stream) == len(step.carry) + sum(n for _, _, n in step.recs)
    n_now = len(stream) if step.final else len(stream) // P * P
    return stream[:n_now], stream[n_now:]


def slices_for(run_blk_off, place, lo, hi):
    """the slice of a run (its members' offsets, its place in the spool) that holds the raw range [lo, hi): (at, bytes, raw_at)"""
    m_lo, m_hi = lo // P, -(-hi // P)
    return (place + int(run_blk_off[m_lo]), int(run_blk_off[m_hi] - run_blk_off[m_lo]), m_lo * P)


# ---------------------------------------------------------------- spools and steps for the tests
BIG = (37, 4095, 4096, 4097, 8193, 70000)       # the smallest record; around the gather kernel's tile, two tiles and a byte; one that straddles three members
CARRIES = (0, 1, 15, 16, 0xfeff)


def _bytes(rng, n, kind):
    """n bytes: 0 compressible (a few symbols, repeats), 1 random (deflate does not shorten them: stored members)"""
    if kind:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return (rng.integers(0, 4, n, dtype=np.uint8) + 65).tobytes()


class Run:
    """a run of `sizes`-byte records: raw stream, record offsets, members, their offsets; place: where the members lie in the spool"""
    def __init__(self, rng, sizes, levels=(6,), kinds=(0,)):
        self.recs = [_bytes(rng, n, kinds[i % len(kinds)]) for i, n in enumerate(sizes)]
        self.raw = b"".join(self.recs)
        self.off = np.cumsum([0] + list(sizes), dtype=np.int64)
        self.blob, self.blk = pack_run(self.raw, levels)
        self.place = 0


def spool_of(runs, pad=b""):
    """the runs' members one behind the other (pad in front: a spool need not begin with the step's slices); sets every run's place"""
    at, parts = len(pad), [pad]
    for r in runs:
        r.place = at
        parts.append(r.blob)
        at += len(r.blob)
    return b"".join(parts)


def step_of(runs, spool, takes, order=None, **kw):
    """takes: (run, first record, one past the last) per slice, in slice order; a slice of a run that gives no record (first == last) holds the
    member of that record's first byte.  order: the merged order as (slice, k-th record of the slice) pairs; default slice after slice"""
    slices, per = [], []
    for r, lo, hi in takes:
        run = runs[r]
        a, b = int(run.off[lo]), int(run.off[hi]) if hi > lo else int(run.off[lo]) + 1
        slices.append(slices_for(run.blk, run.place, a, b))
        per.append([(int(run.off[k]), int(run.off[k + 1] - run.off[k])) for k in range(lo, hi)])
    if order is None:
        order = [(s, k) for s in range(len(takes)) for k in range(len(per[s]))]
    return Step(spool, slices, [(s,) + per[s][k] for s, k in order], **kw)


def want_of(runs, takes, order=None):
    """the records a step_of step gathers, from the runs' own bytes (no inflate: a check of the model itself)"""
    per = [[runs[r].recs[k] for k in range(lo, hi)] for r, lo, hi in takes]
    if order is None:
        order = [(s, k) for s in range(len(takes)) for k in range(len(per[s]))]
    return b"".join(per[s][k] for s, k in order)


def steps(seed=97):
    """label -> Step: the streams that reach every way the gather can go wrong (tests/test_gpu_bammerge.py lists them)"""
    rng = np.random.default_rng(seed)
    out = {}
    # one slice whose first record starts mid-member at every residue, behind every carry; the large sizes; stored members beside deflated ones
    for res in range(16):
        run = Run(rng, (48 + res,) + BIG + (50,), levels=(6, 0), kinds=(0, 1))
        spool = spool_of([run], pad=b"x" * (res * 7))
        for k, n_carry in enumerate(CARRIES):
            out["residue-%d-carry-%d" % (res, n_carry)] = step_of([run], spool, [(0, 1, len(run.recs))], carry=_bytes(rng, n_carry, 0), final=bool((res + k) & 1), level=(res + k) >> 1 & 1)
    # two runs interleaved record by record, a third slice that gives no record
    a, b, c = Run(rng, BIG[::-1] + (37, 38, 39), kinds=(1, 0)), Run(rng, (100, 200, 5000, 37, 66000, 41), levels=(0, 6)), Run(rng, (300, 400))
    spool = spool_of([a, b, c])
    order = [(s, k) for k in range(9) for s in (0, 1) if k < (9 if s == 0 else 5)]
    for level in (0, 1):
        out["two-interleaved-level-%d" % level] = step_of([a, b, c], spool, [(0, 0, 9), (1, 1, 6), (2, 1, 1)], order, carry=b"c" * 15, final=True, level=level)
        out["two-slices-level-%d" % level] = step_of([a, b, c], spool, [(0, 0, 9), (1, 1, 6)], order, carry=b"d" * 16, final=bool(level), level=level)
    # the middle members of a long run: the slice begins at member 1
    long_run = Run(rng, (700,) * 400, levels=(6, 0, 6))
    out["middle-members"] = step_of([long_run], spool_of([long_run]), [(0, 100, 290)], carry=b"", final=False, level=1)
    # 257 slices of small runs, a record or two from each, interleaved
    many = [Run(rng, (37 + k % 50, 300, 45 + k % 7), kinds=(k & 1,)) for k in range(257)]
    spool = spool_of(many)
    takes = [(k, k % 2, 2 + k % 2) for k in range(257)]
    order = [(s, 0) for s in range(257)] + [(s, 1) for s in range(256, -1, -1)]
    for level in (0, 1):
        out["257-slices-level-%d" % level] = step_of(many, spool, takes, order, carry=b"k" * 16, final=bool(level), level=level)
    # a step smaller than one payload: no block, all carry; and the same records as a final step: one short block
    small = Run(rng, (37, 500, 41))
    for final in (False, True):
        out["small-final-%d" % final] = step_of([small], spool_of([small]), [(0, 0, 3)], carry=b"s" * 1000, final=final, level=1)
    out["nothing-final"] = Step(b"", [], [], carry=b"", final=True, level=1)
    out["carry-only-final"] = Step(b"", [], [], carry=b"q" * 77, final=True, level=0)
    return out


def refusals(seed=101):
    """label -> (Step, the return code): every refusal of include/mm355.h, and a good step"""
    rng = np.random.default_rng(seed)
    run = Run(rng, (100, 37, 5000, 70000, 64), levels=(6, 0))
    spool = spool_of([run], pad=b"pad")
    good = step_of([run], spool, [(0, 1, 5)], carry=b"abc", final=True, level=1)

    def but(code, **kw):
        s = Step(good.spool, good.slices, good.recs, good.carry, good.final, good.level)
        for k, v in kw.items():
            setattr(s, k, v)
        return s, code
    (s_at, s_n, s_raw), n_rec = good.slices[0], len(good.recs)
    crc_at = run.place + int(run.blk[1]) - 7
    return {
        "good": but(0),
        "a slice passes base_len": but(EINVAL, slices=[(s_at, len(spool) - s_at + 1, s_raw)]),
        "a slice begins behind base_len": but(EINVAL, slices=[(len(spool) + 1, 0, s_raw)]),
        "negative slice_at": but(EINVAL, slices=[(-1, s_n, s_raw)]),
        "negative slice_bytes": but(EINVAL, slices=[(s_at, -1, s_raw)]),
        "negative slice_raw_at": but(EINVAL, slices=[(s_at, s_n, -1)]),
        "negative rec_len": but(EINVAL, recs=good.recs[:1] + [(0, good.recs[1][1], -1)] + good.recs[2:]),
        "negative rec_at": but(EINVAL, recs=[(0, -5, 37)] + good.recs[1:]),
        "a record passes its slice's payloads": but(EINVAL, recs=good.recs[:-1] + [(0, good.recs[-1][1], good.recs[-1][2] + 1)]),
        "a record before its slice's first payload byte": but(EINVAL, slices=[(s_at, s_n, s_raw + P)]),
        "rec_slice == n_slice": but(EINVAL, recs=[(1,) + good.recs[0][1:]] + good.recs[1:]),
        "rec_slice < 0": but(EINVAL, recs=[(-1,) + good.recs[0][1:]] + good.recs[1:]),
        "n_carry == 0xff00": but(EINVAL, carry=b"z" * P),
        "level 2": but(EINVAL, level=2),
        "level -1": but(EINVAL, level=-1),
        "a slice ends inside a member": but(EIO, slices=[(s_at, s_n - 9, s_raw)], recs=good.recs[:1]),
        "a slice begins inside a member": but(EIO, slices=[(s_at + 5, s_n - 5, s_raw)]),
        "a member's CRC-32 is wrong": but(EIO, spool=spool[:crc_at] + bytes([spool[crc_at] ^ 0x10]) + spool[crc_at + 1:]),
        "a member's ISIZE is wrong": but(EIO, spool=spool[:crc_at + 4] + bytes([spool[crc_at + 4] ^ 1]) + spool[crc_at + 5:], recs=good.recs[:1]),
    }
