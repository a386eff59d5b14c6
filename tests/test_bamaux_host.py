"""Copied aux tags on the host: the bounded walk and the split of mappy-rs_amd/csrc/mm355_bamaux.h and the host formatter with tags
(mm355_bam.h), built with g++ under AddressSanitizer and UBSan into a stand-alone program (tests/host_harness/bamaux_host.cpp), against the
model of tests/_bamaux.py; and, in process through the library, the reader that keeps the tags of a BAM's records and the @RG lines of its
header (mm355_bamread.h, mm355_index.cpp).  GPU side: tests/test_gpu_bamaux.py."""
import ctypes as C
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import _bam
import _bam_sets as BS
import _bamaux as A
import _capi
import _inflate as I
import _sam_sets as SS

EINVAL, EIO = -2, -4


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bamaux_host") / "bamaux_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(_capi.HERE, "host_harness", "bamaux_host.cpp"), "-o", exe, "-lz", "-lpthread"])
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


# ---------------------------------------------------------------- the walk and the split
def _split(harness, tmp_path, cases, tag="cases"):
    """cases: (aux, keep or None) -> per case None (refused) or (kept, mod_off)"""
    src, dst = tmp_path / (tag + ".bin"), tmp_path / (tag + ".out")
    src.write_bytes(b"".join(struct.pack("<ii", len(a), -1 if k is None else len(k)) + (k or "").encode("latin-1") + a for a, k in cases))
    assert _run(harness, "split", src, dst) == ["split %d" % len(cases)]
    got, out, at = dst.read_bytes(), [], 0
    for _ in cases:
        rc, n_out, mod = struct.unpack_from("<iii", got, at)
        at += 12
        assert rc in (0, EINVAL)
        out.append((got[at:at + n_out], mod) if rc == 0 else None)
        at += n_out if rc == 0 else 0
    assert at == len(got)
    return out


EVERY = [("xA", "A", b"q"), ("xc", "c", -5), ("xC", "C", 250), ("xs", "s", -30000), ("xS", "S", 65000), ("xi", "i", -2**31), ("xI", "I", 2**32 - 1),
         ("xf", "f", 1.5), ("xd", "d", -2.25), ("xZ", "Z", b"some text"), ("xH", "H", b"1AE301"), ("eZ", "Z", b"")] + \
        [("B" + sub, "B", (sub, vals)) for sub, vals in (("c", [-1, 2]), ("C", [1, 2, 3]), ("s", [-7]), ("S", [7, 8]), ("i", [-9, 9]), ("I", [2**32 - 1]), ("f", [0.5, -0.5]))] + \
        [("z" + sub, "B", (sub, [])) for sub in A.B_SUBTYPES]


def test_every_type_splits_as_the_model(harness, tmp_path):
    whole = A.block(EVERY)
    cases = [(A.tag(*t), "*") for t in EVERY] + [(whole, "*"), (b"", "*"), (A.tag("xi", "i", 7), "*")]
    got = _split(harness, tmp_path, cases)
    assert got == [A.split(a, k) for a, k in cases] and None not in got
    assert got[len(EVERY)] == (whole, len(whole)) and got[-2] == (b"", 0) and got[-1] == (A.tag("xi", "i", 7), 7)


def test_keep_forms_dropped_names_and_group_order(harness, tmp_path):
    own = [(n.decode(), "C", 1) for n in A.OWN]
    tags = [("MM", "Z", b"C+m,1;"), ("RG", "Z", b"grp"), ("ML", "B", ("C", [200])), ("qs", "f", 12.5)] + own[:8] + [("MN", "i", 400), ("Mm", "Z", b"x"), ("mv", "B", ("c", [1, 0, 1]))] + \
           own[8:] + [("Ml", "B", ("C", [])), ("MM", "Z", b"again")]
    blk = A.block(tags)
    t = {i: A.tag(*x) for i, x in enumerate(tags)}
    keeps = ["*", "MMML", "RG", "MMMLMN", "NMRG", "zz", "qsMlmv", "", "M", "MML", "**", None]
    got = _split(harness, tmp_path, [(blk, k) for k in keeps])
    assert got == [None if k is None else A.split(blk, k) for k in keeps]
    first = t[1] + t[3] + A.tag("mv", "B", ("c", [1, 0, 1]))
    mods = t[0] + t[2] + A.tag("MN", "i", 400) + A.tag("Mm", "Z", b"x") + A.tag("Ml", "B", ("C", [])) + A.tag("MM", "Z", b"again")
    assert got[0] == (first + mods, len(first))                      # every own name dropped, input order inside each group
    assert got[1] == (t[0] + t[2] + A.tag("MM", "Z", b"again"), 0) and got[2] == (t[1], len(t[1])) and got[4] == got[2] and got[5] == (b"", 0)
    assert got[7:10] == [None] * 3 and got[10] == (b"", 0) and got[11] is None   # empty and odd; "**" is a name that matches nothing; NULL


def _refusals():
    good = A.tag("xZ", "Z", b"ok")
    out = [("unknown type", b"xxQ\1"), ("unknown type after a good tag", good + b"xx?\0"), ("B subtype A", b"xxBA" + struct.pack("<I", 1) + b"a"),
           ("B subtype d", b"xxBd" + struct.pack("<I", 0)), ("B subtype Z", b"xxBZ" + struct.pack("<I", 0))]
    for t, v in (("A", b"q"), ("c", -1), ("C", 1), ("s", 1), ("S", 1), ("i", 1), ("I", 1), ("f", 1.0), ("d", 1.0)):
        whole = A.tag("xx", t, v)
        out += [("%s cut to %d" % (t, k), good + whole[:k]) for k in range(3, len(whole))]
    out += [("Z without NUL", b"xxZabc"), ("H without NUL", b"xxH1A"), ("Z without a byte", b"xxZ"), ("Z NUL only behind the block", good + b"xxZabc")]
    out += [("B count overruns", b"xxBC" + struct.pack("<I", 5) + b"abcd"), ("B header cut", b"xxBC\1\0\0"), ("B count 2^32-1", b"xxBC" + struct.pack("<I", 2**32 - 1) + b"ab"),
            ("B product wraps 32 bits", b"xxBI" + struct.pack("<I", 2**30 + 1) + b"abcd"), ("B S product wraps", b"xxBS" + struct.pack("<I", 2**31 + 2) + b"abcd")]
    out += [("stub of %d" % k, good + b"xxi"[:k]) for k in (1, 2, 3)] + [("stub alone %d" % k, b"xyZ"[:k]) for k in (1, 2)]
    return out


def test_each_refusal(harness, tmp_path):
    cases = _refusals()
    assert all(A.split(b) is None for _, b in cases), [n for n, b in cases if A.split(b) is not None]
    got = _split(harness, tmp_path, [(b, "*") for _, b in cases])
    assert got == [None] * len(cases), [n for (n, _), g in zip(cases, got) if g is not None]
    # the wrapped products would fit if computed in 32 bits: (2^30 + 1) * 4 = 4, (2^31 + 2) * 2 = 4
    assert (2**30 + 1) * 4 % 2**32 == 4 and (2**31 + 2) * 2 % 2**32 == 4


def test_bit_flips_and_truncations_get_the_models_verdict(harness, tmp_path):
    """20 000 mutants of valid blocks, none left out: the verdict and, where accepted, the bytes are the model's; the sanitizers stay silent
    (every block and output buffer of the program is a heap block of its exact size)"""
    rng = np.random.default_rng(77)
    bases = [A.block(EVERY), A.block(EVERY[::-1]) + A.mod_pair(40, rng), A.mod_pair(300, rng) + A.tag("RG", "Z", b"g1") + A.tag("NM", "C", 3),
             A.block([("xb", "B", ("I", [1, 2, 3])), ("yb", "B", ("s", [-1] * 9)), ("xZ", "Z", b"")])]
    cases = []
    for k in range(20000):
        b = bytearray(bases[k % len(bases)])
        if k % 5 == 4:
            b = b[:int(rng.integers(0, len(b)))]
        else:
            at = int(rng.integers(0, len(b)))
            b[at] ^= 1 << int(rng.integers(0, 8))
        cases.append((bytes(b), ("*", "MMML", "RGxZ")[k % 3]))
    got = _split(harness, tmp_path, cases, "mutants")
    want = [A.split(a, k) for a, k in cases]
    assert len(got) == 20000 and got == want, next(i for i, (g, w) in enumerate(zip(got, want)) if g != w)
    n_bad = sum(w is None for w in want)
    assert 2000 < n_bad < 18000                                   # both verdicts are well represented


# ---------------------------------------------------------------- the host formatter with tags
def _row(qs, qe, strand, kind, cigar, n_cigar=1, rid=0, ts=100):
    """a row over read[qs:qe]: kind 0 the primary with sam_pri, 1 a supplementary, 2 a secondary; its CIGAR words are appended to `cigar`"""
    r = dict(query_start=qs, query_end=qe, strand=strand, rid=rid, target_len=3000, target_start=ts, target_end=ts + (qe - qs), match_len=qe - qs,
             block_len=max(1, qe - qs), mapq=60, is_primary=int(kind != 2), n_cigar=n_cigar, cigar_off=len(cigar))
    cigar += [max(1, qe - qs) << 4] + [3 << 4 | 7] * (n_cigar - 1)
    return r, dict(score=qe - qs, flags=2 if kind == 0 else 0)


def _auxes(s, rng, k):
    """per read of the set: tags of the k-th length of A.LENGTHS, rotating from read to read and from set to set; one in five none, one in
    seven only the second group (prefix 0)"""
    out = []
    for i in range(len(s["seqs"])):
        n, j = A.LENGTHS[(k + i) % len(A.LENGTHS)], k // len(A.LENGTHS) + i
        out.append(None if j % 5 == 4 else A.two_groups(n, rng, first=0) if j % 7 == 6 and n >= 12 else A.two_groups(n, rng))
    return out


def _format(harness, tmp_path, sets, auxes, level=0, tag="sets"):
    src, aux, dst = tmp_path / (tag + ".bin"), tmp_path / (tag + ".aux"), tmp_path / (tag + ".out")
    src.write_bytes(SS.serialize(sets))
    aux.write_bytes(A.serialize_aux(auxes))
    assert _run(harness, "sets", src, aux, dst, level)[-1] == "sets %d" % len(sets)
    got, at, out = dst.read_bytes(), 0, []
    for s in sets:
        nr = len(s["seqs"])
        n_text, n_lines = np.frombuffer(got, np.int64, 2, at).tolist()
        out.append((got[at + 8 * (nr + 3):at + 8 * (nr + 3) + n_text], np.frombuffer(got, np.int64, nr + 1, at + 16).tolist(), n_lines))
        at += 8 * (nr + 3) + n_text
    assert at == len(got)
    return out


@pytest.fixture(scope="module")
def sets(built):
    rng = np.random.default_rng(5)
    return BS.random_sets(991, 360) + [BS.long_cigar_set(65536, rng, 1), BS.long_cigar_set(65536, rng, -1), BS.long_cigar_set(65535, rng, 1)]


def test_host_formatter_equals_with_aux(harness, sets, tmp_path):
    rng = np.random.default_rng(6)
    auxes = [_auxes(s, rng, k) for k, s in enumerate(sets)]
    auxes[-3:] = [[A.two_groups(n, rng)] for n in (4097, 17, 16)]        # the long-CIGAR records: CG must stay last
    seen, lengths, prefix0, cg_last = set(), set(), 0, 0
    for k, (s, ax, (text, line_off, n_lines)) in enumerate(zip(sets, auxes, _format(harness, tmp_path, sets, auxes))):
        want, want_off = A.expected(s, ax)
        plain = BS.expected(s)[0]
        got = _bam.split(text)
        assert got == want, (k, s["sam_flags"], [i for i, (a, b) in enumerate(zip(got, want)) if a != b][:3], len(got), len(want))
        assert line_off == want_off and n_lines == len(want) and text == _bam.frame(b"".join(want)), k
        for r, p in zip(want, plain):
            flag = struct.unpack_from("<H", r, 18)[0]
            if len(r) > len(p):
                seen.add((flag & 0x914, s["sam_flags"]))
                lengths.add(len(r) - len(p))
                cg_last += p.find(b"CGBI") > 0 and r[-(len(p) - p.find(b"CGBI")):] == p[p.find(b"CGBI"):]
        prefix0 += sum(a is not None and a[1] == 0 and len(a[0]) > 0 for a in ax)
    kinds = {f for f, _ in seen}
    assert kinds >= {0, 0x10, 0x100, 0x110, 0x800, 0x810, 4} and {fl for _, fl in seen} == {0, 1, 2, 3}
    assert lengths >= set(A.LENGTHS[1:]) and prefix0 > 0 and cg_last == 2


def test_record_classes_by_hand(harness, built, tmp_path):
    """one read with a primary, a hard-clipped supplementary and a secondary; tags of two groups: all on the primary, the first group on
    the other two; under soft clipping all on every record; tags of the second group only: nothing on the other two"""
    rng = np.random.default_rng(8)
    cigar = []
    seq, qual = SS.random_read(rng, 60)
    rows = [_row(0, 40, 1, 0, cigar), _row(40, 60, -1, 1, cigar, 2, 1), _row(5, 30, 1, 2, cigar, 1, 2)]
    first, mod = A.tag("RG", "Z", b"g") + A.tag("qs", "f", 9.5), A.tag("MM", "Z", b"C+m,3;") + A.tag("ML", "B", ("C", [255]))
    out = {}
    for fl in (0, SS.SOFTCLIP):
        s = BS.scrub(SS.make_set([r for r, _ in rows], [t for _, t in rows], [0, 3], [0], ["q"], [seq], [qual], [0], fl, cigar=cigar), rng)
        plain = BS.expected(s)[0]
        for name, ax in (("both", (first + mod, len(first))), ("mod", (mod, 0))):
            (text, _, _), = _format(harness, tmp_path, [s], [[ax]])
            out[fl, name] = [g[len(p):] if g[4:len(p)] == p[4:] else None for g, p in zip(_bam.split(text), plain)]   # what stands behind the record's own bytes
    assert out[0, "both"] == [first + mod, first, first] and out[0, "mod"] == [mod, b"", b""]
    assert out[SS.SOFTCLIP, "both"] == [first + mod] * 3 and out[SS.SOFTCLIP, "mod"] == [mod] * 3


def test_level_1_inflates_to_level_0(harness, sets, tmp_path):
    rng = np.random.default_rng(9)
    some = sets[:40] + sets[-1:]
    auxes = [_auxes(s, rng, k) for k, s in enumerate(some)]
    for (t0, off0, n0), (t1, off1, n1) in zip(_format(harness, tmp_path, some, auxes, 0, "l0"), _format(harness, tmp_path, some, auxes, 1, "l1")):
        assert (off0, n0) == (off1, n1) and len(t1) <= len(t0) and (gzip.decompress(t1) if t1 else b"") == (gzip.decompress(t0) if t0 else b"")


def test_check_refuses(harness, built, tmp_path):
    good = next(s for s in BS.random_sets(8, 400) if len(s["seqs"]) >= 2 and s["hit_off"][1] > 0 and s["status"][0] == 0 and s["status"][1] == 0)
    nr = len(good["seqs"])
    blk = A.filler(16)
    huge = SS.make_set([], [], [0, 0], [0], ["u"], ["ACGT"], [None], [0], 0)
    huge["qlens"][0] = 2**31 - 8                               # (the check reads lengths, never the bases or the tags)
    cases = [("good", good, [(blk, 16)] + [None] * (nr - 1), 0), ("empty everywhere", good, [(b"", 0)] * nr, 0), ("absent everywhere", good, [None] * nr, 0),
             ("mod 0", good, [(blk, 0)] + [None] * (nr - 1), 0),
             ("negative length", good, [(-1, 0, blk)] + [None] * (nr - 1), EINVAL), ("negative length on a later read", good, [None, (-5, 0, None)] + [None] * (nr - 2), EINVAL),
             ("null with a length", good, [(16, 0, None)] + [None] * (nr - 1), EINVAL), ("mod above the length", good, [(16, 17, blk)] + [None] * (nr - 1), EINVAL),
             ("negative mod", good, [(16, -1, blk)] + [None] * (nr - 1), EINVAL),
             ("what mm355_bam_check refuses", dict(good, hits=_with(good["hits"], "mapq", 256)), [(blk, 16)] + [None] * (nr - 1), EINVAL),
             ("a long read alone passes", huge, [None], 0), ("a record beyond block_size", huge, [(2**31 - 1, 0, blk)], EINVAL),
             ("the same tags on a short read pass", dict(huge, qlens=np.array([4], np.int32)), [(2**31 - 1, 0, blk)], 0)]
    for name, s, ax, rc in cases:
        src, aux = tmp_path / "c.bin", tmp_path / "c.aux"
        src.write_bytes(SS.serialize([s]))
        aux.write_bytes(A.serialize_aux([ax]))
        assert _run(harness, "check", src, aux) == ["rc %d" % rc, "sets 1"], name


def _with(hits, field, value):
    h = hits.copy()
    h[field][0] = value
    return h


# ---------------------------------------------------------------- the reader, in process
def _read_aux(L, ffi, path, keep, max_reads=3, late=False, opener=None):
    """every read of the file as (name, seq, qual, aux, aux_mod) -- aux None where mm355_reads_aux is NULL -- the @RG lines, or a return code"""
    fx = C.c_void_p()
    rc = opener(fx) if opener else L.mm355_fastx_open_qual(os.fsencode(str(path)), C.byref(fx))
    assert rc == 0
    out = []
    try:
        if not late:
            assert L.mm355_fastx_keep_aux(fx, keep) == 0
        n_rg = C.c_int64(-1)
        rg = L.mm355_fastx_bam_rg(fx, C.byref(n_rg))
        rg = C.string_at(rg, n_rg.value) if rg else None
        assert (rg is None) == (n_rg.value == 0)
        while True:
            rp = C.POINTER(ffi.Reads)()
            rc = L.mm355_fastx_next(fx, max_reads, 1 << 30, C.byref(rp))
            if late:
                L.mm355_reads_free(rp)
                return L.mm355_fastx_keep_aux(fx, keep)
            if rc:
                return rc
            if not rp:
                return out, rg
            r = rp.contents
            qs = L.mm355_reads_quals(rp)
            ln, md = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
            ap = L.mm355_reads_aux(rp, C.byref(ln), C.byref(md))
            assert bool(ap) == bool(ln) == bool(md)
            for i in range(r.n):
                out.append((r.names[i], C.string_at(r.seqs[i], r.lens[i]), C.string_at(qs[i], r.lens[i]) if qs and qs[i] else None,
                            C.string_at(ap[i], ln[i]) if ap else None, md[i] if ap else None))
            L.mm355_reads_free(rp)
    finally:
        L.mm355_fastx_close(fx)


def reads_with_tags(n=12, seed=4):
    """(records as (name, seq, qual), the aux block of each, the uninflated BAM): one record in three on the reverse strand, a secondary
    and a supplementary record in between, header with two @RG lines"""
    rng = np.random.default_rng(seed)
    recs = I.fastq_records(n, seed, with_n=False)
    auxes, body = [], b""
    for i, (nm, sq, ql) in enumerate(recs):
        tags = [("RG", "Z", b"grp%d" % (i % 2)), ("qs", "f", 10.0 + i), ("NM", "C", 1), ("mv", "B", ("c", rng.integers(0, 2, 5 + i).tolist()))]
        aux = A.tag("MN", "i", len(sq)) + A.block(tags[:2]) + A.mod_pair(len(sq), rng) + A.block(tags[2:])
        if i == 5:
            aux = b""
        auxes.append(aux)
        body += I.bam_record(nm, sq, ql, flag=0x10 if i % 3 == 1 else 4 if i % 3 else 0, aux=aux)
        if i % 4 == 0:
            body += I.bam_record(nm, sq[:1], None, flag=0x900 if i % 8 else 0x100, aux=b"xxQ")     # (skipped: its broken aux is never looked at)
    text = b"@HD\tVN:1.6\tSO:unknown\n@RG\tID:grp0\tSM:s\n@PG\tID:basecaller\n@RG\tID:grp1\tSM:s\tDS:@RG\tinside\n@CO\t@RG\tno\n"
    return recs, auxes, I.bam_header(text) + body


RG2 = b"@RG\tID:grp0\tSM:s\n@RG\tID:grp1\tSM:s\tDS:@RG\tinside\n"


def test_reader_keeps_and_filters_aux(built, tmp_path):
    from mappy_rs import _ffi
    L = _ffi.lib()
    recs, auxes, data = reads_with_tags()
    bam = tmp_path / "t.bam"
    bam.write_bytes(I.bgzf_file(data, 701))
    want = [(n, s, q) for n, s, q in recs]
    for keep in (b"*", b"MMML", b"RGmvMN", b"zz"):
        got, rg = _read_aux(L, _ffi, bam, keep)
        assert [g[:3] for g in got] == want and rg == RG2                                     # a 0x10 record is turned back, its aux verbatim
        assert [g[3:] for g in got] == [A.split(a, keep.decode()) for a in auxes], keep
    # nothing kept: today's reads, no aux arrays
    got, rg = _read_aux(L, _ffi, bam, None)
    assert [g[:3] for g in got] == want and all(g[3] is None for g in got) and rg == RG2
    # after the first mm355_fastx_next, and a malformed list of names
    assert _read_aux(L, _ffi, bam, b"*", late=True) == EINVAL
    fx = C.c_void_p()
    assert L.mm355_fastx_open(os.fsencode(str(bam)), C.byref(fx)) == 0
    assert [L.mm355_fastx_keep_aux(fx, k) for k in (b"", b"M", b"MML", b"MM", b"*", None)] == [EINVAL, EINVAL, EINVAL, 0, 0, 0]
    L.mm355_fastx_close(fx)
    # a malformed block: the records before it have been handed out in earlier sub-batches, the call that meets it answers MM355_EIO
    for bad in (b"xxQ\0", b"xxZabc", b"xxBC" + struct.pack("<I", 2**32 - 1), b"xx"):
        blob = I.bam_header() + I.bam_record(b"a", b"ACGT", b"IIII", aux=A.tag("RG", "Z", b"g")) + I.bam_record(b"b", b"ACGT", b"IIII", aux=bad)
        bam.write_bytes(I.bgzf_file(blob, 701))
        assert _read_aux(L, _ffi, bam, b"*", max_reads=1) == EIO, bad
        assert len(_read_aux(L, _ffi, bam, None)[0]) == 2                                     # (skipped, as before, when nothing is kept)


def test_rg_lines_and_other_streams(built, tmp_path):
    from mappy_rs import _ffi
    L = _ffi.lib()
    rec = I.bam_record(b"a", b"ACGT", b"IIII", aux=A.tag("RG", "Z", b"g"))
    p = tmp_path / "h.bam"
    for text, rg in ((b"@HD\tVN:1.6\n@PG\tID:x\n", None), (b"", None), (b"@RG\tID:g\n", b"@RG\tID:g\n"), (b"@HD\tVN:1.6\n@RG\tID:g", b"@RG\tID:g\n"),
                     (b"@RG\tID:a\n@RGX\tno\n@RG\n@rg\tID:no\n@RG\tID:b\n\0\0@RG\tID:padding\n", b"@RG\tID:a\n@RG\tID:b\n"), (RG2 * 3000, RG2 * 3000)):
        p.write_bytes(I.bgzf_file(I.bam_header(text) + rec, 509))
        got, lines = _read_aux(L, _ffi, p, b"*")
        assert lines == rg and got == [(b"a", b"ACGT", b"IIII", A.tag("RG", "Z", b"g"), 5)], text[:40]
    # a FASTQ, plain and bgzip: keep_aux has no effect, no @RG, no aux arrays
    recs = I.fastq_records(7)
    for name, blob in (("r.fq", I.fastq_text(recs)), ("r.fq.gz", I.bgzf_file(I.fastq_text(recs), 300))):
        (tmp_path / name).write_bytes(blob)
        got, lines = _read_aux(L, _ffi, tmp_path / name, b"*")
        assert lines is None and [g[:3] for g in got] == recs and all(g[3] is None for g in got)
    # a header cut inside its text: MM355_EIO from the reader, NULL from mm355_fastx_bam_rg
    p.write_bytes(I.bgzf_file(I.bam_header(RG2)[:20], 509))
    fx, n = C.c_void_p(), C.c_int64(5)
    assert L.mm355_fastx_open(os.fsencode(str(p)), C.byref(fx)) == 0 and not L.mm355_fastx_bam_rg(fx, C.byref(n)) and n.value == 0
    rp = C.POINTER(_ffi.Reads)()
    assert L.mm355_fastx_next(fx, 1, 1 << 30, C.byref(rp)) == EIO and not rp
    L.mm355_fastx_close(fx)


def test_python_surface_without_a_gpu(built):
    import mappy_rs
    blk = A.block(EVERY) + A.mod_pair(20, np.random.default_rng(1)) + A.tag("NM", "C", 1)
    assert mappy_rs.bam_aux_split(blk) == A.split(blk) and mappy_rs.bam_aux_split(blk, "MLxZ") == A.split(blk, "MLxZ") and mappy_rs.bam_aux_split(b"") == (b"", 0)
    for bad, keep in ((b"xxQ\0", "*"), (blk, ""), (blk, "MML"), (blk[:-1], "*")):
        with pytest.raises(ValueError):
            mappy_rs.bam_aux_split(bad, keep)
    assert [mappy_rs._keep_of(x) for x in (False, None, True, ("MM", "ML"), ["RG"], iter(["MM", "MN"]))] == [None, None, b"*", b"MMML", b"RG", b"MMMN"]
    for bad in ("MM", b"MM", ["M"], ["MML"], [b"MM"], [], 1, ["MM", None], ("M\tM",)):
        with pytest.raises(ValueError):
            mappy_rs._keep_of(bad)
