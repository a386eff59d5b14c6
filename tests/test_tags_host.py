"""minimap2's PAF tags (MM355_OUT_TAGS, Aligner(tags=True)) on the CPU.

The region stage: mm355_regs.h compiled for the host (tests/host_harness/regs_tags_host.cpp) must give, next to every hit row, the tags
row the oracle's mm_reg1_t of the same region holds: r->score, r->div (bit for bit), the read's rep_len and sam_pri as mm_sync_regs leaves
it.  The pow rule: with tags a read is deferred when any surviving region's divergence is unsure, without tags only when a strand_retained
comparison reads it.  The Python surface: properties, detach(), paf_line against hand-written lines.  GPU side: tests/test_gpu_tags.py."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O
import _capi
import synthdata as S
from test_chain_only_host import ALL_CHAINS, _inverted_genome
import _tags_truth as T

DEFER_POW = 2


@pytest.fixture(scope="module")
def tags_lib(built):
    L = _capi.build_harness("regs_tags_host", ["-w", "-ffp-contract=off"], ["mm355_regs.h", "mm355_core.h"])
    L.regs_tags_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.regs_tags_host.restype = C.c_int
    return L


def _dtypes():
    import mappy_rs
    return mappy_rs._HIT_DTYPE, mappy_rs._TAG_DTYPE


def test_struct_sizes(tags_lib):
    from mappy_rs import _ffi
    hd, td = _dtypes()
    assert tags_lib.regs_tags_size() == C.sizeof(_ffi.Tags) == td.itemsize == 32
    assert hd.itemsize == C.sizeof(_ffi.Hit) == 128        # mm355_hit_t keeps its layout
    assert tags_lib.regs_reg_size() == 80                  # the device's region record did not grow with sam_pri


def harness_rows(L, orc, seq, want_tags=True, force_unsure=-1):
    """the read through the oracle's front and mm355_regs.h's tail: ([hit dict], [tags tuple]) or the negative defer code"""
    mo = orc.mo
    qlen = len(seq)
    if mo.max_qlen > 0 and qlen > mo.max_qlen:
        return [], []
    a, rep_len, mini_pos, _ = orc.anchors(seq, sorted_=True)
    if len(a) == 0:
        return [], []
    u, ca, _ = orc.chains_final(a, qlen)
    if len(u) == 0:
        return [], []
    opt_i = np.array([mo.flag, mo.mask_len, mo.best_n, orc.k * 2, int(mo.max_gap * 0.8), mo.min_chain_score, mo.seed], np.int64)
    opt_f = np.array([mo.mask_level, mo.pri_ratio], np.float32)
    seq_len = np.array(orc.seq_lens, np.uint32)
    u = np.ascontiguousarray(u, np.uint64); ca = np.ascontiguousarray(ca, np.uint64); mp = np.ascontiguousarray(mini_pos, np.uint64)
    hd, td = _dtypes()
    out = np.zeros(len(u), hd)
    tg = np.full(len(u), 0x55, np.uint8).repeat(td.itemsize).view(td)       # every byte of a written row must come from the header
    n = L.regs_tags_host(opt_i.ctypes.data, opt_f.ctypes.data, seq_len.ctypes.data, qlen, rep_len, len(u), u.ctypes.data, ca.ctypes.data,
                         len(mp), mp.ctypes.data, out.ctypes.data, tg.ctypes.data if want_tags else None, force_unsure)
    if n < 0:
        return n
    hits = [{k: int(h[k]) for k in T.HIT_FIELDS} for h in out[:n]]
    if not want_tags:
        return hits, None
    tags = []
    for t in tg[:n]:
        assert int(t["reserved"]) == 0 and int(t["flags"]) & ~2 == 0      # chain-only: no inversion, no split
        tags.append((int(t["score"]), T.f32_bits(t["div"]), int(t["rep_len"]), int(t["n_ambi"]), int(t["n_gap"]), int(t["n_gapo"]),
                     0, int(t["flags"]) >> 1 & 1, 0))
    return hits, tags


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    """the world of tests/test_gpu_chain_only.py, plus unmutated reads (a chain that matches every minimizer of its span: div == 0)"""
    td = tmp_path_factory.mktemp("tagshost")
    g = _inverted_genome(71)
    fa = str(td / "ref.fa")
    S.write_fasta(fa, g, ["chrA", "chrB"])
    reads, _ = S.make_reads(81, g, 300, n50=6000, lo=300)
    rng = np.random.default_rng(82)
    for st in (100000, 104000, 110000, 101500):
        reads.append(S.codes_to_str(S.mutate(g[0][st:st + 18000], rng, 0.02, 0.01, 0.01)))
    # (mm_est_err counts one more expected minimizer whenever the region stops short of the contig's end: only reads that reach it give 0)
    exact = [S.codes_to_str(g[0][700000:703000]), S.codes_to_str(g[0][0:2500]), S.codes_to_str(g[1][-2000:]), S.codes_to_str(g[0][-3000:]),
             S.codes_to_str(g[1][-5000:]), S.codes_to_str((3 - g[0][-4000:])[::-1].astype(np.uint8))]
    return dict(fa=fa, g=g, reads=reads + exact, n_base=len(reads))


CASES = [("map-ont", {}), ("map-hifi", {}), ("asm20", {}), ("ava-ont", {}), ("map-ont", {"extra_flags": ALL_CHAINS})]
IDS = ["%s-%s" % (p, "all_chains" if kw else "default") for p, kw in CASES]


@pytest.mark.parametrize("preset,kw", CASES, ids=IDS)
def test_tags_rows_equal_oracle_chain_only(tags_lib, world, preset, kw):
    orc = O.OracleAligner(world["fa"], preset=preset, **kw)
    orc.mo.flag &= ~4
    n_hits = n_sec = n_rep = n_zero = n_sam = n_pri_not_sam = 0
    for i, rd in enumerate(world["reads"]):
        exp = T.oracle_tags(orc, rd)
        got = harness_rows(tags_lib, orc, rd)
        assert not isinstance(got, int), (preset, i, got)        # glibc's pow on both sides: est_err marks about one region in 10^6
        hits, tags = got
        assert hits == [{k: e[k] for k in T.HIT_FIELDS} for e in exp], (preset, i)
        assert tags == [T.tags_tuple(e) for e in exp], (preset, i)
        no_tags = harness_rows(tags_lib, orc, rd, want_tags=False)
        assert no_tags[0] == hits                                  # the rows do not depend on the request
        n_zero += sum(e["div"] == 0.0 for e in exp)
        n_sam += sum(e["sam_pri"] for e in exp); n_pri_not_sam += sum(e["is_primary"] and not e["sam_pri"] for e in exp)
        if i < world["n_base"]:
            n_hits += len(exp); n_sec += sum(not e["is_primary"] for e in exp); n_rep += bool(exp) and exp[0]["rep_len"] > 0
    assert n_zero >= 3, n_zero
    if (preset, kw) == ("map-ont", {}):
        assert (n_hits, n_sec, n_rep) == (323, 19, 134)
        assert n_sam > 0 and n_pri_not_sam > 0       # sam_pri is set only where select_sub dropped a region (mm_sync_regs)
    else:
        assert n_hits > 250


def test_unsure_divergence_defers_only_with_tags(tags_lib, world):
    """a region whose divergence pow() rounding could move: with tags the read goes to the host (the value is reported), without tags it does
    not (no strand_retained comparison reads it) and the rows are the oracle's"""
    orc = O.OracleAligner(world["fa"], preset="map-ont")
    orc.mo.flag &= ~4
    rd = world["reads"][0]
    exp = T.oracle_tags(orc, rd)
    assert len(exp) >= 1
    assert harness_rows(tags_lib, orc, rd, want_tags=True, force_unsure=0) == -DEFER_POW
    hits, _ = harness_rows(tags_lib, orc, rd, want_tags=False, force_unsure=0)
    assert hits == [{k: e[k] for k in T.HIT_FIELDS} for e in exp]
    hits, tags = harness_rows(tags_lib, orc, rd, want_tags=True, force_unsure=len(exp) + 5)      # a mark on no surviving region: not deferred
    assert tags == [T.tags_tuple(e) for e in exp]


# ---------------------------------------------------------------- the Python surface on constructed records (no device needed)
def records(rows, tags, chain_only, cigar=(), sbuf=b""):
    """Mapping records of one read from hit rows / tags rows given as dicts, through mappy_rs._batch_to_mappings"""
    import mappy_rs
    from mappy_rs import _ffi
    hd, td = _dtypes()
    n = len(rows)
    ha = np.zeros(n, hd)
    for i, r in enumerate(rows):
        ha[i]["cs_len"] = ha[i]["md_len"] = -1
        for k, v in r.items():
            ha[i][k] = v
    hbuf = C.create_string_buffer(ha.tobytes(), max(1, n * hd.itemsize))
    tbuf = None
    if tags is not None:
        ta = np.zeros(n, td)
        for i, r in enumerate(tags):
            for k, v in r.items():
                ta[i][k] = v
        tbuf = C.create_string_buffer(ta.tobytes(), max(1, n * td.itemsize))
    cg = (C.c_uint32 * max(1, len(cigar)))(*cigar)
    sb = C.create_string_buffer(sbuf, max(1, len(sbuf)))
    off = (C.c_int64 * 2)(0, n)
    st = (C.c_int32 * 1)(0)
    h = _ffi.Hits(n_reads=1, hit_off=off, status=st, hits=C.cast(hbuf, C.POINTER(_ffi.Hit)), cigar=cg, str=C.cast(sb, C.POINTER(C.c_char)),
                  n_hits=n, n_cigar=len(cigar), n_str=len(sbuf), tags=C.cast(tbuf, C.POINTER(_ffi.Tags)) if tbuf is not None else None)
    return mappy_rs._batch_to_mappings(C.pointer(h), 1, ["chr1", "chr2"], chain_only=chain_only)[0]


CHAIN_ROW = dict(query_start=12, query_end=4890, strand=1, rid=0, target_len=1500000, target_start=100200, target_end=105123, match_len=1741,
                 block_len=4923, mapq=60, is_primary=1, score0=1700, cnt=180, subsc=42)
CIG = [200 << 4 | 0, 2 << 4 | 1, 300 << 4 | 0, 5 << 4 | 2, 100 << 4 | 0, 1 << 4 | 1, 49 << 4 | 0]       # 200M2I300M5D100M1I49M
CIGAR_ROW = dict(query_start=0, query_end=652, strand=-1, rid=1, target_len=900000, target_start=7000, target_end=7654, match_len=630,
                 block_len=657, mapq=0, is_primary=0, NM=28, n_cigar=7, cigar_off=0, cs_off=0, cs_len=9, score0=610, cnt=61, subsc=0,
                 dp_max=1100, dp_score=1090)


def test_paf_line_chain_only_primary():
    import mappy_rs
    m, = records([CHAIN_ROW], [dict(score=1690, div=np.float32(0.0312), rep_len=37, flags=2)], chain_only=True)
    assert mappy_rs.paf_line(m, "read1", 5000) == \
        "read1\t5000\t12\t4890\t+\tchr1\t1500000\t100200\t105123\t1741\t4923\t60\ttp:A:P\tcm:i:180\ts1:i:1690\ts2:i:42\tdv:f:0.0312\trl:i:37"
    assert (m.s1, m.s2, m.cm, m.ms, m.AS, m.nn, m.rl, m.zd, m.de, m.tp, m.is_supplementary) == (1690, 42, 180, 0, 0, 0, 37, 0, None, "P", False)
    assert T.f32_bits(m.dv) == T.f32_bits(np.float32(0.0312))


def test_paf_line_divergence_exactly_zero_and_not_estimated():
    import mappy_rs
    m, m2, m3 = records([CHAIN_ROW, dict(CHAIN_ROW, is_primary=0), CHAIN_ROW],
                        [dict(score=1700, div=0.0, rep_len=0, flags=0), dict(score=900, div=-1.0, rep_len=0), dict(score=5, div=1.5, rep_len=0)], chain_only=True)
    assert mappy_rs.paf_line(m, "r", 5000).endswith("\ttp:A:P\tcm:i:180\ts1:i:1700\ts2:i:42\tdv:f:0\trl:i:0")
    assert m.dv == 0.0 and m.is_supplementary is True          # primary without sam_pri
    assert mappy_rs.paf_line(m2, "r", 5000).endswith("\ttp:A:S\tcm:i:180\ts1:i:900\trl:i:0")     # secondary: no s2; div -1: no dv
    assert m2.dv is None and m2.is_supplementary is False
    assert m3.dv is None and "dv:f" not in mappy_rs.paf_line(m3, "r", 5000)


def test_paf_line_cigar_secondary():
    import mappy_rs
    m, = records([CIGAR_ROW], [dict(score=598, div=np.float32(0.04), rep_len=120, n_ambi=1, n_gap=8, n_gapo=3, flags=0)], chain_only=False,
                 cigar=CIG, sbuf=b":200+ac:3\0")
    # de = 1 - 630 / (657 + 1 - 8 + 3) = 1 - 630 / 653 = 0.035222...
    assert mappy_rs.paf_line(m, "q7", 700) == \
        "q7\t700\t0\t652\t-\tchr2\t900000\t7000\t7654\t630\t657\t0\tNM:i:28\tms:i:1100\tAS:i:1090\tnn:i:1\ttp:A:S\tcm:i:61\ts1:i:598\t" \
        "de:f:0.0352\trl:i:120\tcg:Z:200M2I300M5D100M1I49M\tcs:Z::200+ac:3"
    assert m.dv is None and abs(m.de - (1.0 - 630.0 / 653.0)) < 1e-15 and (m.ms, m.AS, m.nn, m.tp) == (1100, 1090, 1, "S")


def test_paf_line_inversion_and_split_records():
    import mappy_rs
    row = dict(CIGAR_ROW, is_primary=1, mapq=13, cs_len=-1, match_len=657, NM=0)
    inv, inv2, spl = records([row, dict(row, is_primary=0), row],
                             [dict(score=0, div=-1.0, rep_len=9, flags=1), dict(score=0, div=-1.0, rep_len=9, flags=1),
                              dict(score=300, div=np.float32(0.01), rep_len=9, flags=2 | 1 << 2)], chain_only=False, cigar=[657 << 4])
    assert mappy_rs.paf_line(inv, "q", 700).split("\t")[12:] == \
        ["NM:i:0", "ms:i:1100", "AS:i:1090", "nn:i:0", "tp:A:I", "cm:i:61", "s1:i:0", "s2:i:0", "de:f:0", "rl:i:9", "cg:Z:657M"]
    assert inv.tp == "I" and inv2.tp == "i" and inv.is_supplementary and inv.de == 0.0
    assert mappy_rs.paf_line(spl, "q", 700).split("\t")[12:] == \
        ["NM:i:0", "ms:i:1100", "AS:i:1090", "nn:i:0", "tp:A:P", "cm:i:61", "s1:i:300", "s2:i:0", "de:f:0", "zd:i:1", "rl:i:9", "cg:Z:657M"]
    assert spl.zd == 1 and not spl.is_supplementary


def test_records_without_tags_and_detach():
    import mappy_rs
    m, = records([CHAIN_ROW], None, chain_only=True)
    for k in ("s1", "s2", "cm", "ms", "AS", "nn", "rl", "zd", "dv", "de", "tp", "is_supplementary"):
        assert getattr(m, k) is None, k
    with pytest.raises(ValueError):
        mappy_rs.paf_line(m, "r", 5000)
    with pytest.raises(ValueError):
        mappy_rs.paf_line(mappy_rs.Mapping(0, 1000, 1, "Hello", 101010, 10, 1010, 1000, 1000, 60, True, [], 0, None, "Cigar string"), "r", 1000)
    a, = records([CIGAR_ROW], [dict(score=598, div=np.float32(0.04), rep_len=120, n_ambi=1, n_gap=8, n_gapo=3, flags=1 << 3)], chain_only=False,
                 cigar=CIG, sbuf=b":200+ac:3\0")
    b, = records([CIGAR_ROW], [dict(score=598, div=np.float32(0.04), rep_len=120, n_ambi=1, n_gap=8, n_gapo=3, flags=1 << 3)], chain_only=False,
                 cigar=CIG, sbuf=b":200+ac:3\0")
    before = [getattr(a, k) for k in ("s1", "s2", "cm", "ms", "AS", "nn", "rl", "zd", "dv", "de", "tp", "is_supplementary")]
    line = mappy_rs.paf_line(a, "q7", 700)
    b.detach()
    assert b._b is None and [getattr(b, k) for k in ("s1", "s2", "cm", "ms", "AS", "nn", "rl", "zd", "dv", "de", "tp", "is_supplementary")] == before
    assert before[7] == 2 and mappy_rs.paf_line(b, "q7", 700) == line and "\tzd:i:2\t" in line
    assert a == b and "s1" not in repr(a) and str(a) == str(b)       # FIELDS, __eq__, __repr__, __str__ do not know the tags


def test_tags_keyword(built, golden_dir):
    import mappy_rs
    from mappy_rs import _ffi
    mmi = os.path.join(golden_dir, "test.mmi")
    assert mappy_rs.Aligner(mmi)._tag_flag == 0
    al = mappy_rs.Aligner(mmi, tags=True)
    assert al._tag_flag == _ffi.OUT_TAGS == 4 and al._mo.flag == mappy_rs.Aligner(mmi)._mo.flag
    assert mappy_rs.Aligner(mmi, cigar=False, tags=True)._tag_flag == 4
    with pytest.raises(TypeError):
        mappy_rs.Aligner(mmi, None, None, None, None, None, None, None, None, 3, None, None, None, None, None, 0, None, True, True)   # keyword-only
    assert mappy_rs.Aligner(mmi).map_no_op("ACGT")[0].s1 is None
