"""Chain-only mapping (Aligner(cigar=False): no MM_F_CIGAR, minimap2's default output mode) on the CPU.

The public surface: the keyword clears MM_F_CIGAR and nothing else, cs / MD are refused up front.  The region stage: mm355_regs.h -- the header
k_regs (mappy-rs_amd/csrc/mm355_regs.hip) compiles for the device -- compiled for the host (tests/host_harness/regs_host.cpp, g++), fed the
oracle's sorted anchors and final chains of each read, must give the oracle's records of the same read mapped without MM_F_CIGAR, field
for field, over the long-read presets and the flags that change the region logic.  GPU side: tests/test_gpu_chain_only.py."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O
import _capi
import synthdata as S


ALL_CHAINS, HARD_MLEVEL, FOR_ONLY, REV_ONLY = 0x800000, 0x20000000, 0x100000, 0x200000
FIELDS = ("query_start", "query_end", "strand", "rid", "target_len", "target_start", "target_end", "match_len", "block_len", "mapq",
          "is_primary", "NM", "score0", "cnt", "n_sub", "subsc", "dp_max", "dp_max2", "dp_score")


@pytest.fixture(scope="module")
def regs_lib(built):
    L = _capi.build_harness("regs_host", ["-w", "-ffp-contract=off"], ["mm355_regs.h", "mm355_core.h"])
    L.regs_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_int32,
                            C.c_void_p, C.c_void_p]
    L.regs_host.restype = C.c_int
    return L


def _hit_dtype():
    from mappy_rs import _ffi
    return np.dtype([(k, np.dtype(t)) for k, t in _ffi.Hit._fields_], align=True)


def regs_records(L, orc, seq):
    """the read through the oracle's front (anchors, chains, long-join) and mm355_regs.h's tail; None when the header defers the read"""
    mo = orc.mo
    qlen = len(seq)
    if mo.max_qlen > 0 and qlen > mo.max_qlen:
        return []
    a, rep_len, mini_pos, _ = orc.anchors(seq, sorted_=True)
    if len(a) == 0:
        return []
    u, ca, _ = orc.chains_final(a, qlen)
    if len(u) == 0:
        return []
    opt_i = np.array([mo.flag, mo.mask_len, mo.best_n, orc.k * 2, int(mo.max_gap * 0.8), mo.min_chain_score, mo.seed], np.int64)
    opt_f = np.array([mo.mask_level, mo.pri_ratio], np.float32)
    seq_len = np.array(orc.seq_lens, np.uint32)
    u = np.ascontiguousarray(u, np.uint64); ca = np.ascontiguousarray(ca, np.uint64); mp = np.ascontiguousarray(mini_pos, np.uint64)
    dt = _hit_dtype()
    out = np.zeros(len(u), dt)
    n = L.regs_host(opt_i.ctypes.data, opt_f.ctypes.data, seq_len.ctypes.data, qlen, rep_len, len(u), u.ctypes.data, ca.ctypes.data,
                    len(mp), mp.ctypes.data, out.ctypes.data)
    if n < 0:
        return None
    recs = []
    for h in out[:n]:
        d = {k: int(h[k]) for k in FIELDS}
        d["is_primary"] = bool(d["is_primary"])
        d["cigar"], d["cs"], d["MD"] = ([] if h["n_cigar"] == 0 else None), (None if h["cs_len"] < 0 else ""), (None if h["md_len"] < 0 else "")
        recs.append(d)
    return recs


def oracle_records(orc, seq):
    return [{**{k: (h[k] if k != "is_primary" else bool(h[k])) for k in FIELDS}, "cigar": h["cigar"], "cs": h["cs"], "MD": h["MD"]}
            for h in orc.map(seq)]


DIV = 0.03   # the inverted copy: a reverse-strand chain under pri_ratio of the primary, above max_gap * 0.8
def _inverted_genome(seed):
    """random contigs plus a 30 kb block with a 6 %-diverged inverted copy 200 kb away: long reads of the block chain to both strands, the
    inverted copy scores below pri_ratio of the primary and above max_gap * 0.8 -- select_sub's strand_retained rule"""
    rng = np.random.default_rng(seed)
    g = S.make_genome(seed, [1500000, 900000], repeats=((5000, 40, 0.01), (2000, 60, 0.02), (300, 300, 0.05)))
    blk = g[0][100000:130000].copy()
    cp = S.mutate(blk, rng, DIV, 0.0, 0.0)[::-1]
    cp = np.where(cp < 4, 3 - cp, 4).astype(np.uint8)
    g[0][330000:330000 + len(cp)] = cp[:len(g[0]) - 330000]
    return g


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    td = tmp_path_factory.mktemp("chainonly")
    g = _inverted_genome(71)
    fa = str(td / "ref.fa")
    S.write_fasta(fa, g, ["chrA", "chrB"])
    reads, _ = S.make_reads(72, g, 180, n50=6000, lo=300)
    rng = np.random.default_rng(73)
    for st in (100000, 104000, 110000, 101500):
        reads.append(S.codes_to_str(S.mutate(g[0][st:st + 18000 + 2000 * (st % 3)], rng, 0.02, 0.01, 0.01)))
    reads += [reads[0][:14], "N" * 300, reads[1][:200] + "N" * 500 + reads[1][200:900]]
    return dict(fa=fa, g=g, reads=reads)


CASES = [("map-ont", {}), ("map-hifi", {}), ("map-pb", {}), ("asm5", {}), ("asm20", {}), ("ava-ont", {}),
         ("map-ont", {"extra_flags": ALL_CHAINS}), ("map-ont", {"extra_flags": HARD_MLEVEL}), ("map-ont", {"extra_flags": FOR_ONLY}),
         ("map-ont", {"extra_flags": REV_ONLY}), ("map-ont", {"best_n": 1, "min_cnt": 2, "min_chain_score": 20})]


@pytest.mark.parametrize("preset,kw", CASES, ids=["%s-%s" % (p, "-".join("%s=%s" % i for i in kw.items()) or "default") for p, kw in CASES])
def test_region_header_equals_oracle_chain_only(regs_lib, world, preset, kw):
    orc = O.OracleAligner(world["fa"], preset=preset, **kw)
    orc.mo.flag &= ~4
    n_hits = n_sec = n_deferred = 0
    for i, rd in enumerate(world["reads"]):
        exp = oracle_records(orc, rd)
        got = regs_records(regs_lib, orc, rd)
        if got is None:          # the pow / logf rules may send a read to the host; with glibc on both sides none should
            n_deferred += 1
            continue
        assert got == exp, (preset, kw, i)
        n_hits += len(exp); n_sec += sum(not h["is_primary"] for h in exp)
    assert n_deferred == 0
    assert n_hits > 100, n_hits
    if not kw.get("extra_flags") == ALL_CHAINS and preset.startswith("map"):
        assert n_sec > 0


def test_strand_retained_regions_are_reached(regs_lib, world):
    """the long reads of the inverted block: besides the primary chain they have a reverse-strand chain under pri_ratio of it and above
    max_gap * 0.8 -- select_sub keeps it only through its strand rule, and filter_strand_retained's divergence comparison decides -- and the
    records still equal the oracle's"""
    orc = O.OracleAligner(world["fa"], preset="map-ont")
    orc.mo.flag &= ~4
    n_reached = 0
    for rd in world["reads"][180:184]:
        assert regs_records(regs_lib, orc, rd) == oracle_records(orc, rd)
        a, _, _, _ = orc.anchors(rd, sorted_=True)
        u, ca, _ = orc.chains_final(a, len(rd))
        first = np.concatenate(([0], np.cumsum(u & np.uint64(0xffffffff))[:-1])).astype(np.int64)
        sc = (u >> np.uint64(32)).astype(np.int64)
        rev = (ca[first, 0] >> np.uint64(63)).astype(np.int64)
        top = int(np.argmax(sc))
        n_reached += int(((rev != rev[top]) & (sc > int(orc.mo.max_gap * 0.8)) & (sc < sc[top] * orc.mo.pri_ratio)).sum())
    assert n_reached >= 4


def test_gen_regs_ties_take_the_higher_index_first(regs_lib, world):
    """two chains with the same score and count whose first anchor is the same: their gen_regs keys (score << 32 | cnt ^ hash) are equal, and
    radix_sort_128x + reversal put the LATER chain first.  ALL_CHAINS keeps the gen_regs order in the records."""
    orc = O.OracleAligner(world["fa"], preset="map-ont", extra_flags=ALL_CHAINS)
    orc.mo.flag &= ~4
    span = 15
    a0 = [(100 + 10 * i, 50 + 10 * i) for i in range(6)]
    a1 = a0[:1] + [(100 + 12 * i, 50 + 10 * i) for i in range(1, 6)]       # same first anchor, other target spacing
    anchors = np.array([(x, span << 32 | y) for x, y in a0 + a1], np.uint64)
    u = np.array([(40 << 32) | 6, (40 << 32) | 6], np.uint64)
    mp = np.array(sorted(set((span << 32) | y for _, y in a0 + a1)), np.uint64)
    opt_i = np.array([orc.mo.flag, orc.mo.mask_len, orc.mo.best_n, orc.k * 2, 4000, orc.mo.min_chain_score, orc.mo.seed], np.int64)
    opt_f = np.array([orc.mo.mask_level, orc.mo.pri_ratio], np.float32)
    seq_len = np.array(orc.seq_lens, np.uint32)
    out = np.zeros(2, _hit_dtype())
    n = regs_lib.regs_host(opt_i.ctypes.data, opt_f.ctypes.data, seq_len.ctypes.data, 400, 0, 2, u.ctypes.data, anchors.ctypes.data,
                           len(mp), mp.ctypes.data, out.ctypes.data)
    assert n == 2
    assert [int(h["target_end"]) for h in out] == [a1[-1][0] + 1, a0[-1][0] + 1]


# ---------------------------------------------------------------- public surface (no device needed)
def _ffi_ok():
    try:
        from mappy_rs import _ffi
        _ffi.lib()
        return True
    except Exception:
        return False


@pytest.fixture(scope="module")
def mappy(built):
    import mappy_rs
    assert _ffi_ok()
    return mappy_rs


def test_cigar_keyword_sets_and_clears_flag_4(mappy, golden_dir):
    mmi = os.path.join(golden_dir, "test.mmi")
    assert mappy.Aligner(mmi)._mo.flag & 4
    assert mappy.Aligner(mmi, cigar=True)._mo.flag & 4
    al = mappy.Aligner(mmi, cigar=False)
    assert not al._mo.flag & 4
    ref = mappy.Aligner(mmi)
    assert al._mo.flag == ref._mo.flag & ~4
    for k, _t in al._mo._fields_:
        if k != "flag":
            assert getattr(al._mo, k) == getattr(ref._mo, k), k
    pb = mappy.Aligner(mmi, preset="map-pb", cigar=False, extra_flags=ALL_CHAINS, scoring=(1, 2, 2, 1))
    assert not pb._mo.flag & 4 and pb._mo.flag & ALL_CHAINS and pb._mo.a == 1


def test_cs_and_md_are_refused_without_cigar(mappy, golden_dir):
    al = mappy.Aligner(os.path.join(golden_dir, "test.mmi"), cigar=False)
    with pytest.raises(ValueError):
        al.map("ACGT" * 50, cs=True)
    with pytest.raises(ValueError):
        al.map("ACGT" * 50, MD=True)


def test_chain_only_mapping_view(mappy):
    """a chain-only hit row (n_cigar 0, cs / md -1, NULL CIGAR arena): empty CIGAR, NM 0, no cs / MD, no cg:Z: field"""
    from mappy_rs import _ffi
    dt = _hit_dtype()
    row = np.zeros(1, dt)
    row[0]["query_end"], row[0]["strand"], row[0]["target_len"], row[0]["target_end"] = 394, 1, 1000, 394
    row[0]["match_len"], row[0]["block_len"], row[0]["mapq"], row[0]["is_primary"] = 393, 393, 60, 1
    row[0]["cs_len"] = row[0]["md_len"] = -1
    buf = C.create_string_buffer(row.tobytes(), dt.itemsize)
    off = (C.c_int64 * 2)(0, 1)
    st = (C.c_int32 * 1)(0)
    h = _ffi.Hits(n_reads=1, hit_off=off, status=st, hits=C.cast(buf, C.POINTER(_ffi.Hit)), cigar=None, str=None, n_hits=1, n_cigar=0, n_str=0)
    out = mappy._batch_to_mappings(C.pointer(h), 1, ["ctg"], chain_only=True)
    m = out[0][0]
    assert m.cigar == [] and m.cigar_str == "" and m.NM == 0 and m.cs is None and m.MD is None
    assert m.mlen == m.blen == 393 and m.mapq == 60 and m.is_primary and m.ctg == "ctg"
    assert "cg:Z:" not in str(m) and str(m).endswith("tp:A:P")
