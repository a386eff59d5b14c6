"""minimap2's PAF tags on the GPU (MM355_OUT_TAGS, Aligner(tags=True)): every field of every mm355_tags_t row equals what the oracle's
mm_reg1_t / mm_extra_t of the same region holds (tests/_tags_truth.py; div bit for bit) -- chain-only through k_regs and through the host
path, CIGAR mode through the device walk (k_extra) and the host walk, with inversion records, split regions and ambiguous bases; the
gap counters of mm355_stage_extra; a request for tags changes no byte of the other outputs; the Python properties and paf_line.
CPU side: tests/test_tags_host.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import synthdata as S
from test_chain_only_host import ALL_CHAINS, _inverted_genome
import _tags_truth as T
import _capi
from _capi import pair, stats

OUT_CS, OUT_TAGS = 1, 4


def map_raw(al, reads, flags):
    """one mm355_map_batch call: (per-read list of (hit dict, tags tuple or None), raw bytes of hits / cigar / str, whether tags came back)"""
    v = _capi.map_raw(al, reads, flags)
    rows, tg, has_tags = v.hits, v.tags, v.tags is not None
    out = []
    for i in range(len(reads)):
        one = []
        for j in range(v.off[i], v.off[i + 1]):
            hd = {k: int(rows[j][k]) for k in T.HIT_FIELDS}
            tt = None
            if has_tags:
                t = tg[j]
                assert int(t["reserved"]) == 0 and int(t["flags"]) >> 4 == 0
                fl = int(t["flags"])
                tt = (int(t["score"]), T.f32_bits(t["div"]), int(t["rep_len"]), int(t["n_ambi"]), int(t["n_gap"]), int(t["n_gapo"]),
                      fl & 1, fl >> 1 & 1, fl >> 2 & 3)
            one.append((hd, tt))
        out.append(one)
    return out, (_capi.raw(v.hits), v.cigar.tobytes(), v.str), has_tags


def expected(orc, rd):
    return [({k: e[k] for k in T.HIT_FIELDS}, T.tags_tuple(e)) for e in T.oracle_tags(orc, rd)]


def _rc(c):
    return np.where(c < 4, 3 - c, 4).astype(np.uint8)[::-1]


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    td = tmp_path_factory.mktemp("gtags")
    g = _inverted_genome(71)
    fa = str(td / "ref.fa")
    S.write_fasta(fa, g, ["chrA", "chrB"])
    # chain-only: the world of tests/test_gpu_chain_only.py plus unmutated reads that reach a contig's end (div == 0, tests/test_tags_host.py)
    reads, _ = S.make_reads(81, g, 300, n50=6000, lo=300)
    rng = np.random.default_rng(82)
    for st in (100000, 104000, 110000, 101500):
        reads.append(S.codes_to_str(S.mutate(g[0][st:st + 18000], rng, 0.02, 0.01, 0.01)))
    reads += [S.codes_to_str(g[0][700000:703000]), S.codes_to_str(g[1][-2000:]), S.codes_to_str(g[0][-3000:]), S.codes_to_str(_rc(g[0][-4000:]))]
    # CIGAR mode: 8-kb reads whose middle 300 / 600 / 1200 bases are reverse-complemented (the extension z-drops there: the region is split
    # and the gap between the halves is aligned as an inversion record), 60 ordinary reads, three 6-kb reads with four Ns each
    inv = []
    for o in (20000, 60000, 150000):
        for ln in (300, 600, 1200):
            inv.append(np.concatenate([g[0][o:o + 4000], _rc(g[0][o + 4000:o + 4000 + ln]), g[0][o + 4000 + ln:o + 8000]]))
    rng = np.random.default_rng(7)
    inv_ont = [S.codes_to_str(S.mutate(c, rng, 0.004, 0.003, 0.003)) for c in inv]      # map-ont: 1 % errors
    plain, _ = S.make_reads(77, g, 60, n50=5000, lo=300)
    ambi = []
    for o in (300000, 700000, 1000000):
        c = g[0][o:o + 6000].copy()
        c[[1000, 2500, 2501, 4800]] = 4
        ambi.append(S.codes_to_str(c))
    return dict(fa=fa, g=g, reads=reads, cigar_reads={True: inv_ont + plain + ambi, False: [S.codes_to_str(c) for c in inv] + plain + ambi})


CASES = [("map-ont", {}), ("map-hifi", {}), ("asm20", {}), ("ava-ont", {}), ("map-ont", {"extra_flags": ALL_CHAINS})]
IDS = ["%s-%s" % (p, "all_chains" if kw else "default") for p, kw in CASES]


@pytest.mark.parametrize("preset,kw", CASES, ids=IDS)
def test_chain_only_tags_parity(world, monkeypatch, preset, kw):
    al, orc = pair(world["fa"], preset, False, **kw)
    reads = world["reads"]
    off, raw_off, has = map_raw(al, reads, 0)
    assert not has                                         # flag off: hits->tags == NULL
    n_host_off = stats(al).n_regs_host
    on, raw_on, has = map_raw(al, reads, OUT_TAGS)
    assert has and raw_on == raw_off                       # ... and the other outputs are byte-identical with the flag on
    st = stats(al)
    assert st.n_regs_dev > 0
    # a region's divergence is unsure with probability ~ 2^-23 pw / (1 - pw), ~ 2e-6 at 5 % divergence: the stricter rule defers (almost) nobody
    assert n_host_off <= st.n_regs_host <= n_host_off + len(reads) // 100, (n_host_off, st.n_regs_host)
    n_hits = n_zero = 0
    for i, rd in enumerate(reads):
        exp = expected(orc, rd)
        assert on[i] == exp, (preset, i, on[i], exp)
        n_hits += len(exp); n_zero += sum(t[1] == 0 for _, t in exp)
    assert n_hits > 250 and n_zero >= 2
    monkeypatch.setenv("MM355_REGS_HOST", "1")
    host, raw_host, has = map_raw(al, reads, OUT_TAGS)
    st2 = stats(al)
    assert has and st2.n_regs_dev == 0 and st2.n_regs_host > 0
    assert host == on and raw_host == raw_on


def test_chain_only_deferred_reads_carry_their_tags(world, monkeypatch):
    """reads k_regs defers (logf table cut short) are finished on the host: the merge in read order carries the tags rows with the hit rows"""
    al, orc = pair(world["fa"], "map-ont", False)
    monkeypatch.setenv("MM355_REGS_LOGT_N", "2500")
    on, _, has = map_raw(al, world["reads"], OUT_TAGS)
    st = stats(al)
    assert has and st.n_regs_dev > 20 and st.n_regs_host > 20
    for i, rd in enumerate(world["reads"]):
        assert on[i] == expected(orc, rd), i


@pytest.mark.parametrize("preset", ["map-ont", "map-hifi", "asm20"])
def test_cigar_mode_tags_parity(world, monkeypatch, preset):
    """every tags field of every record, inversion records and split regions included, through the device walk and the host walk"""
    al, orc = pair(world["fa"], preset, True)
    reads = world["cigar_reads"][preset == "map-ont"]
    exp = [expected(orc, rd) for rd in reads]
    flat = [t for e in exp for _, t in e]
    hits = [h for e in exp for h, _ in e]
    # what the oracle holds on these reads: 9 inversion records, 18 split regions whose score differs from score0, 3 records with Ns
    assert sum(t[6] for t in flat) == 9 and sum(t[8] != 0 for t in flat) == 18
    assert sum(t[0] != h["score0"] for h, t in zip(hits, flat)) == 18 and sum(t[3] > 0 for t in flat) == 3
    assert sum(t[5] > 0 for t in flat) > 50 and any(t[7] == 0 and h["is_primary"] for h, t in zip(hits, flat))      # gaps; supplementary records
    off, raw_off, has = map_raw(al, reads, OUT_CS)
    assert not has
    dev, raw_dev, has = map_raw(al, reads, OUT_CS | OUT_TAGS)
    assert has and raw_dev == raw_off                      # hit rows, CIGAR words and the string arena do not change with the request
    for i in range(len(reads)):
        assert dev[i] == exp[i], (preset, i, dev[i], exp[i])
    monkeypatch.setenv("MM355_EXTRA_HOST", "1")
    host, raw_host, has = map_raw(al, reads, OUT_CS | OUT_TAGS)
    assert has and host == dev and raw_host == raw_dev


def test_stage_extra_gap_counts(world):
    """k_extra's I / D counters through the stage entry (want_cs bit 2) against a count in Python: a match operation cut between lanes, gaps
    that get a segment of their own, gaps on both sides of a segment border, leading and trailing gaps, more than one segment of operations"""
    import mappy_rs
    from mappy_rs import _ffi
    al = mappy_rs.Aligner(world["fa"], preset="map-ont")
    L = al._L
    rng = np.random.default_rng(3)
    t_all = np.asarray(world["g"][0], np.uint8)
    alt = lambda n, first_gap=False: [((1 + (k // 2) % 2, 1 + k % 5) if (k % 2 == 1) != first_gap else (0, 3 + k % 11)) for k in range(n)]
    border = alt(63) + [(1, 4), (2, 9)] + alt(40)                                   # operations 64 and 65 are gaps
    assert [op for op, _ in border[62:66]] == [0, 1, 2, 0]
    cases = [[(0, 3000)], [(0, 5000)], [(0, 100), (2, 2500), (0, 100), (1, 2500), (0, 100)], border, [(1, 5), (0, 50), (2, 7)],
             [(2, 3), (0, 40), (1, 4)], alt(300), alt(129, first_gap=True), [(0, 7)], [(1, 700), (0, 2048), (2, 1)]]
    qs, jobs = [], []
    for i, ops in enumerate(cases):
        t_st, to, q = 5000 + 40000 * i, 0, []
        for op, ln in ops:
            if op == 0:
                q.append(t_all[t_st + to:t_st + to + ln].copy()); to += ln
            elif op == 1:
                q.append(S.random_codes(rng, ln).astype(np.uint8))
            else:
                to += ln
        qs.append(np.concatenate(q).astype(np.uint8)); jobs.append(t_st)
    qcat = np.concatenate(qs + [np.zeros(8, np.uint8)])
    cig = np.array([ln << 4 | op for ops in cases for op, ln in ops] + [0], np.uint32)
    ja = (_ffi.ExtraJob * len(cases))()
    qo = co = 0
    for i, ops in enumerate(cases):
        ja[i].q_off, ja[i].cigar_off, ja[i].rid, ja[i].t_st, ja[i].n_cigar = qo, co, 0, jobs[i], len(ops)
        qo += len(qs[i]); co += len(ops)
    cap = int(5 * (qcat.size + sum(ln for ops in cases for _, ln in ops)) + 64 * len(cig))
    cs = np.zeros(cap, np.uint8)
    sr = al._stage_runner()
    res = {}
    for want in (4, 7, 3, 0):
        r = (_ffi.ExtraRes * len(cases))()
        _ffi.check(L.mm355_stage_extra(sr.ctx, C.byref(al._mo), len(cases), ja, qcat.ctypes.data, qcat.size, cig.ctypes.data, len(cig) - 1, want, r,
                                       cs.ctypes.data, cap))
        res[want] = [(x.mlen, x.blen, x.n_ambi, x.dp_max, x.pad, x.pad2) for x in r]
    sr.close()
    for i, ops in enumerate(cases):
        n_gap, n_gapo = T.gap_counts([ln << 4 | op for op, ln in ops])
        assert res[4][i][4:] == (n_gapo, n_gap) == res[7][i][4:], (i, res[4][i], n_gapo, n_gap)
        assert res[3][i][4:] == (0, 0) == res[0][i][4:]                              # bit clear: both words stay 0
        assert res[4][i][:4] == res[7][i][:4] == res[3][i][:4] == res[0][i][:4]
        assert res[4][i][0] == sum(ln for op, ln in ops if op == 0)                 # (the walk itself ran: every match column matches)


TAG_PROPS = ("s1", "s2", "cm", "ms", "AS", "nn", "rl", "zd", "dv", "de", "tp", "is_supplementary")


def _prop_truth(e, cigar):
    tp = ("I" if e["inv"] else "P") if e["is_primary"] else ("i" if e["inv"] else "S")
    de = 1.0 - float(e["match_len"]) / (e["block_len"] + e["n_ambi"] - e["n_gap"] + e["n_gapo"]) if cigar else None
    dv = None if cigar or not 0.0 <= e["div"] <= 1.0 else e["div"]
    return (e["score"], e["subsc"], e["cnt"], e["dp_max"], e["dp_score"], e["n_ambi"], e["rep_len"], e["split"], dv, de, tp,
            bool(e["is_primary"] and not e["sam_pri"]))


@pytest.mark.parametrize("cigar", [True, False], ids=["cigar", "chain_only"])
def test_python_tags_surface(world, cigar):
    import mappy_rs
    fa = world["fa"]
    reads = (world["cigar_reads"][True][:9] + world["cigar_reads"][True][9:29]) if cigar else world["reads"][:40] + world["reads"][-4:]
    al = mappy_rs.Aligner(fa, preset="map-ont", cigar=cigar, tags=True, devices=[0])
    plain = mappy_rs.Aligner(fa, preset="map-ont", cigar=cigar)
    orc = O.OracleAligner(fa, preset="map-ont")
    if not cigar:
        orc.mo.flag &= ~4
    n = n_dv = 0
    one = []
    for k, rd in enumerate(reads):
        ms = al.map(rd, cs=True) if cigar else al.map(rd)
        one.append(ms)
        exp = T.oracle_tags(orc, rd)
        assert len(ms) == len(exp)
        for m, e in zip(ms, exp):
            want = _prop_truth(e, cigar)
            assert tuple(getattr(m, p) for p in TAG_PROPS) == want, (k, want)
            line = mappy_rs.paf_line(m, "read%d" % k, len(rd))
            cols = line.split("\t")
            assert cols[:12] == [str(x) for x in ("read%d" % k, len(rd), m.q_st, m.q_en, "+" if m.strand > 0 else "-", m.ctg, m.ctg_len, m.r_st,
                                                  m.r_en, m.mlen, m.blen, m.mapq)]
            tags = dict((c[:2], c[5:]) for c in cols[12:])
            assert tags["tp"] == m.tp and int(tags["cm"]) == m.cm and int(tags["s1"]) == m.s1 and int(tags["rl"]) == m.rl
            assert ("s2" in tags) == m.is_primary and ("zd" in tags) == bool(m.zd)
            if cigar:
                assert tags["cg"] == m.cigar_str and tags["cs"] == m.cs and int(tags["NM"]) == m.NM and "dv" not in tags
                assert tags["de"] == ("0" if m.de == 0.0 else "%.4f" % m.de)
            else:
                assert "cg" not in tags and "de" not in tags and "NM" not in tags
                assert tags.get("dv") == (None if m.dv is None else "0" if m.dv == 0.0 else "%.4f" % m.dv)
                n_dv += m.dv is not None
            kept = tuple(getattr(m.detach(), p) for p in TAG_PROPS)
            assert kept == want and m._b is None and mappy_rs.paf_line(m, "read%d" % k, len(rd)) == line
            n += 1
    assert n > 30 and (cigar or n_dv > 30)
    for m in plain.map(reads[0]):
        assert all(getattr(m, p) is None for p in TAG_PROPS)
        with pytest.raises(ValueError):
            mappy_rs.paf_line(m, "r", len(reads[0]))
    assert plain.map(reads[0], cs=cigar) == one[0]                   # __eq__ compares Mapping.FIELDS only
    al.enable_threading(2)
    out = list(al.map_batch([{"seq": r, "id": i} for i, r in enumerate(reads)]))
    by_id = {d["id"]: ms for ms, d in out}
    assert sorted(by_id) == list(range(len(reads)))
    for i in range(len(reads)):
        assert [tuple(getattr(m, p) for p in TAG_PROPS) for m in by_id[i]] == [tuple(getattr(m, p) for p in TAG_PROPS) for m in one[i]]
        assert by_id[i] == one[i]
