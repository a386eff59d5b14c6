"""The long form of cs (minimap2 --cs=long: `=ACGT*ag+tt-c`) on the GPU: k_extra_long through its stage entry (mm355_stage_extra, want_cs bit 3)
on the census of tests/_cs_long.py, the whole mapping path with MM355_OUT_CS_LONG on the device walk and on the host walk (also under EQX),
the short form untouched, the PAF / SAM / BAM writers and the file writers, and the Python surface.  The truth is the oracle's write_cs_core,
mmo_cs_core(..., no_iden = 0, ...), on the hit's CIGAR, its query slice (reverse-complemented codes on '-') and the target codes."""
import ctypes as C
import gzip
import struct

import numpy as np
import pytest

from oracle import oracle as O
import synthdata as S
import _bam
import _cs_long as X
import _paf_sets as PS

pytestmark = pytest.mark.gpu

EQX = 0x4000000
_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def _codes(s):
    return _CODE[np.frombuffer(s.encode(), np.uint8)]


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    """a 260 kb contig with N runs; 60 ONT-like and 6 HiFi-like reads; the aligners and oracles of both presets; the oracle's records, once"""
    import mappy_rs
    td = tmp_path_factory.mktemp("cslong")
    g = S.make_genome(91, [260000], repeats=((3000, 4, 0.01), (600, 12, 0.03)), n_runs=2)
    fa = str(td / "ref.fa")
    S.write_fasta(fa, g, ["chrL"])
    reads, _ = S.make_reads(92, g, 60, n50=5000, lo=300)
    hifi, _ = S.make_reads(93, g, 6, n50=12000, lo=6000, sub=0.0005, ins=0.00075, dele=0.00075)      # error rate 0.002: match operations above 2048 columns
    w = dict(g=g, fa=fa, td=td, reads=reads, hifi=hifi,
             al=mappy_rs.Aligner(fa, preset="map-ont", tags=True), orc=O.OracleAligner(fa, preset="map-ont"),
             al_hifi=mappy_rs.Aligner(fa, preset="map-hifi", tags=True), orc_hifi=O.OracleAligner(fa, preset="map-hifi"))
    w["ref"] = [w["orc"].map(r, cs=True) for r in reads]
    w["ref_hifi"] = [w["orc_hifi"].map(r, cs=True) for r in hifi]
    return w


def _key(m):
    return (m.r_st, m.r_en, m.q_st, m.q_en, m.strand, m.mapq, m.cigar_str, m.mlen, m.blen, m.NM)


def _okey(o):
    return (o["target_start"], o["target_end"], o["query_start"], o["query_end"], o["strand"], o["mapq"], o["cigar_str"], o["match_len"], o["block_len"], o["NM"])


def _truth_of_hit(orc, read, m):
    """mmo_cs_core(no_iden = 0) on the hit's CIGAR, its query slice as U:format.c::get_seqs takes it, and the oracle index's target codes"""
    qc = _codes(read)
    if m.strand < 0:
        qc = np.where(qc < 4, 3 - qc, 4).astype(np.uint8)[::-1]
        q = qc[len(qc) - m.q_en:len(qc) - m.q_st]
    else:
        q = qc[m.q_st:m.q_en]
    t = _codes(orc.seq(m.ctg, m.r_st, m.r_en))
    ops = [(op, ln) for ln, op in m.cigar]
    assert X.t_len(ops) == len(t) and sum(ln for op, ln in ops if op in (0, 1, 7, 8)) == len(q)
    return X.truth(ops, np.ascontiguousarray(q), t)


def _stage(al, regions, want):
    """mm355_stage_extra on the regions -> [(mlen, blen, n_ambi, dp_max, cs, MD)]"""
    from mappy_rs import _ffi
    L = _ffi.lib()
    qcat = np.concatenate([q for _, _, _, q in regions] + [np.zeros(8, np.uint8)])
    cig = np.array([ln << 4 | op for _, _, ops, _ in regions for op, ln in ops] + [0], np.uint32)
    ja = (_ffi.ExtraJob * len(regions))()
    qo = co = 0
    for i, (_, t_st, ops, q) in enumerate(regions):
        ja[i].q_off, ja[i].cigar_off, ja[i].rid, ja[i].t_st, ja[i].n_cigar = qo, co, 0, t_st, len(ops)
        qo += len(q); co += len(ops)
    res = (_ffi.ExtraRes * len(regions))()
    cap = int(5 * (qcat.size + sum(ln for _, _, ops, _ in regions for op, ln in ops)) + 64 * len(cig))
    cs = np.zeros(cap, np.uint8)
    sr = al._stage_runner()
    try:
        _ffi.check(L.mm355_stage_extra(sr.ctx, C.byref(al._mo), len(regions), ja, qcat.ctypes.data, qcat.size, cig.ctypes.data, len(cig) - 1, want, res, cs.ctypes.data, cap))
    finally:
        sr.close()
    return [(r.mlen, r.blen, r.n_ambi, r.dp_max, bytes(cs[r.cs_off:r.cs_off + r.cs_len]).decode(), bytes(cs[r.md_off:r.md_off + r.md_len]).decode()) for r in res]


def test_stage_long_form_on_the_census(world):
    """want_cs 8, 9 (= long) and 8 | 2 (long + MD) on the census regions and 40 random ones: cs is the oracle's long form, MD and the four
    counts are update_extra_stage's; want_cs 3 on the same inputs is still the short form.  ('=' / 'X' operations never reach the device
    walk -- the stage entry refuses them --, so that census case is the host harness's and test_host_walk's.)"""
    al, G = world["al"], np.asarray(world["g"][0], np.uint8)
    rng = np.random.default_rng(4242)
    regions = X.census(rng, G, eqx=False) + X.random_regions(rng, G, 40)
    mo = al._mo
    exp, long_cs = [], []
    for _, t_st, ops, q in regions:
        t = G[t_st:t_st + X.t_len(ops) + 8]
        exp.append(O.update_extra_stage(q, t, ops, mo.a, mo.b, mo.sc_ambi, mo.q, mo.e))
        long_cs.append(X.truth(ops, q, t[:X.t_len(ops)]))
    assert max(len(s) for s in long_cs) > 12000 and sum(len(s) for s in long_cs) > 2 * sum(len(e[4]) for e in exp)
    for want in (8, 9, 8 | 2, 3):
        got = _stage(al, regions, want)
        for i, (reg, g, e) in enumerate(zip(regions, got, exp)):
            assert g[:4] == e[:4], (want, reg[0], g[:4], e[:4])
            want_cs = e[4] if want == 3 else long_cs[i]
            assert g[4] == want_cs, (want, reg[0], len(reg[2]), g[4][:80], want_cs[:80], len(g[4]), len(want_cs))
            assert g[5] == (e[5] if want & 2 else ""), (want, reg[0], g[5][:80], e[5][:80])


@pytest.fixture(scope="module")
def device_walk(world):
    """(ONT records, HiFi records) of mm355_map_batch with MM355_OUT_CS_LONG, the walk on the device (k_extra_long)"""
    from mappy_rs import _ffi
    mp = pytest.MonkeyPatch()
    mp.setenv("MM355_EXTRA_MIN_READS", "1")
    mp.delenv("MM355_EXTRA_HOST", raising=False)
    try:
        return world["al"]._map_many(world["reads"], _ffi.OUT_CS_LONG), world["al_hifi"]._map_many(world["hifi"], _ffi.OUT_CS_LONG)
    finally:
        mp.undo()


def test_whole_path_device_walk(world, device_walk):
    n_hits = n_long_ops = 0
    for recs, reads, ref, orc in ((device_walk[0], world["reads"], world["ref"], world["orc"]), (device_walk[1], world["hifi"], world["ref_hifi"], world["orc_hifi"])):
        for i, (ms, os_) in enumerate(zip(recs, ref)):
            assert [_key(m) for m in ms] == [_okey(o) for o in os_], i
            for m in ms:
                assert m.cs == _truth_of_hit(orc, reads[i], m), (i, m.cs[:80])
                assert m.MD is None
                n_hits += 1
                n_long_ops += sum(1 for ln, op in m.cigar if op == 0 and ln > X.SEG_COLS)
    assert n_hits >= 60 and n_long_ops >= 3      # HiFi-like reads: match operations that k_extra cuts


def test_host_walk_and_eqx(world, device_walk, monkeypatch):
    """MM355_EXTRA_HOST=1, one read at a time through Aligner.map(cs="long"): the records of the device walk; under MM_F_EQX the oracle's
    records and the long form of the '=' / 'X' CIGAR"""
    import mappy_rs
    monkeypatch.setenv("MM355_EXTRA_HOST", "1")
    for al, reads, dev in ((world["al"], world["reads"], device_walk[0]), (world["al_hifi"], world["hifi"], device_walk[1])):
        for i, r in enumerate(reads):
            host = al.map(r, cs="long")
            assert [_key(m) + (m.cs,) for m in host] == [_key(m) + (m.cs,) for m in dev[i]], i
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", extra_flags=EQX)
    orc = O.OracleAligner(world["fa"], preset="map-ont", extra_flags=EQX)
    n_hits = n_x = 0
    for i, r in enumerate(world["reads"][:30]):
        got, ref = al.map(r, cs="long"), orc.map(r)
        assert [_key(m) for m in got] == [_okey(o) for o in ref], i
        for m, d in zip(got, device_walk[0][i]):
            assert "M" not in m.cigar_str and m.cs == _truth_of_hit(orc, r, m) and m.cs == d.cs, i      # (runs end where 'X' begins: the string of the M CIGAR)
            n_hits += 1
            n_x += sum(1 for _, op in m.cigar if op == 8)
    assert n_hits >= 30 and n_x > 100


def test_short_form_untouched(world):
    al, reads = world["al"], world["reads"]
    names = ["r%d" % i for i in range(len(reads))]
    quals = ["I" * len(r) for r in reads]
    for fn, kw in ((al.map_paf, {}), (al.map_sam, dict(quals=quals)), (al.map_bam, dict(quals=quals))):
        a, b, c, d = (fn(reads, names=names, **kw, **cs) for cs in (dict(cs=True), dict(cs="short"), {}, dict(cs=False)))
        assert a == b and c == d and a != c and len(a) > len(c)
        assert (b"cs:Z::" in a or b"csZ:" in a) and b"cs:Z:=" not in a and b"csZ=" not in a and b"cs:Z" not in c and b"csZ" not in c
    n = 0
    for r, os_ in zip(reads, world["ref"]):
        for cs in (True, "short"):
            got = al.map(r, cs=cs)
            assert [m.cs for m in got] == [o["cs"] for o in os_]
        assert all(m.cs is None for m in al.map(r))
        n += len(os_)
    assert n >= 55


def _long_records(world):
    from mappy_rs import _ffi
    al, reads = world["al"], world["reads"]
    names = [None if i % 7 == 3 else "read%d comment" % i if i % 5 == 0 else "read%d" % i for i in range(len(reads))]
    quals = [None if i % 4 == 1 else "".join(chr(35 + (i + j) % 50) for j in range(len(r))) for i, r in enumerate(reads)]
    return names, quals, al._map_many(reads, _ffi.OUT_CS_LONG | _ffi.OUT_TAGS, names=names)


def test_writers(world):
    """map_paf / map_sam / map_bam with cs="long", formatted on the host and on the device: paf_line / sam_lines / record_of over the records"""
    import mappy_rs
    from mappy_rs import _ffi
    al, reads = world["al"], world["reads"]
    names, quals, recs = _long_records(world)
    for i, r in enumerate(reads):
        assert [m.cs for m in al.map(r, cs="long", name=names[i])] == [m.cs for m in recs[i]]
    paf = "".join(mappy_rs.paf_line(m, PS.printed_name(names[i]), len(reads[i])) + "\n" for i, ms in enumerate(recs) for m in ms).encode()
    sam = "".join(ln + "\n" for i, ms in enumerate(recs) if ms for ln in mappy_rs.sam_lines(ms, names[i], reads[i], quals[i])).encode()
    bam = _bam.frame(b"".join(_bam.record_of(ln, al.seq_names) for ln in sam.split(b"\n")[:-1]))
    assert paf.count(b"\tcs:Z:=") == paf.count(b"\n") >= 55 and sam.count(b"\tcs:Z:=") == sam.count(b"\n") >= 55
    for where, on in ((_ffi.PAF_HOST, False), (_ffi.PAF_DEVICE, True)):
        got = al.map_paf(reads, names=names, cs="long", where=where)
        assert al.paf_on_device is on and got == paf, (where, len(got), len(paf))
        got = al.map_sam(reads, names=names, quals=quals, cs="long", hit_only=True, where=where)
        assert al.paf_on_device is on and got == sam, (where, len(got), len(sam))
        got = al.map_bam(reads, names=names, quals=quals, cs="long", hit_only=True, where=where)
        assert al.paf_on_device is on and got == bam, (where, len(got), len(bam))


def _bam_cs_tags(path):
    data = gzip.decompress(open(path, "rb").read())
    assert data[:4] == b"BAM\1"
    at = 8 + struct.unpack_from("<I", data, 4)[0]
    n_ref = struct.unpack_from("<I", data, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 4 + struct.unpack_from("<I", data, at)[0] + 4
    out = []
    for rec in _bam.cut(data[at:]):
        k = rec.find(b"csZ")
        if k >= 0: out.append(rec[k + 3:rec.index(b"\0", k)].decode())
    return out


def test_file_writers(world):
    """map_file and map_bam_file(compress=True, sort=True) on a 64-read FASTQ in sub-batches of 7 reads: the long strings of map()"""
    from mappy_rs import _ffi
    al = world["al"]
    reads = (world["reads"] + world["hifi"])[:64]
    assert len(reads) == 64
    names = ["q%02d" % i for i in range(64)]
    fq = str(world["td"] / "reads.fq")
    with open(fq, "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % (n, r, "I" * len(r)) for n, r in zip(names, reads)))
    recs = al._map_many(reads, _ffi.OUT_CS_LONG | _ffi.OUT_TAGS, names=names)
    want = sorted(m.cs for ms in recs for m in ms)
    assert len(want) >= 60 and all(s.startswith("=") or s[0] in "*+-" for s in want)
    paf, bam = str(world["td"] / "out.paf"), str(world["td"] / "out.bam")
    r = al.map_file(fq, paf, cs="long", sub_batch_reads=7)
    assert r["n_reads"] == 64 and r["n_sub_batches"] >= 10
    text = open(paf, "rb").read()
    assert text == al.map_paf(reads, names=names, cs="long")
    assert sorted(f[5:] for ln in text.decode().split("\n") for f in ln.split("\t") if f.startswith("cs:Z:")) == want
    short = str(world["td"] / "short.paf")
    al.map_file(fq, short, cs=True, sub_batch_reads=7)
    assert open(short, "rb").read() == al.map_paf(reads, names=names, cs="short")
    r = al.map_bam_file(fq, bam, cs="long", sub_batch_reads=7, compress=True, sort=True, hit_only=True)
    assert r["n_reads"] == 64
    assert sorted(_bam_cs_tags(bam)) == want


def test_surface(world):
    import mappy_rs
    al, reads = world["al"], world["reads"][:12]
    for bad in ("LONG", 2, "", b"long", 1.5):
        for call in (lambda: al.map(reads[0], cs=bad), lambda: al.map_paf(reads[:2], cs=bad), lambda: al.map_sam(reads[:2], cs=bad),
                     lambda: al.map_bam(reads[:2], cs=bad), lambda: al.map_batch([{"seq": reads[0]}], cs=bad),
                     lambda: al.map_file("nowhere.fq", "nowhere.paf", cs=bad), lambda: al.map_bam_file("nowhere.fq", "nowhere.bam", cs=bad)):
            with pytest.raises(ValueError):
                call()
    chain = mappy_rs.Aligner(world["fa"], preset="map-ont", cigar=False)
    with pytest.raises(ValueError, match="base-level"):
        chain.map(reads[0], cs="long")
    with pytest.raises(ValueError, match="base-level"):
        chain.map_paf(reads[:2], cs="long")
    from mappy_rs import _ffi
    rc, hp = _ffi.call_map(chain._L, chain._context(), chain._mo, reads[:2], _ffi.OUT_CS_LONG)      # chain-only calls refuse it as they refuse MM355_OUT_CS
    assert rc == _ffi.MM355_EINVAL and not hp
    al.enable_threading(2)
    want_long = {i: [m.cs for m in al.map(r, cs="long")] for i, r in enumerate(reads)}
    want_short = {i: [m.cs for m in al.map(r, cs=True)] for i, r in enumerate(reads)}
    items = [{"seq": r, "i": i} for i, r in enumerate(reads)]
    assert {d["i"]: [m.cs for m in ms] for ms, d in al.map_batch(items, cs="long")} == want_long
    assert {d["i"]: [m.cs for m in ms] for ms, d in al.map_batch(items)} == want_short
    assert {d["i"]: [m.cs for m in ms] for ms, d in al.map_batch(items, cs="short")} == want_short
    assert all(m.cs is None for ms, d in al.map_batch(items, cs=False) for m in ms)
    assert want_long != want_short and all(s[0] in "=*+-" and ":" not in s for v in want_long.values() for s in v)
