"""Chain-only mapping on the GPU (Aligner(cigar=False), mm355_map_batch without MM_F_CIGAR): the region stage k_regs
(mappy-rs_amd/csrc/mm355_regs.hip) and its host path give the oracle's records of the same reads mapped without MM_F_CIGAR, every field of
the C-ABI row; the host switch gives the same rows; a read's hits do not depend on its batch; map_batch / devices work; an index without
sequence maps.  CPU side: tests/test_chain_only_host.py."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import synthdata as S
import _capi
from _capi import stats
from test_chain_only_host import ALL_CHAINS, HARD_MLEVEL, FOR_ONLY, REV_ONLY, _inverted_genome

ROW = ("query_start", "query_end", "strand", "rid", "target_len", "target_start", "target_end", "match_len", "block_len", "mapq",
       "is_primary", "NM", "score0", "cnt", "n_sub", "subsc", "dp_max", "dp_max2", "dp_score", "n_cigar", "cs_len", "md_len")


def map_rows(al, reads):
    """reads through mm355_map_batch on the Aligner's context: per read, a list of row tuples (ROW fields) or the status code"""
    v = _capi.map_raw(al, reads, 0)
    assert len(v.cigar) == 0 and len(v.str) == 0              # n_cigar == 0 and n_str == 0
    off, st, rows = v.off, v.status, v.hits
    out = []
    for i in range(len(reads)):
        if st[i] != 0:
            out.append(int(st[i]))
        else:
            out.append([tuple(int(x[k]) for k in ROW) for x in rows[off[i]:off[i + 1]]])
    return out


def oracle_rows(orc, rd):
    if len(rd) == 0:
        return _ffi_code("MM355_EEMPTY")
    return [tuple(int(h[k]) for k in ROW[:19]) + (0, -1, -1) for h in orc.map(rd)]


def _ffi_code(name):
    from mappy_rs import _ffi
    return getattr(_ffi, name)


def check(al, orc, reads):
    got = map_rows(al, reads)
    n_hits = n_sec = 0
    for i, rd in enumerate(reads):
        exp = oracle_rows(orc, rd)
        assert got[i] == exp, (i, got[i], exp)
        if isinstance(exp, list):
            n_hits += len(exp); n_sec += sum(not r[10] for r in exp)
    return n_hits, n_sec


@pytest.fixture(scope="module")
def world(built, tmp_path_factory):
    td = tmp_path_factory.mktemp("gco")
    g = _inverted_genome(71)
    fa = str(td / "ref.fa")
    S.write_fasta(fa, g, ["chrA", "chrB"])
    reads, _ = S.make_reads(81, g, 300, n50=6000, lo=300)
    rng = np.random.default_rng(82)
    for st in (100000, 104000, 110000, 101500):
        reads.append(S.codes_to_str(S.mutate(g[0][st:st + 18000], rng, 0.02, 0.01, 0.01)))
    return dict(fa=fa, g=g, reads=reads)


def pair(fa, preset, **kw):
    return _capi.pair(fa, preset, False, **kw)


CASES = [("map-ont", {}), ("map-hifi", {}), ("map-pb", {}), ("asm5", {}), ("asm20", {}), ("ava-ont", {}),
         ("map-ont", {"extra_flags": ALL_CHAINS}), ("map-ont", {"extra_flags": HARD_MLEVEL}), ("map-ont", {"extra_flags": FOR_ONLY}),
         ("map-ont", {"extra_flags": REV_ONLY}), ("map-ont", {"best_n": 1}), ("map-ont", {"min_cnt": 2, "min_chain_score": 20}),
         ("map-pb", {"best_n": 2, "min_chain_score": 60})]


@pytest.mark.parametrize("preset,kw", CASES, ids=["%s-%s" % (p, "-".join("%s=%s" % i for i in kw.items()) or "default") for p, kw in CASES])
def test_chain_only_parity(world, preset, kw):
    al, orc = pair(world["fa"], preset, **kw)
    n_hits, n_sec = check(al, orc, world["reads"])
    assert n_hits > 250
    if preset.startswith("map") and kw.get("extra_flags") != ALL_CHAINS:
        assert n_sec > 0
    st = stats(al)
    assert st.n_regs_dev > 0, (st.n_regs_dev, st.n_regs_host)     # k_regs made rows of this case, whatever the host path took


def test_chain_only_mapping_records(world):
    """the Python surface of a chain-only hit: empty CIGAR, NM 0, no cs / MD, no cg:Z: field; cs / MD requests refused"""
    al, orc = pair(world["fa"], "map-ont")
    rd = world["reads"][-1]
    ms = al.map(rd)
    exp = orc.map(rd)
    assert len(ms) == len(exp) > 0
    for m, e in zip(ms, exp):
        assert (m.ctg, m.r_st, m.r_en, m.q_st, m.q_en, m.strand, m.mlen, m.blen, m.mapq, m.is_primary) == \
            (e["target_name"], e["target_start"], e["target_end"], e["query_start"], e["query_end"], e["strand"], e["match_len"],
             e["block_len"], e["mapq"], e["is_primary"])
        assert m.cigar == [] and m.cigar_str == "" and m.NM == 0 and m.cs is None and m.MD is None and "cg:Z:" not in str(m)
    with pytest.raises(ValueError):
        al.map(rd, cs=True)
    from mappy_rs import _ffi
    for fl in (_ffi.OUT_CS, _ffi.OUT_MD):
        assert _capi.map_raw(al, [rd], fl, raise_on_error=False) == (_ffi.MM355_EINVAL, None)


def test_chain_only_edge_reads(world):
    al, orc = pair(world["fa"], "map-ont")
    g = world["g"]
    rng = np.random.default_rng(5)
    base = world["reads"][3]
    iupac = "".join("RYKMSWN"[i % 7] if i % 37 == 0 else c for i, c in enumerate(base))
    long1 = S.codes_to_str(S.mutate(g[0][200000:380000], rng, 0.02, 0.01, 0.01))
    long2 = S.codes_to_str(S.mutate(np.concatenate([g[0][:600000], g[1][:400000]]), rng, 0.01, 0.005, 0.005))
    reads = ["", "ACGTACGTAC", base[:14], "N" * 2000, base[:300] + "N" * 1500 + base[300:2000], iupac, base, base, long1, long2]
    check(al, orc, reads)
    with pytest.raises(RuntimeError):
        al.map("")
    al.enable_threading(2)
    al2, orc2 = pair(world["fa"], "map-ont")
    al2._mo.max_qlen = orc2.mo.max_qlen = 5000
    check(al2, orc2, [r for r in world["reads"][:40]])


def test_chain_only_human_repeats(built, tmp_path):
    """repeat-rich reads on the mid-scale human-like genome: many chains per read, all rows equal the oracle's"""
    g, names = S.make_human_like(3, 0.05)
    fa = str(tmp_path / "h.fa")
    S.write_fasta(fa, g, names)
    reads, _ = S.make_reads(91, g, 150, n50=12000, lo=500)
    for preset in ("map-ont", "map-hifi"):
        al, orc = pair(fa, preset)
        n_hits, n_sec = check(al, orc, reads)
        assert n_hits > 100


def test_host_switch_gives_the_same_rows(world, monkeypatch):
    al, _ = pair(world["fa"], "map-ont")
    dev = map_rows(al, world["reads"])
    st = stats(al)
    assert st.n_regs_dev > 0 and st.n_regs_host == 0
    monkeypatch.setenv("MM355_REGS_HOST", "1")
    host = map_rows(al, world["reads"])
    st2 = stats(al)
    assert st2.n_regs_dev == 0 and st2.n_regs_host > 0
    assert host == dev


def test_deferred_reads_merge_in_read_order(world, monkeypatch):
    """MM355_REGS_LOGT_N shrinks the device's logf table: reads whose primary chain scores beyond it are deferred by k_regs and finished on
    the host, the others stay on the device; the merged rows equal the oracle's in read order"""
    al, orc = pair(world["fa"], "map-ont")
    monkeypatch.setenv("MM355_REGS_LOGT_N", "2500")
    check(al, orc, world["reads"])
    st = stats(al)
    assert st.n_regs_dev > 20 and st.n_regs_host > 20, (st.n_regs_dev, st.n_regs_host)


def test_hits_do_not_depend_on_the_batch(world):
    al, _ = pair(world["fa"], "map-ont")
    reads = world["reads"][:120]
    whole = map_rows(al, reads)
    parts = []
    for lo, hi in ((0, 1), (1, 37), (37, 120)):
        parts += map_rows(al, reads[lo:hi])
    assert parts == whole
    rev = map_rows(al, reads[::-1])[::-1]
    assert rev == whole


def test_map_batch_and_devices_in_chain_only_mode(world):
    import mappy_rs
    reads = world["reads"]
    al = mappy_rs.Aligner(world["fa"], preset="map-ont", cigar=False, devices=[0])
    one = [al.map(r) for r in reads[:50]]
    al.enable_threading(2)
    items = [{"seq": r, "id": i} for i, r in enumerate(reads)]
    out = list(al.map_batch(iter(items)))
    assert sorted(d["id"] for _, d in out) == list(range(len(items)))
    by_id = {d["id"]: ms for ms, d in out}
    for i in range(50):
        assert by_id[i] == one[i]
        assert all(m.cs is None and m.cigar == [] for m in by_id[i])


def test_no_seq_index_maps_chain_only(built, golden_dir, tmp_path):
    import mappy_rs
    from test_oracle_golden import ENTERO
    mmi = bytearray(open(os.path.join(golden_dir, "test.mmi"), "rb").read())
    mmi[20:24] = (2).to_bytes(4, "little")
    f = tmp_path / "noseq.mmi"; f.write_bytes(bytes(mmi[:-((4 * 400 + 7) // 8 * 4)]))
    al = mappy_rs.Aligner(str(f), cigar=False)
    orc = O.OracleAligner(os.path.join(golden_dir, "test.mmi"))
    orc.mo.flag &= ~4
    got = map_rows(al, [ENTERO])[0]
    assert got == oracle_rows(orc, ENTERO) and len(got) == 1
    assert got[0][7:10] == (393, 393, 60)
    with pytest.raises(RuntimeError):
        mappy_rs.Aligner(str(f)).map(ENTERO)
