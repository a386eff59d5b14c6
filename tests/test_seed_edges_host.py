"""The inputs of tests/test_gpu_seed_edges.py reach what they are there for -- asserted on the CPU, with the oracle and the plain model of
tests/_seed_census.py only, so that the GPU tests cannot quietly stop reaching a branch -- and the host's flat table (mm355_index_get) on the
genome whose table wraps.

Why these inputs exist.  The census of the inputs the suite had before them (`python tests/_seed_census.py` prints this table: it rebuilds the
reads of four older tests from their seeds, builds the oracle's index with the map-ont preset, and runs select_census over every read and
Table over the index's keys; CPU only, a few seconds):

| input | reads | mid_occ | table lines | load | carry into line 0 | streaks | none | all | heap | clamp | above max_max_occ | reads mz_flt filters | most hits |
|---|---|---|---|---|---|---|---|---|---|---|---|---|---|
| test_gpu_stages.py::world | 168 | 53 | 32768 | 0.42 | 0 | 270 | 270 | 0 | 0 | 0 | 0 | 1 | 2078 |
| test_gpu_stages.py::_repeat_world | 5 | 119 | 32768 | 0.42 | 0 | 92 | 92 | 0 | 0 | 0 | 0 | 0 | 963 |
| test_gpu_map.py::test_map_parity_ultra_long_reads | 5 | 13 | 65536 | 0.52 | 0 | 102 | 102 | 0 | 0 | 0 | 0 | 0 | 70796 |
| test_gpu_map.py::test_map_parity_adversarial_inputs (low-complexity reads) | 10 | 10 | 16384 | 0.34 | 0 | 0 | 0 | 0 | 0 | 0 | 0 | 10 | 4497 |

Every streak of high-occurrence hits in them is filtered whole (`none`: max_high_occ <= 0): no streak is kept whole, none goes through the
heap, none meets the clamp at 128 or a hit above max_max_occ, and no table carries an entry from its last line round to line 0.

What cannot be seen from outside.  k_mzflt skips its exact sort when no bucket of its count sketch holds more than mid_occ minimizers.
count_sketch_max restates that sketch, and test_select_world_census asserts that the long read overflows a bucket although mm_seed_mz_flt
filters nothing in it; that the kernel then really went through the sort is not observable through the stage entry -- the result is the
same either way, which is the point of the proof."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
import _seed_census as SC
import _seed_worlds as W


def _looked_up(orc, reads):
    out = set()
    for rd in reads:
        out.update((orc.sketch(rd)[:, 0] >> np.uint64(8)).tolist())
    return out


@pytest.fixture(scope="module")
def wrap(built):
    w = W.wrap_world()
    orc = W.oracle_for(w)
    tab = SC.Table(SC.genome_keys(orc, [w["seq"]]))
    return dict(w=w, orc=orc, tab=tab, looked_up=_looked_up(orc, w["reads"]))


def test_wrap_world_census(wrap):
    tab, orc = wrap["tab"], wrap["orc"]
    assert tab.n_lines == 128 and len(tab.keys) == 524
    assert tab.wrap_carry > 0                                             # entries homed before the end sit in line 0
    c = SC.lookup_census(tab, wrap["looked_up"])
    assert c["n_present"] == len(tab.keys)                                # the reads look every key of the index up
    assert c["present_must_cross"] >= 1                                   # whatever order the builder inserted in
    assert len(c["absent_in_full_last_line"]) >= 1 and len(c["absent_cross"]) >= 1
    assert len(c["absent_3_fetches"]) >= 1
    assert c["n_absent"] >= 2000
    host = tab.place()                                                    # the host builder's order: the same two keys, exactly
    assert sum(1 for n, wrapped in host.values() if wrapped) == tab.wrap_carry
    # the tiny index: two lines
    t = W.two_line_world()
    o2 = W.oracle_for(t)
    t2 = SC.Table(SC.genome_keys(o2, [t["seq"]]))
    assert t2.n_lines == 2 and 1 <= len(t2.keys) <= 4
    assert len(_looked_up(o2, t["reads"]) - t2.present) > 100             # absent keys by the hundred, half of them homed in line 1


# what each option set of the select world must reach (summary() of the censuses of all reads): name -> least value
SELECT_NEEDS = dict(
    default=dict(all=3, heap=10, clamp=1, at_start=1, at_end=1, heap_straddles=1, heap_tie=1, across_mask=1, past_mask=1, none=100),
    max_max_occ_30=dict(all_cut=1, heap_cut=1, all=3, heap=10),
    occ_dist_0=dict(else_=900, across_mask=1, past_mask=1),
    occ_dist_100=dict(all=3, heap=300, clamp=1, heap_straddles=50, heap_tie=50))


def test_select_world_census():
    w = W.select_world()
    for name, fields in W.OPTION_SETS.items():
        orc = W.oracle_for(w, fields)
        assert (orc.mo.mid_occ, orc.k, orc.w) == (W.MID_OCC, 15, 10)
        cs = {}
        for rn, rd in w["reads"].items():
            c = cs[rn] = SC.select_census(orc, rd)
            _, rep_len, mini_pos, _ = orc.anchors(rd, sorted_=False)
            assert (c["n_mini"], c["rep_len"]) == (len(mini_pos), rep_len), (name, rn)      # the restatement is mm_seed_select
        s = SC.summary(list(cs.values()))
        for key, least in SELECT_NEEDS[name].items():
            assert s[key] >= least, (name, key, s)
        if name == "occ_dist_0":
            assert s["none"] == s["all"] == s["heap"] == 0
        if name == "max_max_occ_30":          # the cut must take part of a kept streak, not all of it: counts on both sides of 30
            mixed = [st for c in cs.values() for st in c["streaks"] if st["cls"] == "all" and 0 < st["above_max_max"] < st["L"]]
            assert mixed, name
        # the clamp read: one streak of more than 12000 hits, 128 of them through the heap
        st = cs["clamp"]["streaks"]
        assert len(st) == 1 and st[0]["L"] > 12000 and st[0]["at_start"] and st[0]["at_end"]
        if fields.get("occ_dist", 500) > 0:
            assert st[0]["cls"] == "heap" and st[0]["k"] == 128 and st[0]["clamped"] and st[0]["tie"]
        # the long read: hits past the mask kept in LDS, and a streak across its end
        assert cs["long"]["n_m0"] > SC.SEL_MASK_HITS + 10000 and len(w["reads"]["long"]) >= 360000
        assert any(x["across_mask"] and x["L"] > 500 for x in cs["long"]["streaks"])
        # mm_seed_mz_flt: the tandem read loses minimizers and has more than MZ_STAGE of them; the long read loses none although its
        # count sketch overflows (more than 8192 * mid_occ / 4 minimizers)
        assert cs["tandem"]["mz_filtered"] > 0 and cs["tandem"]["n_mz_raw"] > SC.MZ_STAGE and cs["tandem"]["n_mz"] > 0
        assert cs["long"]["mz_filtered"] == 0 and cs["long"]["n_mz_raw"] > SC.CS_BUCKETS * W.MID_OCC // 4
        assert cs["long"]["cs_max"] > W.MID_OCC
        assert all(c["mz_filtered"] == 0 for rn, c in cs.items() if rn != "tandem")


def test_strand_and_name_instantiations_have_work():
    """the other instantiations of the select world's tests: kept seeds with several occurrences on both strands (the c_eff loops of
    k_seed_select and k_seed_expand's rescan under MM_F_FOR_ONLY / MM_F_REV_ONLY), and anchors on the read's own contig and on a contig
    whose name sorts before the read's (MM_F_NO_DIAG | MM_F_NO_DUAL)"""
    import _named_truth as T
    w = W.select_world()
    orc = W.oracle_for(w, {})
    both = {}
    for rn in ("nine", "clamp", "revnine", "long"):
        c = SC.select_census(orc, w["reads"][rn])
        both[rn] = sum(1 for key, cnt, flt in zip(c["keys"], c["cnt"], c["flt"])
                       if not flt and cnt > 1 and len({p & 1 for p in SC.idx_get(orc, key)}) == 2)
    assert all(v >= 3 for v in both.values()) and both["clamp"] >= 100 and both["long"] >= 100, both   # kept seeds with occurrences on both strands
    orc.mo.flag |= W.NO_DIAG | W.NO_DUAL
    full = orc.anchors(w["reads"]["selfie"], sorted_=False)[0]
    a, _, _, n_self = T.filtered_anchors(orc, w["reads"]["selfie"], b"selfie")
    rid = (full[:, 0] >> np.uint64(32)) & np.uint64(0x7fffffff)
    assert n_self > 10 and (rid == 1).sum() > 1000 and (rid == 2).sum() > 10 and len(a) < len(full) - 1000


# ------------------------------------------------------------------ the host's flat table on the genome whose table wraps
def test_host_table_on_the_wrap_world(wrap):
    """mm355_index_get of the host-built index (table_insert, mm355_host_get: the `(line + 1) & mask` of both at the end of the table) against
    mmo_idx_get: every key of the genome, and absent keys -- all that the reads look up, all the census homes in full lines among them"""
    from mappy_rs import _ffi
    L = _ffi.lib()
    w, orc, tab = wrap["w"], wrap["orc"], wrap["tab"]
    io, mo = _ffi.IdxOpt(), _ffi.MapOpt()
    L.mm355_set_opt(None, C.byref(io), C.byref(mo))
    h = C.c_void_p()
    assert L.mm355_index_load(w["fa"].encode(), C.byref(io), 2, C.byref(h)) == 0
    try:
        nm, nd, tb = C.c_int64(), C.c_int64(), C.c_int64()
        L.mm355_index_stat(h, C.byref(nm), C.byref(nd), C.byref(tb), None)
        assert nd.value == len(tab.keys) and tb.value == tab.n_lines * SC.SLOTS * 16          # the model's sizing rule is the product's
        buf = np.zeros(64, np.uint64)
        for key in tab.keys:
            want = SC.idx_get(orc, key)
            n = L.mm355_index_get(h, key, buf.ctypes.data, 64)
            assert n == len(want) > 0 and [int(v) for v in buf[:n]] == want, key
        absent = sorted(wrap["looked_up"] - tab.present)
        c = SC.lookup_census(tab, absent)
        rng = np.random.default_rng(9)
        absent += [int(k) for k in rng.integers(0, 1 << 30, 3000) if int(k) not in tab.present]
        assert len(absent) >= 2000 and len(c["absent_in_full_line"]) > 100 and len(c["absent_cross"]) > 10
        for key in absent:
            assert L.mm355_index_get(h, key, buf.ctypes.data, 64) == 0 and not SC.idx_get(orc, key), key
    finally:
        L.mm355_index_free(h)
