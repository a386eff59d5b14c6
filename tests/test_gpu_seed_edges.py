"""The seed stage at its edges: k_seed_lookup and the table builders where the flat table wraps from its last line to line 0, every branch of
k_seed_select (streak filtered whole, kept whole with the max_max_occ cut, the max-heap with its ties, the clamp at 128, streaks at hit 0,
at the last hit and across the end of the mask kept in LDS, the `else` form), the strand-filter and named instantiations of select and expand
on the same reads, and k_mzflt with and without anything to filter.

Every comparison is bit-exact: the stage entry's anchors in generation order, rep_len and n_mini (and the call's n_mz / n_hit / n_a counters)
against the oracle's collect_seed_hits, read by read.  The same mid_occ, occ_dist, max_max_occ and flag are written into the product's and
the oracle's MapOpt.  That the inputs (tests/_seed_worlds.py) reach these branches is asserted without the product by
tests/test_seed_edges_host.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import _seed_census as SC
import _seed_worlds as W
import _named_truth as T


def _expected(orc, reads, names=None):
    """per read: (anchors, rep_len, n_mini, n_mz after the filter, hits)"""
    out = []
    for i, rd in enumerate(reads):
        if names is None:
            a, rep, mp, mz = orc.anchors(rd, sorted_=False)
        else:
            a, rep, mp, _ = T.filtered_anchors(orc, rd, names[i])
            mz = orc.anchors(rd, sorted_=False)[3]
        hits = sum(1 for x in (mz[:, 0] >> np.uint64(8)).tolist() if SC.idx_count(orc, x))
        out.append((a, rep, len(mp), len(mz), hits))
    return out


def _check(sr, orc, reads, names=None, label=""):
    """one stage call on `reads` against the oracle; returns the number of anchors compared"""
    exp = _expected(orc, reads, names)
    tot = sum(len(e[0]) for e in exp)
    got, rep, nmp = sr.anchors(reads, sorted_=False, cap=2 * tot + 4096, names=names)
    st = sr.stats()
    for i, (a, rep_len, n_mini, _, _) in enumerate(exp):
        assert got[i].shape == a.shape, (label, i, got[i].shape, a.shape)
        assert np.array_equal(got[i], a), (label, i)
        assert (int(rep[i]), int(nmp[i])) == (rep_len, n_mini), (label, i)
    assert (st.n_mz, st.n_hit, st.n_a) == (sum(e[3] for e in exp), sum(e[4] for e in exp), tot), label
    return tot


# ------------------------------------------------------------------ 1. the table wrap, three routes to the table
@pytest.fixture(scope="module")
def host_mmi(built, tmp_path_factory):
    """the .mmi files the host-built indices of the two small worlds save"""
    import mappy_rs
    d = tmp_path_factory.mktemp("seed_edges")
    out = {}
    for name, w in (("wrap", W.wrap_world()), ("two", W.two_line_world())):
        al = mappy_rs.Aligner(w["fa"])
        out[name] = str(d / (name + ".mmi"))
        al.save_index(out[name])
    return out


def _route(route, world, mmi, tmp_path, monkeypatch):
    import mappy_rs
    if route == "host":
        return mappy_rs.Aligner(world["fa"])
    if route == "device_built":
        al = mappy_rs.Aligner(world["fa"], build_on_gpu=True)
    else:
        monkeypatch.setenv("MM355_IDXLOAD_PIECE", "256")             # the lines at the wrap are filled from different pieces
        al = mappy_rs.Aligner(mmi, load_on_gpu=True)
    assert al._L.mm355_index_get(al._idx, 0, None, 0) == -7          # MM355_EUNSUP, no host table: what the reads see was inserted on the device
    saved = str(tmp_path / "again.mmi")
    al.save_index(saved)
    assert open(saved, "rb").read() == open(mmi, "rb").read()
    return al


@pytest.mark.parametrize("route", ["host", "device_built", "device_loaded"])
def test_table_wrap(host_mmi, tmp_path, monkeypatch, route):
    """(line + 1) & line_mask at the end of the table: k_seed_lookup's walk-on on all three routes, table_insert on the first,
    table_insert_dev on the other two.  Every key of the genome is looked up (two of them sit beyond the wrap), and thousands of absent
    keys, some of which walk from the last line into line 0 and some of which need three line fetches"""
    w = W.wrap_world()
    al = _route(route, w, host_mmi["wrap"], tmp_path, monkeypatch)
    orc = W.oracle_for(w)
    assert al._mo.mid_occ == orc.mo.mid_occ
    nl = C.c_int64()
    al._L.mm355_index_stat(al._idx, None, None, C.byref(nl), None)
    assert nl.value == 128 * SC.SLOTS * 16
    sr = al._stage_runner()
    try:
        assert _check(sr, orc, w["reads"], label=route) > 1000
        # one read per call as well: a tile of its own, the slots past its end read line 0
        for rd in w["reads"][:3]:
            _check(sr, orc, [rd], label=route)
    finally:
        sr.close()


@pytest.mark.parametrize("route", ["host", "device_built", "device_loaded"])
def test_two_line_table(host_mmi, tmp_path, monkeypatch, route):
    """an index of one 40-base contig: line_mask == 1"""
    w = W.two_line_world()
    al = _route(route, w, host_mmi["two"], tmp_path, monkeypatch)
    orc = W.oracle_for(w)
    nl = C.c_int64()
    al._L.mm355_index_stat(al._idx, None, None, C.byref(nl), None)
    assert nl.value == 2 * SC.SLOTS * 16
    sr = al._stage_runner()
    try:
        assert _check(sr, orc, w["reads"], label=route) >= 6             # the contig, its reverse complement, a read that holds it
    finally:
        sr.close()


# ------------------------------------------------------------------ 2. the branches of k_seed_select
class _Select:
    """the select world on the device and in the oracle, with one option set at a time written into both MapOpt records"""

    def __init__(self):
        import mappy_rs
        from mappy_rs import _ffi
        self.w = W.select_world()
        self.al = mappy_rs.Aligner(self.w["fa"])
        self.orc = O.OracleAligner(self.w["fa"])
        assert self.al._mo.mid_occ == self.orc.mo.mid_occ and self.al._mo.flag == self.orc.mo.flag
        self.mo0, self.omo0 = bytes(self.al._mo), bytes(self.orc.mo)
        self.mo = _ffi.MapOpt.from_buffer_copy(self.mo0)
        self.sr = _ffi.StageRunner(self.al._idx, self.mo, 0)

    def use(self, fields, flag=0):
        C.memmove(C.byref(self.mo), self.mo0, len(self.mo0))
        C.memmove(C.byref(self.orc.mo), self.omo0, len(self.omo0))
        W.set_opts(self.mo, fields, flag)
        W.set_opts(self.orc.mo, fields, flag)
        for k in ("mid_occ", "occ_dist", "max_max_occ", "q_occ_frac", "flag"):
            assert getattr(self.mo, k) == getattr(self.orc.mo, k), k

    def reads(self, *names):
        return [self.w["reads"][n] for n in (names or self.w["reads"])]


@pytest.fixture(scope="module")
def sel(built):
    s = _Select()
    yield s
    s.sr.close()


@pytest.mark.parametrize("opts", list(W.OPTION_SETS))
def test_select_branches(sel, opts):
    """default: `all`, heap (ties at the cut, tile-straddling), clamp at 128 of > 12000, st == 0, en == n_m0, a streak across hit 65536 and
    streaks past it; max_max_occ = 30: the cut inside kept and heap streaks; occ_dist = 0: the `else` form; occ_dist = 100: hundreds of
    small heaps"""
    sel.use(W.OPTION_SETS[opts])
    assert _check(sel.sr, sel.orc, sel.reads(), label=opts) > 50000


@pytest.mark.parametrize("flag", [W.FOR_ONLY, W.REV_ONLY], ids=["for_only", "rev_only"])
@pytest.mark.parametrize("opts", ["default", "occ_dist_100"])
def test_select_strand_filter(sel, opts, flag):
    """MM_F_FOR_ONLY / MM_F_REV_ONLY: the c_eff loops of k_seed_select over kept seeds out of the heap, k_seed_expand's rescan with c > 1"""
    sel.use(W.OPTION_SETS[opts], flag)
    n = _check(sel.sr, sel.orc, sel.reads(), label="%s+%x" % (opts, flag))
    sel.use(W.OPTION_SETS[opts])
    both = sum(len(sel.orc.anchors(rd, sorted_=False)[0]) for rd in sel.reads())
    assert 1000 < n < both - 1000                                           # the filter took anchors and left anchors


@pytest.mark.parametrize("opts", ["default", "max_max_occ_30", "occ_dist_100"])
def test_select_named(sel, opts):
    """MM_F_NO_DIAG | MM_F_NO_DUAL with names: k_seed_select_named / k_seed_expand_named on the same streaks.  `selfie` is the contig of
    its own name and length (diagonal dropped, MM_SEED_SELF on what is left of its strand); every read's name sorts after `aaa` (anchors
    there dropped) and before `zmain`; one read has no name"""
    sel.use(W.OPTION_SETS[opts], W.NO_DIAG | W.NO_DUAL)
    order = ["selfie", "clamp", "nine", "isle_a", "long", "revnine", "isle_c", "tandem"]
    names = [n.encode() for n in order]
    names[3] = None
    reads = sel.reads(*order)
    n = _check(sel.sr, sel.orc, reads, names=names, label="named " + opts)
    n_self = sum(T.filtered_anchors(sel.orc, rd, nm)[3] for rd, nm in zip(reads[:1], names[:1]))
    plain = sum(len(sel.orc.anchors(rd, sorted_=False)[0]) for rd in reads)
    assert n_self > 10 and 50000 < n < plain - 1000


# ------------------------------------------------------------------ 3. k_mzflt
def test_mzflt(sel):
    """the tandem read (more than MZ_STAGE minimizers, most of them filtered) and the long read (nothing to filter, but a count sketch
    that cannot prove it -- see tests/test_seed_edges_host.py on what can be observed), default q_occ_frac; each alone and both in one batch"""
    sel.use({})
    assert sel.mo.q_occ_frac > 0
    t, l = sel.reads("tandem", "long")
    raw = len(sel.orc.sketch(t))
    kept = len(sel.orc.anchors(t, sorted_=False)[3])
    assert raw > SC.MZ_STAGE and 0 < kept < raw // 4
    _check(sel.sr, sel.orc, [t], label="tandem")                          # (n_mz of the call is compared with the oracle's filtered count)
    _check(sel.sr, sel.orc, [l], label="long")
    _check(sel.sr, sel.orc, [l, t, sel.w["reads"]["isle_b"]], label="both")
