"""The chain fill at its edges: k_chain_segments, k_chain_small and k_chain_big (chain_big_segment) against the oracle's mg_lchain_dp fill,
bit-exact in a, f, p and v, on inputs that between them reach every segment class of k_chain_segments and every regime of the wave's
scan -- LDS-ring and HBM reads, the max_chain_iter clamp at 40, 200, 5000 and 8000, the 64-anchor jump of st, the break and the n_skip
carried from one 64-lane batch to the next, the reflected walk of the closed form, the max_ii rescan and rescue, anchors 32768 and more
into a segment -- under option sets that move every quantity the fill reads: max_chain_iter, max_chain_skip, bw, max_gap, max_gap_ref,
max_frag_len, chain_gap_scale, chain_skip_scale (never non-zero on the device before) and another k / w.

The same fields are written into the product's and the oracle's MapOpt.  That the inputs (tests/_chain_worlds.py) reach these branches
is asserted without the product by tests/test_chain_census_host.py.

GPU time of the tests, measured on an MI355X (call phase): every case of test_fill_parity, test_fill_parity_other_k_w and
test_chains_parity under 0.2 s, the two worlds' fixture 0.6 s; test_mosaic_fill 2.5 s (default), 1.8 s (skip_1) and 0.2 s (iter_3_skip_0)
-- the read's 150 000 anchors are one segment, so one wave."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import _chain_worlds as W

MM355_EUNSUP = -7


class _World:
    """one world on the device and in the oracle, with one option set at a time written into both MapOpt records; the oracle's sorted
    anchors of every read are worked out once (no option set here touches the seed stage)"""

    def __init__(self, wd, k=None, w=None):
        import mappy_rs
        from mappy_rs import _ffi
        self.wd = wd
        kw = {} if k is None else dict(k=k, w=w)
        self.al = mappy_rs.Aligner(wd["fa"], preset=W.PRESET, **kw)
        self.orc = O.OracleAligner(wd["fa"], preset=W.PRESET, k=k, w=w)
        assert (self.al.k, self.al.w, self.al._mo.mid_occ) == (self.orc.k, self.orc.w, self.orc.mo.mid_occ)
        self.mo0, self.omo0 = bytes(self.al._mo), bytes(self.orc.mo)
        self.mo = _ffi.MapOpt.from_buffer_copy(self.mo0)
        self.sr = _ffi.StageRunner(self.al._idx, self.mo, 0)
        self.reads = list(wd["reads"].values())
        self.anchors = [self.orc.anchors(rd, sorted_=True)[0] for rd in self.reads]
        self.cap = sum(len(a) for a in self.anchors) + 4096

    def use(self, fields):
        C.memmove(C.byref(self.mo), self.mo0, len(self.mo0))
        C.memmove(C.byref(self.orc.mo), self.omo0, len(self.omo0))
        W.set_opts(self.mo, fields)
        W.set_opts(self.orc.mo, fields)
        for key in ("bw", "max_gap", "max_gap_ref", "max_frag_len", "max_chain_skip", "max_chain_iter", "chain_gap_scale", "chain_skip_scale"):
            assert getattr(self.mo, key) == getattr(self.orc.mo, key), key

    def check_fill(self, label):
        """sr.chain on all reads in one call against the oracle; returns the anchors compared"""
        got = self.sr.chain(self.reads, cap=self.cap)
        for i, rd in enumerate(self.reads):
            a, f, p, v = got[i]
            ef, ep, ev, _ = self.orc.chain_fill(self.anchors[i], len(rd))
            assert np.array_equal(a, self.anchors[i]), (label, i)
            assert np.array_equal(f, ef), (label, i, np.flatnonzero(f != ef)[:8])
            assert np.array_equal(p.astype(np.int64), ep), (label, i, np.flatnonzero(p != ep)[:8])
            assert np.array_equal(v, ev), (label, i, np.flatnonzero(v != ev)[:8])
        return sum(len(a) for a in self.anchors)

    def check_chains(self, label):
        got = self.sr.chains(self.reads, cap=self.cap)
        n_u = 0
        for i, rd in enumerate(self.reads):
            eu, eb = self.orc.chains(self.anchors[i], len(rd))
            assert np.array_equal(got[i][0], eu), (label, i)
            assert np.array_equal(got[i][1], eb), (label, i)
            n_u += len(eu)
        return n_u

    def close(self):
        self.sr.close()


@pytest.fixture(scope="module")
def worlds(built):
    ws = {name: _World(make()) for name, make in W.WORLDS.items()}
    yield ws
    for w in ws.values():
        w.close()


@pytest.mark.parametrize("opts", list(W.OPTION_SETS))
def test_fill_parity(worlds, opts):
    for name, w in worlds.items():
        w.use(W.OPTION_SETS[opts])
        assert w.check_fill((name, opts)) > 10000


@pytest.mark.parametrize("kw", W.KW_SETS, ids=lambda kw: "k%d_w%d" % kw)
def test_fill_parity_other_k_w(built, kw):
    """another q_span (19 and 21 instead of 15) on the arrays world"""
    w = _World(W.arrays_world(), *kw)
    try:
        w.use({})
        assert w.check_fill(kw) > 3000
        w.use(W.OPTION_SETS["skip_scale_0.5_gap_scale_2"])
        assert w.check_fill(kw) > 3000
    finally:
        w.close()


@pytest.mark.parametrize("max_iter", [8001, 0])
def test_max_chain_iter_outside_the_mark_window_is_refused(worlds, max_iter):
    w = worlds["stages"]
    w.use(dict(max_chain_iter=max_iter))
    from mappy_rs import _ffi
    with pytest.raises(_ffi.Mm355Error) as e:
        w.sr.chain(w.reads[:1], cap=w.cap)
    assert e.value.code == MM355_EUNSUP
    w.use({})
    assert len(w.sr.chain(w.reads[:1], cap=w.cap)[0][0]) == len(w.anchors[0])       # the context goes on working


@pytest.mark.parametrize("opts", W.CHAINS_SETS)
def test_chains_parity(worlds, opts):
    """mg_chain_backtrack and compact_a behind fills they had not seen: u[] and the compacted anchors"""
    n_u = 0
    for name, w in worlds.items():
        w.use(W.OPTION_SETS[opts])
        n_u += w.check_chains((name, opts))
    assert n_u > 20


@pytest.fixture(scope="module")
def mosaic(built):
    w = _World(W.mosaic_world())
    yield w
    w.close()


@pytest.mark.parametrize("opts", list(W.MOSAIC_SETS))
def test_mosaic_fill(mosaic, opts):
    """117 000 anchors of the read lie 32768 and more into their segment: a mark of tw[] left in a slot none of whose aliases was written
    since answers `marked` for the anchor 32768 further on.  On the kernel that cleared tw[] once per segment only, iter_3_skip_0 failed
    (f of anchor 131377: one of the two anchors the model of the kernel's write order names, tests/test_chain_census_host.py) and skip_1
    and default passed, as that model says they do: the wave writes the marks of all 64 lanes of a batch, so the slots of a co-linear
    stretch are rewritten at once.  With tw[] cleared every 32768 anchors all three pass."""
    mosaic.use(W.MOSAIC_SETS[opts])
    assert mosaic.check_fill(("mosaic", opts)) > 140000
