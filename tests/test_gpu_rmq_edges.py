"""mg_lchain_rmq on the device at its edges: k_rmq_sort, k_rmq_dp and k_rmq_backtrack (mappy-rs_amd/csrc/mm355_rmq.hip) with rmq_pass
around them, held read by read to what the plain model of tests/_rmq_census.py predicts from the oracle:

state       every read comes back KEEP, DONE, HOST or HOST_ALL exactly as predicted -- the kernel hands a read over when, and only when,
            its contract says so (two equal minimal priorities, an inner set the rings cannot hold, a negative cap); no read is skipped;
chains      KEEP and DONE reads hold the oracle's u[] and compacted anchors bit for bit; HOST / HOST_ALL reads hold no chain and the
            anchors the handed-over pass started from, sorted by x;
statistics  n_rmq_reads, n_rmq_host, n_v_rmq and rmq_scanned of the call are the sums the model gives;
end to end  the reads handed over, and as many that are not, map like the oracle's (the hand-over to the host chainer);
recovery    after rmq_size_cap = -1 has sent every read to the host, the same context chains the default set.

The inputs and option sets are tests/_rmq_worlds.py; that they reach the HBM prefix of the window, the reuse of the summary slots, a
winner beyond the rings, the cap clamp, every form of the inner walk and every event is asserted without the product by
tests/test_rmq_census_host.py.  The same fields are written into the product's and the oracle's MapOpt.

Time of the tests, measured on an MI355X machine (call phase; nearly all of it is the model's prediction on the CPU, worked out once per
world and option set -- the sr.rmq call itself takes 5 to 60 ms): edges_ont default 3.7 s (with the world's build), every other case of
test_rmq_state_chains_and_statistics between 0.05 and 2.9 s (the wide worlds 1.7 to 2.9 s, edges_asm20 1.1 to 1.9 s, edges_ont 0.8 to
1.0 s, the arrays worlds 0.2 to 0.6 s); test_handed_over_reads_map_like_the_oracle 3.0 s (wide_asm20), 2.1 s (wide_ont) and 0.1 to 0.2 s for
the other worlds; test_recovery_after_a_negative_cap 0.13 s, test_mixed_batch 0.05 s.  The module as a whole: 2.0 min."""
import collections
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import _chain_worlds as CW
import _rmq_census as RC
import _rmq_worlds as W

STATS = ("n_rmq_reads", "n_rmq_host", "n_v_rmq", "rmq_scanned")
RMQ_FLAGS = RC.MM_F_RMQ | RC.MM_F_NO_LJOIN | RC.MM_F_SPLICE | RC.MM_F_SR


class _World:
    """one world on the device, with one option set at a time written into the product's MapOpt (the oracle's copy of the set lives in
    W.predictions, and the two records are compared field by field)"""

    def __init__(self, name):
        import mappy_rs
        from mappy_rs import _ffi
        self.name = name
        wd = W.WORLDS[name]()
        self.al = mappy_rs.Aligner(wd["fa"], preset=wd["preset"])
        self.mo0 = bytes(self.al._mo)
        self.mo = _ffi.MapOpt.from_buffer_copy(self.mo0)
        self.sr = _ffi.StageRunner(self.al._idx, self.mo, 0)
        self.names = list(wd["reads"])
        self.reads = list(wd["reads"].values())
        self.cap = sum(len(a) for a in W.anchors_of(name)) + 4096

    def use(self, opts):
        C.memmove(C.byref(self.mo), self.mo0, len(self.mo0))
        CW.set_opts(self.mo, W.OPTION_SETS[opts])
        omo = W.oracle_for(self.name, W.OPTION_SETS[opts]).mo
        assert (self.al.k, self.al.w) == (W.oracle_for(self.name).k, W.oracle_for(self.name).w)
        for key in W.FIELDS:
            mine, theirs = getattr(self.mo, key), getattr(omo, key)
            assert (mine & RMQ_FLAGS) == (theirs & RMQ_FLAGS) if key == "flag" else mine == theirs, key

    def check(self, opts):
        """one sr.rmq call on all reads of the world under `opts` against the predictions; returns the states"""
        self.use(opts)
        pds = W.predictions(self.name, opts)
        got = self.sr.rmq(self.reads, cap=self.cap)
        st = self.sr.stats()
        assert len(got) == len(pds) == len(self.reads)
        want = collections.Counter()
        for nm, (u, a, state), pd in zip(self.names, got, pds):
            label = (self.name, opts, nm)
            want.update(pd["stats"])
            assert state == pd["state"], (label, state, pd["state"], [(k, r["event"], r["at"]) for k, _, _, r in pd["passes"]])
            if state >= RC.HOST:
                assert len(u) == 0, label
                assert a.shape == pd["a"].shape and np.all(a[1:, 0] >= a[:-1, 0]), label
                order = lambda x: x[np.lexsort((x[:, 1], x[:, 0]))]
                assert np.array_equal(order(a), order(pd["a"])), label
            else:
                assert np.array_equal(u, pd["u"]), label
                assert np.array_equal(a, pd["a"]), label
        have = {key: int(getattr(st, key)) for key in STATS}
        assert have == {key: int(want[key]) for key in STATS}, (self.name, opts, have, dict(want))
        return [pd["state"] for pd in pds]

    def close(self):
        self.sr.close()


@pytest.fixture(scope="module")
def worlds(built):
    ws = {}

    def get(name):
        if name not in ws:
            ws[name] = _World(name)
        return ws[name]
    yield get
    for w in ws.values():
        w.close()


@pytest.mark.parametrize("world,opts", [(world, opts) for world, sets in W.RUNS.items() for opts in sets], ids=lambda x: x)
def test_rmq_state_chains_and_statistics(worlds, world, opts):
    """the regression case kept from the first run of this test: edges_asm20 and edges_asm5 hold three reads without anchors (random,
    empty, tiny).  rmq_pass counted them into n_rmq_reads after a primary pass (its flags start out DONE for every read of the batch,
    listed or not): 40 where the model says 37, under every option set; states, chains and the other three statistics were right"""
    states = worlds(world).check(opts)
    assert len(states) >= 3


def test_recovery_after_a_negative_cap(worlds):
    w = worlds("edges_ont")
    assert RC.DONE not in w.check("cap_neg")
    assert RC.DONE in w.check("default")
    w = worlds("edges_asm20")
    assert set(w.check("cap_neg")) == {RC.KEEP, RC.HOST_ALL}
    assert RC.DONE in w.check("default")


def test_mixed_batch(worlds):
    """KEEP, DONE and HOST reads in one call: the resident grids' cursors serve a ragged list, k_rmq_backtrack skips the flagged reads"""
    states = worlds("arrays_hifi").check("default")
    assert {RC.KEEP, RC.DONE, RC.HOST} <= set(states)


@pytest.mark.parametrize("world", list(W.RUNS))
def test_handed_over_reads_map_like_the_oracle(built, world):
    """the hand-over to the host chainer (mm355_glue_chain_rmq and the long-join branch of the host tail) under the preset's own options:
    the reads predicted HOST / HOST_ALL and as many (two at least) predicted DONE, hit for hit as tests/test_gpu_map.py compares them"""
    import mappy_rs
    from test_gpu_map import check_reads
    wd = W.WORLDS[world]()
    pds = W.predictions(world, "default")
    reads = list(wd["reads"].values())
    host = [rd for rd, pd in zip(reads, pds) if pd["state"] >= RC.HOST]
    done = [rd for rd, pd in zip(reads, pds) if pd["state"] == RC.DONE][:max(len(host), 2)]
    al = mappy_rs.Aligner(wd["fa"], preset=wd["preset"])
    orc = O.OracleAligner(wd["fa"], preset=wd["preset"])
    n_hits, _ = check_reads(al, orc, host + done)
    assert n_hits >= 2
