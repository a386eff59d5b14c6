"""What stands behind map_file / map_bam_file and needs no GPU: the sub-batch pipeline (mappy_rs/_pipeline.py), driven with fake callables
that count every allocation and every free, and the merge driver with its two step functions (mappy_rs._merge, _GatherStep, _PackedStep) on
synthetic runs, against the stable sort stated in Python.  The GPU tests pin the files the writers make; these pin what can deadlock or leak."""
import io
import random
import threading
import time

import numpy as np
import pytest

import _bammerge as M


# ---------------------------------------------------------------- the pipeline
class Boom(Exception):
    pass


class Fake:
    """n_items items for a Pipeline of n_workers.  Every item, result and context is counted when it is made and when it is given back; a
    sub-batch exists from the allocation of its item to the free of its result (in between it is an item, a result, or for the length of one
    work() call both), and on every allocation at most 2 * n_workers may exist: the check is made here, under the lock.
    fail_next / fail_work: the index at which next_item / work raises Boom"""

    def __init__(self, n_items, n_workers, fail_next=None, fail_work=None, delay=0.0):
        self.n_items, self.n_workers, self.fail_next, self.fail_work, self.delay = n_items, n_workers, fail_next, fail_work, delay
        self.lock = threading.Lock()
        self.k = 0
        self.items, self.results = set(), set()           # alive now
        self.items_made = self.items_freed = self.results_made = self.results_freed = 0
        self.slots, self.released = [], []
        self.most, self.over = 0, []
        self.rng = random.Random(5)

    def _count(self):
        n = len(self.items | self.results)
        self.most = max(self.most, n)
        if n > 2 * self.n_workers or len(self.items) > 2 * self.n_workers or len(self.results) > 2 * self.n_workers:
            self.over.append((n, len(self.items), len(self.results)))

    def next_item(self):
        with self.lock:
            if self.k == self.fail_next:
                raise Boom("next_item %d" % self.k)
            if self.k == self.n_items:
                return None
            k, self.k = self.k, self.k + 1
            assert k not in self.items
            self.items.add(k); self.items_made += 1
            self._count()
            return ("item", k)

    def work(self, ctx, item):
        k = item[1]
        assert ctx[0] == "ctx"
        if self.delay:
            with self.lock:
                d = self.rng.uniform(0, self.delay)
            time.sleep(d)
        with self.lock:
            assert k in self.items
            if k == self.fail_work:
                raise Boom("work %d" % k)
            self.results.add(k); self.results_made += 1
            self._count()
            return ("result", k)

    def free_item(self, item):
        with self.lock:
            self.items.remove(item[1]); self.items_freed += 1        # (KeyError: freed twice)

    def free_result(self, result):
        with self.lock:
            self.results.remove(result[1]); self.results_freed += 1

    def acquire(self, slot):
        with self.lock:
            self.slots.append(slot)
        return ("ctx", slot)

    def release(self, ctx):
        with self.lock:
            self.released.append(ctx[1])

    def pipeline(self, ordered):
        from mappy_rs import _pipeline
        return _pipeline.Pipeline(self.next_item, self.work, self.free_item, self.free_result, self.acquire, self.release, self.n_workers, ordered)

    def settled(self, pipe):
        """after the `with` block: no thread is left, and everything made was given back exactly once"""
        t_end = time.monotonic() + 5
        for t in pipe.threads:
            t.join(max(0.0, t_end - time.monotonic()))
        assert not any(t.is_alive() for t in pipe.threads)
        assert self.items_made == self.items_freed and not self.items
        assert self.results_made == self.results_freed and not self.results
        assert sorted(self.slots) == sorted(self.released) == list(range(len(self.slots)))
        assert not self.over and self.most <= 2 * self.n_workers, (self.over[:3], self.most)


@pytest.mark.parametrize("ordered", [True, False])
def test_delivery_order_and_memory_bound(ordered):
    """40 items, 3 workers, work sleeps 0 - 5 ms: in order as 0..39, or every index exactly once; never more than 6 sub-batches exist;
    a result is alive while the loop body has it and freed when the loop asks for the next"""
    f = Fake(40, 3, delay=0.005)
    got = []
    with f.pipeline(ordered) as pipe:
        for k, res in pipe:
            assert res == ("result", k) and k in f.results
            assert not got or got[-1] not in f.results
            got.append(k)
    assert (got == list(range(40))) if ordered else (sorted(got) == list(range(40)))
    assert pipe.n_items == 40 and len(f.slots) == 3
    f.settled(pipe)
    assert f.most > 1                       # (the bound was approached at all: more than one sub-batch at a time)


@pytest.mark.parametrize("n_items, n_workers, want", [(1, 4, 1), (2, 4, 2), (9, 2, 2), (0, 3, 0)])
def test_no_more_workers_than_items(n_items, n_workers, want):
    """one item gives one worker; no item: no worker, no context, and the loop ends at once"""
    f = Fake(n_items, n_workers)
    with f.pipeline(True) as pipe:
        got = [k for k, _ in pipe]
    assert got == list(range(n_items)) and pipe.n_items == n_items
    assert len(f.slots) == want and len(pipe.threads) == 1 + want
    f.settled(pipe)


@pytest.mark.parametrize("ordered", [True, False])
@pytest.mark.parametrize("where", ["next_item", "work", "consumer", "break"])
def test_failure_stops_everything_and_frees_everything(where, ordered):
    """Boom at item 5 in next_item, in work, or in the loop body at the sixth result: that exception is the one raised, every thread ends,
    every item, result and context made is given back once.  A loop that is left with `break` ends the same way, without an exception"""
    f = Fake(40, 3, fail_next=5 if where == "next_item" else None, fail_work=5 if where == "work" else None, delay=0.002)
    n_got = 0
    try:
        with f.pipeline(ordered) as pipe:
            for k, res in pipe:
                if n_got == 5 and where == "consumer":
                    raise Boom("consumer %d" % n_got)
                if n_got == 5 and where == "break":
                    break
                n_got += 1
        raised = None
    except Boom as e:
        raised = str(e)
    assert raised == {"next_item": "next_item 5", "work": "work 5", "consumer": "consumer 5", "break": None}[where]
    assert n_got <= 5 or (where == "work" and not ordered)      # in order nothing behind the failed item is delivered
    f.settled(pipe)
    assert f.items_made < 40                                    # the reader stopped early


def test_acquire_failure_is_raised():
    f = Fake(8, 2)

    def no_context(slot):
        raise Boom("acquire %d" % slot)
    f.acquire = no_context
    with pytest.raises(Boom, match="acquire"):
        with f.pipeline(True) as pipe:
            for _ in pipe:
                pass
    f.slots = f.released = []
    f.settled(pipe)


# ---------------------------------------------------------------- the merge: one driver, two step functions
def _synthetic_runs(seed):
    """three runs of records of many sizes with keys that tie inside a run and across runs: (the _bammerge runs, per run the sorted keys)"""
    rng = np.random.default_rng(seed)
    sizes = ((37, 4095, 4096, 70000, 41, 300, 64), (100, 200, 5000, 37, 66000, 41), (300, 400, 38, 39, 8193))
    runs = [M.Run(rng, s, levels=(6, 0), kinds=(0, 1)) for s in sizes]
    keys = [np.sort(rng.integers(0, 6, len(s)).astype(np.uint64)) for s in sizes]
    return runs, keys


def _stable_sort_stream(runs, keys):
    """the model: all records, run after run, stably sorted by key"""
    recs = [(int(k), r.recs[i]) for r, ks in zip(runs, keys) for i, k in enumerate(ks)]
    return b"".join(b for _, b in sorted(recs, key=lambda x: x[0]))


@pytest.mark.parametrize("chunk", [1, 9000, 1 << 30])
def test_merge_steps_give_the_stable_sort(built, monkeypatch, chunk):
    """a step of one record, of a few records, of everything: the plain step (level 0: no context) and the packed step (host `where`, both
    levels) write the blocks of the model's stable sort -- mm355_bgzf_wrap / mm355_bgzf_deflate of that stream, byte for byte"""
    import mappy_rs
    from mappy_rs import _ffi
    L = _ffi.lib()
    monkeypatch.setattr(mappy_rs, "SORT_CHUNK_BYTES", chunk)
    runs, keys = _synthetic_runs(11)
    want = _stable_sort_stream(runs, keys)
    lens = [np.diff(r.off) for r in runs]
    none = np.zeros(0, np.int64)

    def no_context(slot):
        raise AssertionError("a host step took a context")
    # plain runs: the spool holds the records themselves
    raw_at = np.cumsum([0] + [len(r.raw) for r in runs])
    plain = [mappy_rs._Run(k, l, int(at), none, None) for k, l, at in zip(keys, lens, raw_at)]
    out = io.BytesIO()
    n_out, t_ix = mappy_rs._merge(L, plain, np.frombuffer(b"".join(r.raw for r in runs), np.uint8), out, mappy_rs._GatherStep(L, 0), None, (no_context, None))
    assert b"".join(M.members(out.getvalue())) == want
    assert out.getvalue() == mappy_rs.bgzf_wrap(want) and n_out == len(out.getvalue()) and t_ix == 0.0
    # packed runs: the spool holds their members
    spool = np.frombuffer(M.spool_of(runs), np.uint8)
    packed = [mappy_rs._Run(k, l, r.place, none, r.blk) for k, l, r in zip(keys, lens, runs)]
    for level in (0, 1):
        out = io.BytesIO()
        n_out, _ = mappy_rs._merge(L, packed, spool, out, mappy_rs._PackedStep(L, level, _ffi.PAF_HOST), None, (no_context, None))
        assert b"".join(M.members(out.getvalue())) == want, level
        assert out.getvalue() == mappy_rs.bgzf_wrap(want, compress=bool(level)) and n_out == len(out.getvalue()), level


def test_merge_of_nothing(built):
    import mappy_rs
    from mappy_rs import _ffi
    L = _ffi.lib()
    out = io.BytesIO()
    assert mappy_rs._merge(L, [], np.zeros(0, np.uint8), out, mappy_rs._GatherStep(L, 0)) == (0, 0.0) and out.getvalue() == b""
