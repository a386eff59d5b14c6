"""What stands behind Aligner.map_batch and needs no GPU, no library and no Aligner (mappy_rs/_batch.py): the cut of an iterable into
sub-batches against an element-wise model stated here, and the engine -- work queue, back-off, workers, collector, result channel -- driven
with fakes that count every context taken and given back.  The GPU tests pin what map_batch returns; these pin what can deadlock or leak."""
import collections.abc
import gc
import threading
import time

import pytest

from mappy_rs import _batch as B

MSG_KEY = "AHHH Key \U0001F5DD\uFE0F  not found in iterated dictionary"
MSG_CAP = ("Internal error adding data to work queue, without backoff. "
           "Is your fastq batch larger than 50000? Perhaps try `map_batch` with back_off=True?")


# ---------------------------------------------------------------- the cut
def model(seqs, size_of, max_bases, queue_cap, back_off, eager):
    """the oracle: one element at a time.  Returns (sub-batches as lists of the caller's own dicts, the exception or None).
    A sub-batch ends when it holds size_of(its number) reads or the next read would take it over max_bases.  eager: a sub-batch that is
    full by its read count leaves before the next element is looked at (what the chunk-wise cut of a list or tuple does); otherwise it
    leaves once the next element has passed its checks.  The two differ only in how many sub-batches were out when an element raises."""
    subs, cur, bases = [], [], 0
    try:
        for n, item in enumerate(seqs):
            if eager and len(cur) >= size_of(len(subs)):
                subs.append(cur); cur, bases = [], 0
            if not isinstance(item, dict):
                raise TypeError("Element in iterable is not a dictionary")
            if "seq" not in item:
                raise KeyError(MSG_KEY)
            if not isinstance(item["seq"], str):
                raise ValueError("`seq` must be a string")
            if not back_off and n >= queue_cap:
                raise RuntimeError(MSG_CAP)
            if cur and (len(cur) >= size_of(len(subs)) or bases + len(item["seq"]) > max_bases):
                subs.append(cur); cur, bases = [], 0
            cur.append(item); bases += len(item["seq"])
    except Exception as e:
        return subs, e
    return subs + ([cur] if cur else []), None


class Seq(collections.abc.Sequence):
    """a Sequence that is neither list nor tuple"""

    def __init__(self, items):
        self._items = list(items)

    def __len__(self):
        return len(self._items)

    def __getitem__(self, i):
        return self._items[i]


WRAPS = {"list": list, "tuple": tuple, "iter": iter, "seq": Seq}


def reads_of(n, length=40):
    return [{"seq": "ACGT" * (length // 4), "i": i} for i in range(n)]


def check_cut(orig, wrap, size_of, max_bases=300, queue_cap=50, back_off=True):
    """cuts WRAPS[wrap](orig) and compares with the model on `orig`: boundaries, reads, item copies, and the exception with the number of
    sub-batches that were out before it.  Returns (sizes, exception)."""
    got, err = [], None
    try:
        for reads, items in B.sub_batches(WRAPS[wrap](orig), size_of, max_bases, queue_cap, back_off):
            got.append((reads, items))
    except Exception as e:
        err = e
    eager = wrap in ("list", "tuple") and (back_off or len(orig) <= queue_cap)
    want, want_err = model(orig, size_of, max_bases, queue_cap, back_off, eager)
    assert [len(r) for r, _ in got] == [len(s) for s in want]
    for (reads, items), sub in zip(got, want):
        assert reads == [it["seq"] for it in sub]
        assert items == sub and all(type(a) is dict and a is not b for a, b in zip(items, sub))
    assert type(err) is type(want_err) and (err is None or err.args == want_err.args), (err, want_err)
    return [len(r) for r, _ in got], err


def map_batch_size_of(n_known, max_workers, max_reads):
    """Aligner.map_batch's rule, restated: a known length is cut into about two sub-batches per worker, not below 1024 reads and not above
    max_reads; an unknown one ramps 512, 1024, ... a step every max_workers sub-batches"""
    if n_known is not None:
        fixed = min(max_reads, max(1024, -(-n_known // (2 * max_workers))))
        return lambda k: fixed
    return lambda k: min(max_reads, 512 << min(4, k // max_workers))


@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("n", [0, 1, 6, 7, 8, 13, 14, 15, 30, 63, 64, 65, 127, 128, 129])
def test_cut_by_read_limit(wrap, n):
    """read limits 7 and 64 at k * limit - 1, k * limit, k * limit + 1; nothing at all gives no sub-batch"""
    for limit in (7, 64):
        sizes, err = check_cut(reads_of(n, 4), wrap, lambda k: limit, queue_cap=1000)
        assert err is None and sizes == [limit] * (n // limit) + [n % limit] * (n % limit > 0)


@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("n, want", [(2047, [1024, 1023]), (2048, [1024, 1024]), (2049, [1025, 1024]), (9216 * 2 + 1, [9216, 9216, 1])])
def test_cut_known_length_sizes(wrap, n, want):
    """one worker: a known length below, at and above 2 * max_workers * 1024 reads, and one past two full sub-batches of 9216"""
    known = None if wrap == "iter" else n
    sizes, err = check_cut(reads_of(n, 4), wrap, map_batch_size_of(known, 1, 9216), max_bases=1 << 30, queue_cap=1 << 30)
    assert err is None and sum(sizes) == n
    if known is not None:
        assert sizes == want


@pytest.mark.parametrize("max_workers, max_reads, want", [(1, 9216, [512, 1024, 2048, 4096, 8192, 8192, 1]),
                                                         (2, 3000, [512, 512, 1024, 1024, 2048, 2048, 3000, 3000, 3000, 7])])
def test_cut_iterator_ramp(max_workers, max_reads, want):
    """unknown length: 512, 1024, ... 8192, a step every max_workers sub-batches, capped at the read limit"""
    sizes, err = check_cut(reads_of(sum(want), 4), "iter", map_batch_size_of(None, max_workers, max_reads), max_bases=1 << 30, queue_cap=1 << 30)
    assert err is None and sizes == want


@pytest.mark.parametrize("wrap", WRAPS)
def test_cut_by_base_limit(wrap):
    """300 bases, 7 reads of 40 fit: a read of 100 in the second chunk of 7 takes it over the limit (it is cut after 6 reads, 300 bases),
    a read of 500 ends the sub-batch before it and goes alone, and the sub-batches behind them are full again"""
    orig = reads_of(40)
    orig[10]["seq"] = "A" * 100
    orig[17]["seq"] = "C" * 500
    sizes, err = check_cut(orig, wrap, lambda k: 7)
    assert err is None and sizes == [7, 6, 4, 1, 7, 7, 7, 1]
    sizes, err = check_cut([{"seq": "G" * 301}], wrap, lambda k: 7)
    assert err is None and sizes == [1]


BAD = {"not_a_dict": (("seq", "ACGT"), TypeError), "no_seq": ({"id": 1}, KeyError), "bytes_seq": ({"seq": b"ACGT"}, ValueError)}


@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("kind", BAD)
def test_cut_bad_element(wrap, kind):
    """30 elements, 7 to a sub-batch: the bad one first, inside the first chunk, at chunk boundaries, and in the last chunk.  The exception
    of the reference, at that element; a list or tuple has handed out every full chunk before it, anything else the sub-batches that
    ended before the element before it"""
    bad, exc = BAD[kind]
    for at in (0, 3, 6, 7, 14, 27, 28, 29):
        orig = reads_of(30)
        orig[at] = bad
        sizes, err = check_cut(orig, wrap, lambda k: 7)
        assert type(err) is exc
        assert len(sizes) == (at // 7 if wrap in ("list", "tuple") else max(0, (at - 1) // 7))


class Sub(dict):
    pass


@pytest.mark.parametrize("wrap", WRAPS)
def test_cut_dict_subclass_is_copied_to_a_plain_dict(wrap):
    """a dict subclass is no reason to fail: it leaves the chunk-wise cut and comes out as a plain dict like the rest"""
    for at in (0, 3, 7, 29):
        orig = reads_of(30)
        orig[at] = Sub(orig[at])
        sizes, err = check_cut(orig, wrap, lambda k: 7)
        assert err is None and sizes == [7, 7, 7, 7, 2]


@pytest.mark.parametrize("wrap", WRAPS)
def test_cut_capacity_rule_without_back_off(wrap):
    """back_off=False: queue_cap elements pass, one more raises at element queue_cap -- after the seven sub-batches that ended before
    the element before it, for a list as well (the chunk-wise cut is not used then)"""
    sizes, err = check_cut(reads_of(50), wrap, lambda k: 7, back_off=False)
    assert err is None and sizes == [7] * 7 + [1]
    sizes, err = check_cut(reads_of(51), wrap, lambda k: 7, back_off=False)
    assert type(err) is RuntimeError and "without backoff" in str(err) and sizes == [7] * 7
    sizes, err = check_cut(reads_of(51), wrap, lambda k: 7, back_off=True)
    assert err is None and sum(sizes) == 51


# ---------------------------------------------------------------- the engine
class Boom(Exception):
    pass


class Fake:
    """map_sub, acquire and release for a BatchRun.  A sub-batch's `names` is its number (the engine only passes it on); a read is "k.j",
    its result ("hit", read), or a RuntimeError entry for a read named "k.empty".  Counts the contexts taken and given back and the
    calls; `pending` is what the run had pending at the start of every call.  fail_sub / fail_acquire: the sub-batch / slot that raises Boom"""

    def __init__(self, delay=0.0, fail_sub=None, fail_acquire=None):
        self.delay, self.fail_sub, self.fail_acquire = delay, fail_sub, fail_acquire
        self.lock = threading.Lock()
        self.acquired, self.released, self.calls, self.pending = [], [], [], []
        self.run = None

    def acquire(self, slot):
        with self.lock:
            if slot == self.fail_acquire:
                raise Boom("acquire %d" % slot)
            self.acquired.append(slot)
        return ("ctx", slot)

    def release(self, ctx):
        with self.lock:
            self.released.append(ctx[1])

    def map_sub(self, ctx, reads, names):
        assert ctx[0] == "ctx"
        with self.lock:
            self.calls.append(names)
            self.pending.append(self.run.pending)
        if names == self.fail_sub:
            raise Boom("map_sub %d" % names)
        if self.delay:
            time.sleep(self.delay)
        return [RuntimeError("Sequence is empty") if r.endswith("empty") else ("hit", r) for r in reads]

    def start(self, max_workers, queue_cap=1 << 30, channel_cap=1 << 30, back_off=True):
        self.run = B.BatchRun(self.map_sub, self.acquire, self.release, max_workers, queue_cap, channel_cap, back_off)
        return self.run

    def submit(self, n_sub, n_reads=5):
        """n_sub sub-batches of n_reads reads; returns the dicts, in order"""
        items = []
        for k in range(n_sub):
            sub = [{"seq": "%d.%d" % (k, j)} for j in range(n_reads)]
            self.run.submit([it["seq"] for it in sub], sub, k)
            items += sub
        return items

    def settled(self, st):
        """every thread of the run ends (within a deadline that is not waited for when all is well) and every context went back"""
        t_end = time.monotonic() + 10
        for t in st.threads:
            t.join(max(0.0, t_end - time.monotonic()))
        assert not any(t.is_alive() for t in st.threads)
        assert sorted(self.released) == sorted(self.acquired) == list(range(len(self.acquired)))


@pytest.mark.parametrize("n_sub, max_workers, want", [(40, 3, 3), (1, 4, 1), (2, 4, 2), (9, 2, 2)])
def test_every_item_comes_out_once_with_its_own_dict(n_sub, max_workers, want):
    """never more workers than max_workers or than sub-batches, one context each; results carry the very dict that was submitted"""
    f = Fake(delay=0.001)
    run = f.start(max_workers)
    items = f.submit(n_sub)
    assert len(run.st.threads) == want
    it = run.finish()
    assert it.t_first_yield is None
    got = list(it)
    assert sorted(id(d) for _, d in got) == sorted(id(d) for d in items) and all(m == ("hit", d["seq"]) for m, d in got)
    assert it.n_sub_batches == n_sub == len(it.t_sub_done) and sorted(f.calls) == list(range(n_sub)) and it.t_first_yield is not None
    assert len(f.acquired) == want and len(it._st.threads) == want + 1
    with pytest.raises(StopIteration):
        next(it)
    f.settled(it._st)


def test_nothing_submitted_ends_at_once():
    f = Fake()
    it = f.start(3).finish()
    assert list(it) == [] and it.n_sub_batches == 0 and f.acquired == [] and len(it._st.threads) == 1
    f.settled(it._st)


def test_per_read_errors_give_no_tuple():
    f = Fake()
    run = f.start(2)
    subs = [[{"seq": "0.0"}, {"seq": "0.empty"}, {"seq": "0.2"}], [{"seq": "1.empty"}], [{"seq": "2.0"}]]
    for k, sub in enumerate(subs):
        run.submit([it["seq"] for it in sub], sub, k)
    it = run.finish()
    assert sorted(d["seq"] for _, d in it) == ["0.0", "0.2", "2.0"]
    f.settled(it._st)


def test_back_off_bounds_pending_reads():
    """queue_cap 30, sub-batches of 10 reads, a slow map_sub: no call ever sees more than 30 + 10 reads pending, and all 400 results arrive;
    without back-off the same run queues far more"""
    f = Fake(delay=0.002)
    f.start(3, queue_cap=30)
    items = f.submit(40, 10)
    it = f.run.finish()
    assert sorted(d["seq"] for _, d in it) == sorted(d["seq"] for d in items) and len(items) == 400
    assert max(f.pending) <= 30 + 10, max(f.pending)
    f.settled(it._st)
    g = Fake(delay=0.002)
    g.start(3, queue_cap=30, back_off=False)
    g.submit(40, 10)
    it = g.run.finish()
    assert sum(1 for _ in it) == 400 and max(g.pending) > 30 + 10
    g.settled(it._st)


def test_full_result_channel_does_not_stop_the_producer():
    """a channel of 3 entries, sub-batches of 10 results, nobody reading: the workers cannot make room, so back-off must not wait for them"""
    f = Fake()
    f.start(3, queue_cap=30, channel_cap=3)
    items = []
    producer = threading.Thread(target=lambda: items.extend(f.submit(20, 10)), daemon=True)
    producer.start()
    producer.join(10)
    assert not producer.is_alive()
    it = f.run.finish()
    assert sorted(d["seq"] for _, d in it) == sorted(d["seq"] for d in items) and len(items) == 200
    f.settled(it._st)


def test_failing_map_sub_is_raised_once_at_the_end():
    """Boom at sub-batch 5 of 200: what was produced is yielded, then Boom, then StopIteration; the other workers stop after their call"""
    f = Fake(delay=0.001, fail_sub=5)
    f.start(3)
    items = f.submit(200)
    it = f.run.finish()
    got = []
    with pytest.raises(Boom, match="map_sub 5"):
        for r in it:
            got.append(r)
    with pytest.raises(StopIteration):
        next(it)
    seqs = [d["seq"] for _, d in got]
    assert len(set(seqs)) == len(seqs) and set(seqs) <= {d["seq"] for d in items} and not any(s.startswith("5.") for s in seqs)
    assert len(seqs) == 5 * (len(f.calls) - 1) and len(f.calls) < 200
    f.settled(it._st)


def test_failing_acquire_is_raised_once_at_the_end():
    f = Fake(delay=0.001, fail_acquire=1)
    f.start(3)
    f.submit(200)
    it = f.run.finish()
    with pytest.raises(Boom, match="acquire 1"):
        for _ in it:
            pass
    with pytest.raises(StopIteration):
        next(it)
    assert len(f.calls) < 200
    t_end = time.monotonic() + 10
    for t in it._st.threads:
        t.join(max(0.0, t_end - time.monotonic()))
    assert not any(t.is_alive() for t in it._st.threads) and sorted(f.released) == sorted(f.acquired) and 1 not in f.acquired


@pytest.mark.parametrize("channel_cap", [1 << 30, 3])
def test_abort_joins_every_thread_and_returns_every_context(channel_cap):
    """abort() after some submits -- also with workers blocked on a full channel: when it returns no thread is left and no context is out"""
    f = Fake(delay=0.002)
    run = f.start(3, channel_cap=channel_cap)
    f.submit(10)
    run.abort()
    assert len(run.st.threads) == 3 and not any(t.is_alive() for t in run.st.threads)
    assert sorted(f.released) == sorted(f.acquired) == [0, 1, 2]


@pytest.mark.parametrize("how", ["abandon", "close"])
def test_abandoned_or_closed_iterator_releases_workers_and_contexts(how):
    """300 results for a channel of 20, the iterator dropped (or closed) after one item: the workers blocked on the full channel give up,
    hand their contexts back and exit, and so does the collector"""
    f = Fake()
    f.start(3, channel_cap=20)
    f.submit(30, 10)
    it = f.run.finish()
    st = it._st
    next(it)
    assert len(st.threads) == 4 and any(t.is_alive() for t in st.threads)       # blocked: 300 results do not fit 20 slots
    if how == "close":
        it.close()
    else:
        del it
        gc.collect()
    f.settled(st)
    assert st.cancel.is_set() and st.abandoned.is_set() and len(f.acquired) == 3
