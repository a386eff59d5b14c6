"""What stands behind Aligner.map_batch and needs no GPU: the cut of an iterable into sub-batches (sub_batches, a generator without threads)
and the engine that maps them (BatchRun: work queue, back-off, lazily started workers, collector, bounded result channel, the iterator).
It knows nothing of ctypes, numpy or the library: it is given callables and caps, and moves reads, dicts and opaque results.

    run = BatchRun(map_sub, acquire, release, max_workers, queue_cap, channel_cap, back_off)
    try:
        for reads, items in sub_batches(seqs, size_of, max_bases, queue_cap, back_off):
            run.submit(reads, items, names)
    except BaseException:
        run.abort()
        raise
    return run.finish()

This is not _pipeline.Pipeline and shares no base with it, because the contracts differ: here the caller's thread is the producer and the call
returns before anyone consumes, the bound is in reads and results are per read.  A run ends through the finalizer of the iterator it handed
out (or close(), or abort()), not by leaving a `with` block."""
import collections
import threading
import time
import weakref


def sub_batches(seqs, size_of, max_bases, queue_cap, back_off):
    """yields (reads, items) for the dicts of `seqs`: reads is the list of their "seq" strings, items a copy of each dict (the reference hands
    back its own copy, lib.rs:849-855, 977-979).  Sub-batch number k holds at most size_of(k) reads and at most max_bases bases (a longer read
    goes alone).  What the reference raises for an element is raised here, out of next(), when that element is reached."""
    k = n_fast = 0
    limit = size_of(0)
    # lists and tuples of plain dicts with str sequences -- what a FASTQ reader hands over -- are cut a sub-batch at a time with
    # C-level loops (0.4 us per read instead of 2 under the interpreter: the producer shares the GIL with the workers' result
    # building).  Anything else -- another element type, a missing key, a sub-batch over the base limit, the capacity rule without
    # back-off -- leaves the remainder to the element-wise loop below, which raises what the reference raises, at the same element.
    if isinstance(seqs, (list, tuple)) and (back_off or len(seqs) <= queue_cap):
        n_all = len(seqs)
        while n_fast < n_all:
            chunk = seqs[n_fast:n_fast + limit]
            if set(map(type, chunk)) != {dict}:
                break
            try:
                reads = [it["seq"] for it in chunk]
            except KeyError:
                break
            if set(map(type, reads)) != {str} or sum(map(len, reads)) > max_bases:
                break
            yield reads, list(map(dict, chunk))
            n_fast += len(chunk)
            k += 1
            limit = size_of(k)
        if n_fast:
            seqs = seqs[n_fast:]
    reads, items, bases = [], [], 0
    for n_pending, item in enumerate(seqs, n_fast):
        if not isinstance(item, dict):
            raise TypeError("Element in iterable is not a dictionary")
        if "seq" not in item:
            raise KeyError("AHHH Key \U0001F5DD\uFE0F  not found in iterated dictionary")
        s = item["seq"]
        if not isinstance(s, str):
            raise ValueError("`seq` must be a string")
        # capacity rule made deterministic: without back-off more than 50 000 pending items is an error
        if not back_off and n_pending >= queue_cap:
            raise RuntimeError("Internal error adding data to work queue, without backoff. "
                               "Is your fastq batch larger than 50000? Perhaps try `map_batch` with back_off=True?")
        if reads and (len(reads) >= limit or bases + len(s) > max_bases):
            yield reads, items
            reads, items, bases = [], [], 0
            k += 1
            limit = size_of(k)
        reads.append(s)
        items.append(dict(item))
        bases += len(s)
    if reads:
        yield reads, items


class _Channel:
    """bounded multi-producer channel (the reference's ArrayQueue(50000) + crossbeam `bounded(20000)`, lib.rs:430, 950): producers block while it is full, the consumer blocks
    while it is empty; both waits release the GIL."""

    def __init__(self, cap):
        self.cap = cap
        self.d = collections.deque()
        self.cv = threading.Condition()

    def put_many(self, items, cancel):
        """appends the entries in order, waiting whenever the channel is full; False when `cancel` was set while waiting"""
        i, n = 0, len(items)
        with self.cv:
            while i < n:
                while len(self.d) >= self.cap:
                    if cancel.is_set():
                        return False
                    self.cv.wait(0.2)
                room = self.cap - len(self.d)
                self.d.extend(items[i:i + room])
                i += room
                self.cv.notify_all()
        return True

    def get_many(self, limit):
        """blocks until at least one entry is there, then takes up to `limit` of them under ONE lock acquisition (a lock per result was a
        microsecond and a half of the consumer's GIL time per read)"""
        with self.cv:
            while not self.d:
                self.cv.wait()
            was_full = len(self.d) >= self.cap
            n = min(limit, len(self.d))
            out = [self.d.popleft() for _ in range(n)]
            if was_full:
                self.cv.notify_all()      # producers may be waiting for room
            return out

    def __len__(self):
        return len(self.d)


class _BatchState:
    """Everything the worker threads and the collector of one map_batch call share with its iterator.  The threads hold THIS object (through
    their BatchRun), never the iterator the caller gets: when the caller drops the iterator (or calls close()) a weakref finalizer sets
    `cancel` / `abandoned` here, the workers blocked on the full result channel give up, return their GPU contexts to the Aligner's pool and
    exit -- the reference's workers stop the same way when their `tx.send` fails because the receiver is gone."""

    def __init__(self, channel_cap):
        self.ch = _Channel(channel_cap)
        self.cancel = threading.Event()      # workers stop taking sub-batches (worker error, validation error, abandoned iterator)
        self.abandoned = threading.Event()   # nobody will ever read the channel again
        self.errors = []
        self.n_sub_batches = 0
        self.t_sub_done = []      # wall-clock time each sub-batch left the GPU pipeline (tests / latency diagnostics)
        self.threads = []         # the workers; after finish() workers + collector (tests: they must all exit once the iterator is gone)

    def close(self):
        self.cancel.set()
        self.abandoned.set()


class AlignmentBatchResultIter:
    """Iterator returned by map_batch (lib.rs:923-991): yields (list[Mapping], dict) in COMPLETION order.

    Mirrors the reference's plumbing: workers push results into a bounded channel (mappy_rs.RESULT_CHANNEL_CAP entries, lib.rs:430 + 950) and
    `__next__` blocks on it (`rx.recv()`, lib.rs:973) -- here with the GIL released.  A full channel blocks the workers: a slow consumer holds
    back the GPU pipeline instead of growing memory (back-pressure).  `Finished` arrives after every worker is done (lib.rs:804-815)."""

    _FINISHED = object()

    def __init__(self, state):
        self._st = state
        self._done = False
        self._buf = []            # results taken from the channel in one go, handed out one by one (reversed: pop() from the end)
        self.t_first_yield = None
        self._fin = weakref.finalize(self, _BatchState.close, self._st)   # the state, not the iterator, is what the threads keep alive

    n_sub_batches = property(lambda s: s._st.n_sub_batches)
    t_sub_done = property(lambda s: s._st.t_sub_done)

    def __iter__(self):
        return self

    def __next__(self):
        if self._done:
            raise StopIteration("Finished")
        if not self._buf:
            self._buf = self._st.ch.get_many(2048)
            self._buf.reverse()
        r = self._buf.pop()
        if r is AlignmentBatchResultIter._FINISHED:
            self._done = True
            if self._st.errors:
                raise self._st.errors[0]
            raise StopIteration("Finished")
        if self.t_first_yield is None:
            self.t_first_yield = time.perf_counter()
        return r

    def close(self):
        """stop mapping what has not been started yet; results already produced are dropped"""
        self._st.close()


class BatchRun:
    """The engine of one map_batch call.  map_sub(ctx, reads, names) -> one entry per read (an Exception entry: no result for that read) is
    all it knows about mapping; ctx is what acquire(slot) gave the worker, which hands it to release() when it ends.
    submit() queues a sub-batch from the caller's thread -- with back_off it first waits while more than queue_cap reads are pending -- and
    starts a worker while there are fewer than max_workers and fewer than sub-batches.  finish() starts the collector, which sends `Finished`
    once every worker is done, and returns the iterator over the result channel of channel_cap entries.  The first exception of a worker
    stops the others after their current call and is raised by the iterator at `Finished`.  abort() instead of finish(): nothing is yielded,
    every thread is joined and every context is back when it returns."""

    def __init__(self, map_sub, acquire, release, max_workers, queue_cap, channel_cap, back_off):
        self._map_sub, self._acquire, self._release = map_sub, acquire, release
        self._max_workers, self._queue_cap, self._back_off = max_workers, queue_cap, back_off
        self.st = _BatchState(channel_cap)
        self._workers = self.st.threads
        self._work = collections.deque()    # sub-batches (reads, items, names) waiting for a worker
        self._cv = threading.Condition()
        self._closed = False
        self.pending = 0                    # reads in `_work`, not yet taken by a worker

    def _worker(self, slot):
        st, cv, work = self.st, self._cv, self._work
        ctx = None
        try:
            ctx = self._acquire(slot)
            while True:
                with cv:
                    while not work and not self._closed and not st.cancel.is_set():
                        cv.wait(0.2)
                    if st.cancel.is_set() or not work:
                        return
                    reads, items, names = work.popleft()
                    self.pending -= len(reads)
                    cv.notify_all()                                   # the producer may be waiting for room (back-off)
                maps = self._map_sub(ctx, reads, names)
                st.t_sub_done.append(time.perf_counter())
                # a worker error on one read => no result for that id (lib.rs:621-623)
                out = [(m, it) for m, it in zip(maps, items) if not isinstance(m, Exception)]
                if not st.ch.put_many(out, st.cancel):
                    return
        except Exception as e:   # surfaced by the iterator when it finishes, like a worker panic in the reference
            st.errors.append(e)
            st.cancel.set()
        finally:
            if ctx is not None:
                self._release(ctx)

    def submit(self, reads, items, names):
        st, cv = self.st, self._cv
        with cv:
            # the reference's work queue holds 50 000 reads (lib.rs:429): with back-off the producer sleeps until the workers have
            # made room (lib.rs:870-888), so a huge iterable never sits in memory as pending sub-batches
            # (not while the result channel is full: nobody reads it before map_batch has returned, so the workers cannot make room)
            while (self._back_off and self.pending > 0 and self.pending + len(reads) > self._queue_cap and not st.cancel.is_set()
                   and len(st.ch) < st.ch.cap):
                cv.wait(0.05)
            self._work.append((reads, items, names))
            self.pending += len(reads)
            st.n_sub_batches += 1
            cv.notify()
        if len(self._workers) < self._max_workers and len(self._workers) < st.n_sub_batches:
            t = threading.Thread(target=self._worker, args=(len(self._workers),), daemon=True)
            self._workers.append(t)
            t.start()

    def _close_and_join(self):
        with self._cv:
            self._closed = True
            self._cv.notify_all()
        for t in self._workers:
            t.join()

    def _collect(self):   # the reference's collector thread: `Finished` once every worker is done (lib.rs:804-815)
        self._close_and_join()
        self.st.ch.put_many([AlignmentBatchResultIter._FINISHED], self.st.abandoned)

    def finish(self):
        t = threading.Thread(target=self._collect, daemon=True)
        t.start()
        self.st.threads = self._workers + [t]
        return AlignmentBatchResultIter(self.st)

    def abort(self):
        self.st.close()                     # the workers stop after their current sub-batch
        self._close_and_join()
