"""The sub-batch pipeline behind map_file / map_bam_file: a reader thread, lazily started workers, the caller's loop as the consumer.
It knows nothing of formats, ctypes or the GPU: it is given callables and moves opaque items and results between threads.

    with Pipeline(next_item, work, free_item, free_result, acquire, release, n_workers, ordered) as pipe:
        for k, result in pipe:
            ...

next_item() returns the next sub-batch, or None at the end (reader thread); work(ctx, item) turns one into a result (a worker thread; ctx is
what acquire(slot) gave that worker); the loop gets (input index, result), in input order when `ordered`, else as results complete.
Memory: 2 * n_workers tokens, one per sub-batch in existence, from before it is read until the loop is done with its result (it asks for
the next one, or leaves): a slow consumer holds the reader back.  Workers: started as items arrive, never more than there are items, each
with one context from its start to its end.  Failure: the first exception of the reader or a worker stops the rest (the others finish the
call they are in) and is raised in the loop.  The end: leaving the `with` block -- normally, through that exception, one of the loop body's
own, or a `break` -- joins every thread, frees every item no worker took and every result the loop did not get or still holds, exactly once
each, and has returned every context.  The loop body never frees what it is given."""
import queue
import threading


class Pipeline:
    def __init__(self, next_item, work, free_item, free_result, acquire, release, n_workers, ordered):
        self._next_item, self._work, self._free_item, self._free_result = next_item, work, free_item, free_result
        self._acquire, self._release, self._n_workers, self._ordered = acquire, release, n_workers, ordered
        self._tokens = threading.Semaphore(2 * n_workers)
        self._todo = queue.Queue()              # (index, item) for the workers; None: no more
        self._cv = threading.Condition()
        self._done = {}                         # index -> result, in completion order, until the loop takes it
        self._held = None                       # the result the loop body has now
        self._errors = []
        self._cancel = threading.Event()
        self._n_taken = 0
        self.n_items = None                     # how many items were read; known once the reader has ended
        self.threads = []                       # the reader and the workers

    def __enter__(self):
        t = threading.Thread(target=self._read, daemon=True)
        self.threads.append(t)
        t.start()
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __iter__(self):
        return self

    def _fail(self, e):
        with self._cv:
            self._errors.append(e)
            self._cancel.set()
            self._cv.notify_all()

    def _read(self):
        k = 0
        try:
            while not self._cancel.is_set():
                if not self._tokens.acquire(timeout=0.2):
                    continue
                item = self._next_item()
                if item is None:
                    break
                self._todo.put((k, item))
                k += 1
                if len(self.threads) - 1 < min(self._n_workers, k):
                    t = threading.Thread(target=self._run, args=(len(self.threads) - 1,), daemon=True)
                    self.threads.append(t)
                    t.start()
        except BaseException as e:
            self._fail(e)
        finally:
            for _ in self.threads[1:]:
                self._todo.put(None)
            with self._cv:
                self.n_items = k
                self._cv.notify_all()

    def _run(self, slot):
        ctx = None
        try:
            ctx = self._acquire(slot)
            while True:
                got = self._todo.get()
                if got is None:
                    return
                k, item = got
                try:
                    if self._cancel.is_set():       # (after a failure the queue is only emptied)
                        continue
                    result = self._work(ctx, item)
                finally:
                    self._free_item(item)
                with self._cv:
                    self._done[k] = result
                    self._cv.notify_all()
        except BaseException as e:
            self._fail(e)
        finally:
            if ctx is not None:
                self._release(ctx)

    def _drop_held(self):
        if self._held is not None:
            held, self._held = self._held, None
            self._free_result(held[0])
            self._tokens.release()

    def __next__(self):
        self._drop_held()
        with self._cv:
            while True:
                if self._cancel.is_set():
                    if self._errors:
                        raise self._errors[0]
                    raise StopIteration
                k = self._n_taken if self._ordered else next(iter(self._done), None)
                if k in self._done:
                    result = self._done.pop(k)
                    break
                if self.n_items is not None and self._n_taken >= self.n_items:
                    raise StopIteration
                self._cv.wait(0.2)
        self._n_taken += 1
        self._held = (result,)
        return k, result

    def close(self):
        """stops what has not begun, waits for every thread, frees what is left; safe to call again"""
        self._cancel.set()
        for t in self.threads:
            t.join()
        self._drop_held()
        while not self._todo.empty():           # what no worker took: the items read after a failure
            got = self._todo.get()
            if got is not None:
                self._free_item(got[1])
        while self._done:
            self._free_result(self._done.popitem()[1])
