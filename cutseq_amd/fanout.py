"""Ordered fan-out over the GPUs, once for both host pipelines (``run.run_pipeline``, ``textio.run_text_pipeline``).

Counterpart of ``make_runner(inpaths, cores=N)`` + ``runner.run`` (cutseq/run.py:436, 473, 753, 794): items are dealt
round-robin to one :class:`Worker` thread per GPU, come back in any order and are emitted strictly in input order.
What a worker does with an item and what the consumer does with a finished one is the caller's; the threads, the
sentinels, the re-ordering and which error wins are here, because a mistake in them is a hang, not a wrong byte.
"""
from __future__ import annotations

import queue
import threading
import time
from collections import deque
from typing import Callable, Iterable, List, Optional, Sequence

from . import shard


class Worker(threading.Thread):
    """One GPU: keeps ``SLOTS`` items in flight on its engine and reports every finished one to ``done`` (the queue
    :func:`run_ordered` gives its workers) as ``(k, result)``, then itself ("this device is finished", or failed:
    ``error``).  Subclasses supply the five methods below.  (``self.engine`` is what ``_collect_stats`` asks.)"""

    SLOTS = 2

    def __init__(self, name: str):
        super().__init__(daemon=True, name=name)
        self.done: Optional["queue.Queue"] = None
        self.inbox: "queue.Queue" = queue.Queue(maxsize=self.SLOTS)
        self.inflight: deque = deque()  # (k, slot, handle), oldest first
        self.submitted = 0
        self.engine = None
        self.stats = None  # summed cs_stats of every engine this device has had
        self.poly_a_bp = None  # ... and, for a plan with a PolyATrimOp, the bases those removed per mate
        self.error: Optional[BaseException] = None

    def begin(self) -> None:
        """Before the first item."""

    def ensure(self, item) -> None:
        """The engine this item needs.  A rebuild calls :meth:`drain` first, and :meth:`_collect_stats` before it
        closes a ``self.engine`` that has counted."""

    def submit(self, slot: int, item):
        """Start the item on ``slot`` -> what :meth:`finish` needs to complete it."""
        raise NotImplementedError

    def finish(self, slot: int, handle):
        """Wait for ``slot`` -> the result that goes to ``done``."""
        raise NotImplementedError

    def close(self) -> None:
        """Release the engine(s); always called."""

    @staticmethod
    def _tick(key: str, t0: float) -> float:
        """Profiling hook of :meth:`run` (keys idle, ensure, submit) -> now.  The base records nothing;
        ``textio.TextWorker`` overrides it with the CUTSEQ_PROFILE accounting."""
        return time.perf_counter()

    def _collect_stats(self) -> None:
        part = [s.as_dict() for s in self.engine.stats()]
        self.stats = part if self.stats is None else [shard.merge_stats([a, b]) for a, b in zip(self.stats, part)]
        if getattr(getattr(self.engine, "plan", None), "has_poly_a", False):  # (engines without the op have no such count)
            self.poly_a_bp = [a + b for a, b in zip(self.poly_a_bp or (0, 0), self.engine.polya_bp())]

    def _finish_oldest(self) -> None:
        k, slot, handle = self.inflight.popleft()
        self.done.put((k, self.finish(slot, handle)))

    def drain(self) -> None:
        while self.inflight:
            self._finish_oldest()

    def run(self):
        try:
            t0 = time.perf_counter()
            self.begin()
            t0 = self._tick("ensure", t0)
            while True:
                item = self.inbox.get()
                t0 = self._tick("idle", t0)
                if item is None:
                    break
                k, item = item
                self.ensure(item)
                self._tick("ensure", t0)
                if len(self.inflight) == self.SLOTS:
                    self._finish_oldest()  # frees exactly the slot this item takes
                t0 = time.perf_counter()
                slot = self.submitted % self.SLOTS
                self.submitted += 1
                self.inflight.append((k, slot, self.submit(slot, item)))
                t0 = self._tick("submit", t0)
            self.drain()
            if self.engine is not None:
                self._collect_stats()
        except BaseException as exc:
            self.error = exc
        finally:
            try:
                self.close()
            finally:
                self.done.put(self)


def run_ordered(workers: Sequence[Worker], items: Iterable, emit: Callable, orphan: Callable,
                admit: Optional[Callable] = None, discard: Optional[Callable] = None,
                closers: Sequence[Callable] = ()) -> None:
    """Deal ``items`` round-robin to ``workers`` and call ``emit(result)`` for every finished one, strictly in input
    order, on the collector thread.  ``orphan(result)`` gets every finished item that will never be emitted because
    something failed (buffers to hand back).  ``admit(failed)``, if given, is called before an item is dealt and may
    block (a budget); it must return once ``failed()`` is true.  ``discard(item)`` gets every item that was taken from
    ``items`` and never submitted after a failure: the one in the feed loop's hands and those left in the inboxes.  (An
    item a worker failed on, or had in flight when it failed, is nobody's: its buffers may still be the device's.)
    ``closers`` all run at the end, whatever happened.

    Raises the first error of: the item source or ``admit``, the collector (``emit``, a worker's error as it was
    reported, an item that went missing), a worker, a closer."""
    failure: List[BaseException] = []
    done: "queue.Queue" = queue.Queue()

    def collect():
        waiting, next_k, alive = {}, 0, len(workers)
        try:
            while alive or waiting:
                got = done.get()
                if isinstance(got, Worker):
                    alive -= 1
                    if got.error is not None:
                        raise got.error
                    if not alive and waiting:  # (what could be emitted has been: next_k is not among them)
                        raise RuntimeError(f"item {next_k} went missing between the GPU workers and the writers "
                                           f"({len(waiting)} later ones are waiting behind it)")
                    continue
                waiting[got[0]] = got[1]
                while next_k in waiting:
                    emit(waiting.pop(next_k))
                    next_k += 1
        except BaseException as exc:
            failure.append(exc)
            for k in sorted(waiting):
                orphan(waiting.pop(k))
            while alive:  # keep the workers from blocking on a dead consumer
                got = done.get()
                if isinstance(got, Worker):
                    alive -= 1
                else:
                    orphan(got[1])

    collector = threading.Thread(target=collect, daemon=True, name="cutseq-collect")
    for w in workers:
        w.done = done
        w.start()
    collector.start()
    errors, undealt = [], []  # in the order they win; items taken from the source that reached no inbox
    try:
        for k, item in enumerate(items):
            undealt.append(item)
            if admit is not None and not failure:
                admit(lambda: bool(failure))
            w = workers[k % len(workers)]
            while not failure:
                try:
                    w.inbox.put((k, item), timeout=0.2)
                    undealt.pop()
                    break
                except queue.Full:
                    continue
            if failure:
                break
    except BaseException as exc:
        errors.append(exc)
    for w in workers:
        while True:  # the sentinel must get in even when the worker died with a full inbox
            try:
                w.inbox.put(None, timeout=0.2)
                break
            except queue.Full:
                if not w.is_alive():
                    break
    for w in workers:
        w.join()
    collector.join()
    for w in workers:  # what a worker that failed left in its inbox
        while not w.inbox.empty():
            got = w.inbox.get()
            if got is not None:
                undealt.append(got[1])
    for item in undealt if discard is not None else ():
        discard(item)
    errors += failure
    errors += [w.error for w in workers if w.error is not None]
    for close in closers:
        try:
            close()
        except BaseException as exc:  # keep closing the others
            errors.append(exc)
    if errors:
        raise errors[0]
