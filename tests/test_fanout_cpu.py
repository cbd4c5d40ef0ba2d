"""The ordered fan-out (cutseq_amd/fanout.py) without a GPU: fake workers on the real base class, whose "engine" is a
Python object that records its calls and finishes an item when the test lets it.  What goes wrong here goes wrong as a
hang, so every run happens in a helper thread that must be over within 10 s and must leave no ``cutseq-*`` thread."""
import threading

from cutseq_amd import fanout

BOUND = 10.0


class Boom(Exception):
    pass


class Item:
    def __init__(self, k, gate=None, opens=None, rebuild=False):
        self.k, self.gate, self.opens, self.rebuild = k, gate, opens, rebuild


class FakeStats:
    def __init__(self, d):
        self.d = d

    def as_dict(self):
        return dict(self.d)


class FakeEngine:
    def __init__(self, log):
        self.log, self.submits, self.closed = log, 0, False

    def submit(self, slot, item):
        self.log.append(("submit", slot, item.k))
        self.submits += 1
        return item

    def wait(self, slot, item):
        if item.gate is not None:
            assert item.gate.wait(BOUND), f"item {item.k} was never let go"
        self.log.append(("wait", slot, item.k))

    def stats(self):
        return [FakeStats({"reads": self.submits, "per_op": [self.submits, 1]})]

    def close(self):
        self.closed = True


class FakeWorker(fanout.Worker):
    """``submit_raises`` / ``finish_raises``: the k of the item at which that call fails; ``loses``: the k of an item
    that is finished and never reported; ``before_raise``: waited for before ``submit_raises`` takes effect."""

    def __init__(self, i, finished, submit_raises=None, finish_raises=None, loses=None, before_raise=None):
        super().__init__(f"cutseq-fake{i}")
        self.finished, self.log, self.closed = finished, [], False
        self.submit_raises, self.finish_raises, self.loses, self.before_raise = submit_raises, finish_raises, loses, before_raise

    def begin(self):
        self.engine = FakeEngine(self.log)

    def ensure(self, item):
        if item.rebuild:
            self.drain()
            self._collect_stats()
            self.engine.close()
            self.engine = FakeEngine(self.log)

    def submit(self, slot, item):
        if item.k == self.submit_raises:
            if self.before_raise is not None:
                assert self.before_raise.wait(BOUND)
            raise Boom(f"submit of item {item.k}")
        return self.engine.submit(slot, item)

    def finish(self, slot, item):
        self.engine.wait(slot, item)
        if item.k == self.finish_raises:
            raise Boom(f"finish of item {item.k}")
        if item.opens is not None:
            item.opens.set()
        self.finished.append(item.k)
        return item

    def _finish_oldest(self):
        if self.inflight[0][0] == self.loses:
            self.inflight.popleft()
        else:
            super()._finish_oldest()

    def close(self):
        self.closed = True


class Run:
    """One bounded run of ``fanout.run_ordered`` -> what was emitted, orphaned, discarded and raised."""

    def __init__(self, workers, items, emit_raises=None, before_emit_raises=None, on_emit=None, admit=None, closers=()):
        self.emitted, self.orphaned, self.discarded, self.error = [], [], [], None

        def emit(item):
            if item.k == emit_raises:
                if before_emit_raises is not None:
                    assert before_emit_raises.wait(BOUND)
                raise Boom(f"emit of item {item.k}")
            self.emitted.append(item.k)
            if on_emit is not None:
                on_emit()

        def target():
            try:
                fanout.run_ordered(workers, items, emit, lambda item: self.orphaned.append(item.k), admit=admit,
                                   discard=lambda item: self.discarded.append(item.k), closers=closers)
            except BaseException as exc:
                self.error = exc

        t = threading.Thread(target=target, daemon=True, name="fanout-test-run")
        t.start()
        t.join(BOUND)
        assert not t.is_alive(), "run_ordered did not return"
        assert [th.name for th in threading.enumerate() if th.name.startswith("cutseq-")] == []


def closers(n, raises=()):
    ran = []

    def make(i):
        def close():
            ran.append(i)
            if i in raises:
                raise OSError(f"closer {i}")
        return close

    return ran, [make(i) for i in range(n)]


def test_emits_in_input_order_whatever_order_the_workers_finish_in():
    """Worker 0 cannot finish item 0 before worker 2 has finished item 2."""
    finished = []
    two_done = threading.Event()
    items = [Item(k, gate=two_done if k == 0 else None, opens=two_done if k == 2 else None) for k in range(40)]
    workers = [FakeWorker(i, finished) for i in range(3)]
    run = Run(workers, items)
    assert run.error is None
    assert run.emitted == list(range(40)) and run.orphaned == []
    assert sorted(finished) == list(range(40)) and finished.index(2) < finished.index(0)
    assert [sorted(k for op, _, k in w.log if op == "submit") for w in workers] == [list(range(i, 40, 3)) for i in range(3)]
    assert all(w.closed and w.error is None for w in workers)


def test_a_workers_error_is_raised_and_what_finished_is_emitted_or_orphaned():
    finished = []
    workers = [FakeWorker(i, finished, submit_raises=7 if i == 1 else None) for i in range(3)]  # worker 1: items 1, 4, 7
    ran, cl = closers(3)
    run = Run(workers, [Item(k) for k in range(40)], closers=cl)
    assert isinstance(run.error, Boom) and str(run.error) == "submit of item 7" and run.error is workers[1].error
    assert ran == [0, 1, 2]
    assert run.emitted == list(range(len(run.emitted)))  # a prefix, in order
    assert sorted(run.emitted + run.orphaned) == sorted(finished)
    assert 7 not in finished and all(w.closed for w in workers)


def test_a_worker_that_died_with_a_full_inbox_does_not_hold_the_shutdown_up():
    finished = []
    inbox_full = threading.Event()
    worker = FakeWorker(0, finished, submit_raises=0, before_raise=inbox_full)

    def source():
        for k in range(100):
            if k == 1 + worker.SLOTS:  # item 0 is with the worker, the next SLOTS are in its inbox
                assert worker.inbox.full()
                inbox_full.set()
            yield Item(k)

    run = Run([worker], source())
    assert isinstance(run.error, Boom) and str(run.error) == "submit of item 0"
    assert worker.closed and worker.inbox.empty()
    assert run.emitted == [] and run.orphaned == []
    assert sorted(run.discarded) == [1, 2, 3]  # what was in the inbox, and the item the feed loop could not get in


def test_the_sources_error_wins_over_a_later_workers():
    finished = []
    workers = [FakeWorker(i, finished, finish_raises=3 if i == 1 else None) for i in range(2)]  # item 3: finished at the drain

    def source():
        for k in range(100):
            if k == 5:
                raise ValueError("source at item 5")
            yield Item(k)

    ran, cl = closers(2)
    run = Run(workers, source(), closers=cl)
    assert isinstance(run.error, ValueError) and str(run.error) == "source at item 5"
    assert isinstance(workers[1].error, Boom)  # ... which happened, and lost
    assert all(w.closed and not w.is_alive() for w in workers) and ran == [0, 1]
    assert sorted(k for w in workers for op, _, k in w.log if op == "submit") == [0, 1, 2, 3, 4]
    assert sorted(run.emitted + run.orphaned) == sorted(finished)


def test_emits_error_is_raised_the_rest_is_orphaned_and_a_blocked_admit_returns():
    finished = []
    workers = [FakeWorker(i, finished) for i in range(2)]
    budget = threading.Semaphore(2 * 2 * FakeWorker.SLOTS + 2)
    blocked, gave_up = threading.Event(), []

    def admit(failed):
        while not budget.acquire(timeout=0.05):
            blocked.set()
            if failed():
                gave_up.append(True)
                return

    # every emitted item gives its share of the budget back, as a writer does; an orphaned one here does not, so that
    # the feed loop is stuck in admit() when emit fails (emit waits for that before it raises)
    taken = []

    def source():
        for k in range(100):
            taken.append(k)
            yield Item(k)

    run = Run(workers, source(), emit_raises=7, before_emit_raises=blocked, on_emit=budget.release, admit=admit)
    assert isinstance(run.error, Boom) and str(run.error) == "emit of item 7"
    assert run.emitted == list(range(7)) and gave_up == [True]
    assert sorted(run.emitted + [7] + run.orphaned) == sorted(finished)
    assert len(run.orphaned) > 0 and all(w.closed for w in workers)
    assert sorted(finished + run.discarded) == taken and len(taken) < 100  # nothing taken from the source is left lying


def test_a_closers_error_is_raised_last_and_stops_no_other_closer():
    ran, cl = closers(4, raises=(1, 2))
    run = Run([FakeWorker(i, []) for i in range(2)], [Item(k) for k in range(6)], closers=cl)
    assert isinstance(run.error, OSError) and str(run.error) == "closer 1"
    assert ran == [0, 1, 2, 3] and run.emitted == list(range(6))

    ran, cl = closers(4, raises=(1,))
    workers = [FakeWorker(i, [], submit_raises=3 if i == 1 else None) for i in range(2)]
    run = Run(workers, [Item(k) for k in range(6)], closers=cl)
    assert isinstance(run.error, Boom) and run.error is workers[1].error
    assert ran == [0, 1, 2, 3]


def test_an_item_no_worker_reported_is_named():
    finished = []
    workers = [FakeWorker(i, finished, loses=4 if i == 0 else None) for i in range(2)]
    run = Run(workers, [Item(k) for k in range(12)])
    assert isinstance(run.error, RuntimeError) and "item 4 went missing" in str(run.error)
    assert all(w.error is None for w in workers)  # both ended cleanly
    assert run.emitted == [0, 1, 2, 3] and sorted(run.orphaned) == list(range(5, 12))


def test_slots_are_reused_oldest_first_and_a_rebuilt_engines_stats_are_kept():
    assert FakeWorker.SLOTS == 2
    worker = FakeWorker(0, [])
    run = Run([worker], [Item(k, rebuild=k == 5) for k in range(8)])
    assert run.error is None and run.emitted == list(range(8))
    third = worker.log.index(("submit", 0, 2))
    assert worker.log[:third] == [("submit", 0, 0), ("submit", 1, 1), ("wait", 0, 0)]  # one finish, of the oldest: its slot
    for at, entry in enumerate(worker.log):  # every submit takes a slot nothing is in flight on
        if entry[0] == "submit":
            busy = [s for op, s, k in worker.log[:at] if op == "submit" and ("wait", s, k) not in worker.log[:at]]
            assert entry[1] not in busy and len(busy) < FakeWorker.SLOTS
    # the rebuild for item 5 drained items 3 and 4 first; the first engine counted 5 submits, the second 3
    rebuilt = next(at for at, entry in enumerate(worker.log) if entry[0] == "submit" and entry[2] == 5)
    assert [k for op, _, k in worker.log[:rebuilt] if op == "wait"] == [0, 1, 2, 3, 4]
    assert worker.stats == [{"reads": 8, "per_op": [8, 2]}]
    assert worker.engine.closed is False and worker.closed
