"""``engine.quiet_gc``: what every hipGraph capture of the package runs under.  Python's cyclic collector is emptied before the capture and held off
until the last capture under way has ended (ranks emulated by threads capture side by side), then put back as it was."""
import gc
import threading

from gptst_amd import engine


class _Cycle:
    def __init__(self, log):
        self.me, self.log = self, log

    def __del__(self):
        self.log.append(gc.isenabled())


def test_dead_cycles_go_before_the_capture_and_none_is_collected_inside():
    assert gc.isenabled()
    log = []
    _Cycle(log)
    with engine.quiet_gc():
        assert log == [True] and not gc.isenabled()          # collected on entry, with the collector still on
        _Cycle(log)
        for _ in range(3):
            [[] for _ in range(5000)]                         # allocations that would start a young-generation collection
        assert log == [True]
        with engine.quiet_gc():
            assert not gc.isenabled()
        assert not gc.isenabled() and log == [True]
    assert gc.isenabled()
    gc.collect()
    assert log == [True, True]


def test_a_collector_that_was_off_stays_off_and_threads_share_the_hold():
    gc.disable()
    try:
        with engine.quiet_gc():
            pass
        assert not gc.isenabled()
    finally:
        gc.enable()
    inside, leave = threading.Event(), threading.Event()

    def other():
        with engine.quiet_gc():
            inside.set()
            leave.wait(10)
    t = threading.Thread(target=other)
    t.start()
    assert inside.wait(10)
    with engine.quiet_gc():
        pass
    assert not gc.isenabled()                                 # the other thread's capture is still under way
    leave.set()
    t.join()
    assert gc.isenabled()
