"""
ProjectionFarm.map() left early, on CPU workers (tests/farm_cpu_worker.py): a ``break``, an exception from the consumer or
from the iterator ends the generator while projections are still with the workers.  Whatever way it ends, the farm's books
are clean afterwards -- nothing in flight, every slot free -- and the next ``map()`` on the same farm hands out its own
projections only.  (A ``map()`` that ended early used to leave its results in the queue: the next call yielded them under
their old ids and never handed out its own.)
"""
import functools
import time

import numpy as np
import pytest

import farm_cpu_worker

NW, MS, DEPTH = 2, 3, 2
SCALES = (1.0, 0.9, 0.8, 0.7, 0.6, 0.5)       # six projections, no two alike: a stale map cannot pass for the right one
KEYS = ("f", "T", "dx", "dy", "df", "err")


class _ConsumerError(Exception):
    pass


@pytest.fixture(scope="module")
def stack():
    from oracle import cpu_model
    from umpa_amd.synth import make_stack
    cpu_model.native("port")
    sam, ref, _ = make_stack(40, 44, 3, MS, df=True, seed=7, amplitude=1.0)
    return sam, ref


def _want(sam, ref):
    from oracle import cpu_model
    return cpu_model.port.UMPAModelDF(sam, ref, window_size=NW, max_shift=MS).match(quiet=True, num_threads=1)


def _books_are_clean(farm):
    assert [w["inflight"] for w in farm._workers] == [0] * len(farm._workers)
    assert not farm._by_seq and not farm._held
    for w in farm._workers:
        assert sorted(w["free_in"]) == list(range(DEPTH)) and sorted(w["free_out"]) == list(range(DEPTH))


def _take_one_and_leave(farm, items, how):
    """The first result of ``farm.map(items)``; the generator is then left by ``how`` and closed."""
    gen = farm.map(items, timeout=60.0, num_threads=1)
    first = []
    try:
        if how == "break":
            for pid, res in gen:
                first.append((pid, res))
                break
        else:
            with pytest.raises(_ConsumerError):
                for pid, res in gen:
                    first.append((pid, res))
                    raise _ConsumerError("the consumer gave up")
    finally:
        gen.close()
    assert len(first) == 1
    return first[0]


def _second_map_is_its_own(farm, sam, ref):
    """Two further projections under ids the abandoned series used: exactly these two come back, each with the maps of
    its own input, and the call does not wait for its time limit."""
    again = {0: np.ascontiguousarray(0.95 * sam), 5: np.ascontiguousarray(0.85 * sam)}
    t0 = time.time()
    seen = []
    for pid, res in farm.map(again.items(), timeout=60.0, num_threads=1):
        seen.append(pid)
        assert pid in again, "a projection of the earlier series was handed out under id %r" % (pid,)
        want = _want(again[pid], ref)
        for k in KEYS:
            np.testing.assert_array_equal(res[k], want[k], err_msg="id %r, %s" % (pid, k))
    assert sorted(seen) == [0, 5]
    assert time.time() - t0 < 60.0
    _books_are_clean(farm)


@pytest.mark.parametrize("how", ["break", "consumer raises"])
def test_map_abandoned_then_reused(stack, how):
    from umpa_amd.farm import ProjectionFarm
    sam, ref = stack
    items = [(p, np.ascontiguousarray(s * sam)) for p, s in enumerate(SCALES)]
    with ProjectionFarm(ref, NW, MS, devices=[None, None], worker=farm_cpu_worker.run, depth=DEPTH) as farm:
        pid, res = _take_one_and_leave(farm, items, how)
        np.testing.assert_array_equal(res["T"], _want(items[pid][1], ref)["T"])
        _books_are_clean(farm)
        _second_map_is_its_own(farm, sam, ref)


@pytest.mark.parametrize("how", ["break", "consumer raises"])
def test_map_abandoned_with_a_failure_in_flight(stack, how):
    """Projections 2 and 3 fail in their workers.  Each is the second task of its worker, so the first result handed out is
    projection 0 or 1, and at that moment both failures are still in flight (with their worker, or as messages in the
    queue): the clean-up meets them, and no ProjectionFailed comes out of it."""
    from umpa_amd.farm import ProjectionFarm
    sam, ref = stack
    items = [(p, np.ascontiguousarray(s * sam)) for p, s in enumerate(SCALES)]
    worker = functools.partial(farm_cpu_worker.run, fail_pids=(2, 3))
    with ProjectionFarm(ref, NW, MS, devices=[None, None], worker=worker, depth=DEPTH) as farm:
        pid, res = _take_one_and_leave(farm, items, how)          # (a ProjectionFailed from the clean-up would surface here)
        assert pid in (0, 1)
        np.testing.assert_array_equal(res["T"], _want(items[pid][1], ref)["T"])
        _books_are_clean(farm)
        _second_map_is_its_own(farm, sam, ref)


def test_map_whose_iterator_raises(stack):
    """The iterator fails after four projections were submitted: the input slot taken for the fifth goes back, the four
    are collected, and the farm serves the next map()."""
    from umpa_amd.farm import ProjectionFarm
    sam, ref = stack

    def items():
        for p, s in enumerate(SCALES[:4]):
            yield p, np.ascontiguousarray(s * sam)
        raise _ConsumerError("the producer gave up")

    with ProjectionFarm(ref, NW, MS, devices=[None, None], worker=farm_cpu_worker.run, depth=DEPTH) as farm:
        with pytest.raises(_ConsumerError):
            list(farm.map(items(), timeout=60.0, num_threads=1))
        _books_are_clean(farm)
        _second_map_is_its_own(farm, sam, ref)
