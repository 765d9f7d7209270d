"""Host side of park and resume: streaming.Pacer against a brute-force restatement of its rules under a fake clock, and
serve_stream's pacing validator.  No GPU."""
import itertools
import math

import numpy as np
import pytest

from sparkmi.pipeline import _stream_pacing
from sparkmi.streaming import Pacer


class Clock:
    def __init__(self):
        self.t = 100.0

    def __call__(self):
        return self.t


def _ref_lead(first, frames, key, now, rate):
    return -math.inf if key not in first else frames[key] / rate - (now - first[key])


def _ref_park(live, parked, pending, lead, max_batch, max_open, max_ahead):
    """The three rules, waiter by waiter.  Somebody waits: every parked request, and the pending one while fewer than max_open
    are open.  A waiter that a free row can serve costs nobody a row.  Each waiter beyond those takes the row of the live
    request with the largest lead (ties: the smaller key) among those whose lead exceeds max_ahead -- a request that has not
    spoken has lead -inf and never qualifies; the callers pass no finished request as live.  With no such request the waiter
    goes on waiting."""
    if max_ahead is None or max_open <= max_batch:
        return []
    waiting = [("parked", k) for k in parked]
    if pending and len(live) + len(parked) < max_open:
        waiting.append(("pending", None))
    free, out = max_batch - len(live), []
    for _ in waiting:
        if free > 0:
            free -= 1
            continue
        ok = [k for k in live if k not in out and lead[k] > max_ahead]
        if not ok:
            break
        out.append(max(ok, key=lambda k: (lead[k], -k)))
    return out


def _ref_resume(parked, free, urgent, lead, resume_ahead):
    c = sorted(parked, key=lambda k: (lead[k], k))
    if urgent:
        c = [k for k in c if lead[k] < resume_ahead]
    return c[: max(0, free)]


def test_lead_and_first_chunk():
    clk = Clock()
    p = Pacer(2, 5, 1.0, frame_rate=50, clock=clk)
    assert p.active and p.resume_ahead == 0.5
    assert p.lead(0) == -math.inf
    clk.t += 3.0                      # time before the first chunk does not count
    p.yielded(0, 100)
    assert p.lead(0) == 2.0
    clk.t += 0.5
    p.yielded(0, 25)
    assert p.lead(0) == 2.5 - 0.5
    clk.t += 10
    assert p.lead(0) == 2.5 - 10.5
    p.close(0)
    assert p.lead(0) == -math.inf


def test_decisions_match_the_restated_rules():
    rng = np.random.Generator(np.random.PCG64(7))
    parks = resumes = 0
    for trial in range(3000):
        max_batch = int(rng.integers(1, 5))
        max_open = int(rng.integers(1, 9))
        max_ahead = [None, 0.5, 2.0][int(rng.integers(0, 3))]
        resume = None if rng.integers(0, 2) or max_ahead is None else float(rng.uniform(0, max_ahead))
        clk = Clock()
        p = Pacer(max_batch, max_open, max_ahead, resume, frame_rate=50, clock=clk)
        keys = list(range(int(rng.integers(1, max(max_open, max_batch) + 1))))
        first, frames = {}, {}
        for k in keys:
            if rng.integers(0, 4):    # some have not spoken yet
                clk.t += float(rng.integers(0, 3)) * 0.25
                f = int(rng.integers(0, 16)) * 25         # quarter-second grid: ties happen
                p.yielded(k, f)
                first[k], frames[k] = clk.t, f
        clk.t += float(rng.integers(0, 8)) * 0.25
        lead = {k: _ref_lead(first, frames, k, clk.t, 50.0) for k in keys}
        assert all(p.lead(k) == lead[k] for k in keys)
        n_live = int(rng.integers(0, min(len(keys), max_batch) + 1))
        perm = rng.permutation(keys).tolist()
        live, parked = perm[:n_live], perm[n_live:]
        if not (max_ahead is not None and max_open > max_batch):
            parked = []               # an inert pacer never has parked requests
        pending = bool(rng.integers(0, 2))
        got = p.to_park(live, parked, pending)
        want = _ref_park(live, parked, pending, lead, max_batch, p.max_open, max_ahead)
        assert got == want, (trial, live, parked, lead)
        parks += len(got)
        for k in got:                 # each rule on its own
            assert lead[k] > max_ahead and lead[k] != -math.inf
            assert parked or (pending and len(live) + len(parked) < max_open)
        if parked:
            free = max_batch - len(live) + len(got)
            urgent = p.to_resume(parked, free, True)
            assert urgent == _ref_resume(parked, free, True, lead, p.resume_ahead)
            rest = [k for k in parked if k not in urgent]
            anyone = p.to_resume(rest, free - len(urgent), False)
            assert anyone == _ref_resume(rest, free - len(urgent), False, lead, p.resume_ahead)
            resumes += len(urgent) + len(anyone)
            # rows never idle while a parked request exists (no pending request admitted here)
            assert len(urgent) + len(anyone) == min(free, len(parked))
            assert not set(got) & set(urgent + anyone), "a row is never emptied to be handed straight back"
    assert parks > 20 and resumes > 20


def test_orderings_and_ties():
    clk = Clock()
    p = Pacer(3, 6, 1.0, 0.5, frame_rate=50, clock=clk)
    for k, f in ((0, 150), (1, 150), (2, 100), (3, 10), (4, 20)):
        p.yielded(k, f)               # leads 3, 3, 2, 0.2, 0.4 at the same clock
    assert p.to_park([2, 1, 0], [3, 4], False) == [0, 1]            # largest lead first, ties by key, two waiters
    assert p.to_park([2, 1, 0], [3], False) == [0]
    assert p.to_park([2, 1, 0], [], True) == [0]                    # a pending request and room to open it
    assert p.to_park([2, 1, 0], [], False) == []                    # nobody waits
    assert p.to_park([2, 1], [3], False) == []                      # the free row serves the waiter
    assert p.to_park([5, 2], [3, 4], False) == [2]                  # 5 has not spoken: never parked
    assert p.to_resume([4, 3, 2], 2, True) == [3, 4]                # smallest lead first, only those below resume_ahead
    assert p.to_resume([4, 3, 2], 3, True) == [3, 4]
    assert p.to_resume([2, 0, 1], 2, False) == [2, 0]
    assert p.to_resume([2], 0, False) == []
    full = Pacer(3, 5, 1.0, clock=clk)
    for k in range(5):
        full.yielded(k, 500)
    assert full.to_park([0, 1, 2], [], True) == [0]
    assert full.to_park([0, 1], [3, 4, 5], True) == [0, 1]          # max_open reached: the pending one does not count, the parked do
    assert (p.parks, p.resumes) == (5, 6)


@pytest.mark.parametrize("kw", [dict(max_open=None, max_ahead=0.1), dict(max_open=3, max_ahead=0.1), dict(max_open=2, max_ahead=0.1),
                                dict(max_open=8, max_ahead=None)])
def test_inert(kw):
    clk = Clock()
    p = Pacer(3, clock=clk, **kw)
    assert not p.active
    for k in range(3):
        p.yielded(k, 10000)
    for live, pending in itertools.product(([0, 1, 2], [0], []), (False, True)):
        assert p.to_park(live, [], pending) == []
    assert p.parks == 0


def test_validator():
    assert _stream_pacing(4) == (4, None, None)
    assert _stream_pacing(4, 9, 2.0) == (9, 2.0, 1.0)
    assert _stream_pacing(4, 9, 2, 0) == (9, 2.0, 0.0)
    assert _stream_pacing(4, 9, 2.0, 2.0) == (9, 2.0, 2.0)
    assert _stream_pacing(4, None, 0.5) == (4, 0.5, 0.25)            # accepted and inert
    assert _stream_pacing(4, 2, 0.5) == (2, 0.5, 0.25)
    assert _stream_pacing(4, np.int64(6), np.float32(1.0))[0] == 6
    for bad in (dict(max_open=0), dict(max_open=-3), dict(max_open=2.5), dict(max_open=True), dict(max_open="5"),
                dict(max_open=8, max_ahead=0), dict(max_open=8, max_ahead=-1.0), dict(max_open=8, max_ahead=float("nan")),
                dict(max_open=8, max_ahead=float("inf")), dict(max_open=8, max_ahead="1"),
                dict(max_open=8, max_ahead=1.0, resume_ahead=-0.1), dict(max_open=8, max_ahead=1.0, resume_ahead=1.5),
                dict(max_open=8, resume_ahead=-1.0)):
        with pytest.raises(ValueError):
            _stream_pacing(4, **bad)
    for bad in (dict(max_batch=0), dict(max_batch=2, max_open=4, max_ahead=0.0), dict(max_batch=2, max_open=4, max_ahead=1.0, resume_ahead=2.0)):
        with pytest.raises(ValueError):
            Pacer(**bad)
