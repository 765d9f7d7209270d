"""Plain-Python restatement of include/sparkmi.h's "When an output is final" (smi_pitchs_*): how many final outputs a pitch stream
has emitted once it holds n input samples, and where the stretched tail it keeps begins.  The samples themselves are stated
once, in tests/pitch_ref.py: ``stream`` cuts ``pitch_ref.pitch`` of the whole input into the pieces the rule allows.

With t = (tp, tq), r = (rp, rq), the stretch P / Q and the resampling up / down of ``pitch_ref.plan`` and taps h[0 .. 2G]
(G = 10 max(up, down) for ``resample_taps``; 0 at up = down = 1):

    E(n) = tempo_stream_ref.emitted(n, P, Q, N, D)              stretched samples emitted
    K(n) = max(0, ceil((E(n) up - G) / down))                   final outputs, while the stream goes on
    K    = ceil(L tq / tp)                                      after the last push
    tail = z[max(0, ceil((K down - G) / up)) .. E)              what the outputs still to come reach of what is emitted

``wrong="reach"`` is the variant the tests must tell apart: it emits ceil(E up / down) outputs, ignoring the filter's reach."""
import numpy as np

import pitch_ref as pr
import tempo_stream_ref as ts


def half(up, down):
    """G of ``resample_taps(up, down)``; no filter at 1/1"""
    return 0 if (up, down) == (1, 1) else 10 * max(up, down)


def n_taps(t, r, N=16):
    pl = pr.plan(0, t, r, N)
    G = half(pl["up"], pl["down"])
    return 2 * G + 1 if G else 0


def frames(n, t, r, N, D, last):
    """frames of the stretch emitted by a stream that holds n samples"""
    pl = pr.plan(0, t, r, N)
    return ts.frames(int(n), pl["P"], pl["Q"], N, D, last)


def stretched(n, t, r, N, D, last):
    """E(n); M after the last push"""
    pl = pr.plan(0, t, r, N)
    return ts.emitted(int(n), pl["P"], pl["Q"], N, D, last)


def emitted(n, t, r, N, D, last, wrong=None):
    """K(n): final outputs emitted so far; n_out after the last push"""
    n = int(n)
    if last:
        return -((-n * int(t[1])) // int(t[0]))
    pl = pr.plan(0, t, r, N)
    up, down = pl["up"], pl["down"]
    E = stretched(n, t, r, N, D, False)
    if wrong == "reach":
        return -((-E * up) // down)
    assert wrong is None
    return max(0, -((-(E * up - half(up, down))) // down))


def tail_start(K, t, r, N=16):
    """the first stretched sample output K reaches: where the stored tail of a stream that has emitted K outputs begins"""
    pl = pr.plan(0, t, r, N)
    up, down = pl["up"], pl["down"]
    return max(0, -((-(int(K) * down - half(up, down))) // up))


def tail_bound(t, r, N=16):
    """ceil((2 G + down) / up) + 1: smi_join's bound on such a tail (the header's own, 2 G / up, is below it)"""
    pl = pr.plan(0, t, r, N)
    up, down = pl["up"], pl["down"]
    return -((-(2 * half(up, down) + down)) // up) + 1


def stream(x, cuts, t, r, N, D, wrong=None):
    """(pieces, places): ``pitch_ref.pitch(x, ...)`` cut where a stream pushed in chunks of ``cuts`` samples (they sum to x.size;
    the last push is the stream's last) emits it, and per push the places of the stretch's frames it made final"""
    x = np.asarray(x, dtype=np.float32)
    assert sum(cuts) == x.size
    out, s = pr.pitch(x, t, r, N, D)
    pieces, places, e0, f0 = [], [], 0, 0
    for i, n in enumerate(ts.lengths_after(cuts)):
        last = i == len(cuts) - 1
        e1, f1 = emitted(n, t, r, N, D, last, wrong), frames(n, t, r, N, D, last)
        pieces.append(out[e0:e1])
        places.append(s[f0:f1])
        e0, f0 = e1, f1
    assert e0 == out.size and f0 == s.size
    return pieces, places
