"""Plain-Python restatement of include/sparkmi.h's "when a frame is final" (smi_tempos_*): how many output samples a tempo stream
has emitted once it holds n input samples.  The samples themselves are stated once, in tests/tempo_ref.py: ``stream`` cuts
``tempo_ref.tempo`` of the whole input into the pieces the rule allows."""
import numpy as np

import tempo_ref as tr


def nominal(k, p, q, H):
    return (k * H * p) // q


def ready(k, p, q, N, D):
    """R_k: the input samples after which frame k can no longer change"""
    H = N // 2
    if k == 0:
        return H
    return max(nominal(k, p, q, H), nominal(k - 1, p, q, H) + H) + D + N


def frames(n, p, q, N, D, last):
    """frames emitted by a stream that holds n samples (all K of them after the last push)"""
    H = N // 2
    M = -((-n * q) // p)
    if last:
        return (M - 1) // H + 1 if M else 0
    if p == q:
        return n // H
    f = 0
    while (f + 1) * H <= M and n >= ready(f, p, q, N, D):
        f += 1
    return f


def emitted(n, p, q, N, D, last):
    """E(n): outputs emitted so far; M after the last push; everything at once at p = q"""
    n, p, q, N, D = int(n), int(p), int(q), int(N), int(D)
    if last:
        return -((-n * q) // p)
    if p == q:
        return n
    return frames(n, p, q, N, D, False) * (N // 2)


def history_start(f, p, q, N, D):
    """the first input sample frame f can still read"""
    H = N // 2
    if f == 0:
        return 0
    return max(0, min(nominal(f, p, q, H), nominal(f - 1, p, q, H) + H) - D)


def lengths_after(cuts):
    """n after every push of the given lengths"""
    return np.cumsum(np.asarray(cuts, dtype=np.int64)).tolist()


def stream(x, cuts, p, q, N, D):
    """(pieces, places): ``tempo_ref.tempo(x, ...)`` cut where a stream pushed in chunks of ``cuts`` samples (they sum to
    x.size; the last push is the stream's last) emits it, and per push the places of the frames it made final"""
    x = np.asarray(x, dtype=np.float32)
    assert sum(cuts) == x.size
    out, s = tr.tempo(x, p, q, N, D)
    pieces, places, e0, f0 = [], [], 0, 0
    for i, n in enumerate(lengths_after(cuts)):
        last = i == len(cuts) - 1
        e1, f1 = emitted(n, p, q, N, D, last), frames(n, p, q, N, D, last)
        pieces.append(out[e0:e1])
        places.append(s[f0:f1])
        e0, f0 = e1, f1
    assert e0 == out.size and f0 == s.size
    return pieces, places
