"""numpy references of the device-side stream joiner (``smi_join_*``, sparkmi/audio.py: StreamJoiner).

Join.  A request's chunks c_0 .. c_{m-1}, overlap n, fade tables fi = linspace(0, 1, n), fo = linspace(1, 0, n) in float64, t the
last n samples of the previous chunk:

    c_0, the only chunk:    emits c_0                                 c_0, not last:       emits c_0[:L-n]
    c_i, i >= 1, not last:  emits fade(c_i[:n], t), c_i[n:L-n]        c_i, i >= 1, last:   emits fade(c_i[:n], t), c_i[n:]
    fade(a, t) = fl32(a * fi + t * fo)   (float64 products and sum, one rounding to fp32)

``joined`` evaluates that in float64 and casts to fp32; ``swap_fades`` and ``tail_shift`` build the wrong variants the tests must
tell apart.  Where every L >= 2n it is ``streaming.crossfade(chunks, n).astype(float32)``.

Streaming emission.  x is the joined stream, N samples after a push.  An output k is final once every input of its sum is there,
(k down + H) // up <= N - 1; ``emitted`` counts those by their definition (the closed form is max(0, ceil((N up - H) / down))).
After the last push all ceil(N up / down) outputs are out.  ``pieces`` is the emission built on ``resample_ref.emulate_fp32``: the
piece of push i is emulate_fp32(x[:N_i])[K_{i-1} : K_i] -- what a resampler that sees only the stream so far can say.  Its wrong
variants: ``early=1`` emits one output too soon (its sum then lacks samples that have not come yet) and ``short=1`` forgets the
oldest input sample each push still uses (a history one sample short; where that sample meets the end tap h[2H], which is a zero of
the windowed sinc, the next one; ``early`` likewise goes one output further where the first early one lacks only the sample under
h[0])."""
import numpy as np

import resample_ref as rr


def joined_lengths(lengths, n):
    """N after each push; the last chunk of ``lengths`` is the stream's last"""
    out, total = [], 0
    for i, L in enumerate(lengths):
        total += L if i == len(lengths) - 1 else L - n
        out.append(total)
    return out


def joined(chunks, n, swap_fades=False, tail_shift=0):
    """the joined stream of all chunks, fp32"""
    fi, fo = np.linspace(0, 1, n), np.linspace(1, 0, n)
    if swap_fades:
        fi, fo = fo, fi
    out, tail = [], None
    for i, c in enumerate(chunks):
        c = np.asarray(c, np.float32)
        last = i == len(chunks) - 1
        head = c[:n].astype(np.float64) * fi + tail.astype(np.float64) * fo if i and n else c[:0].astype(np.float64)
        if i == 0:
            body = c if last else c[: c.size - n]
        else:
            body = c[n:] if last else c[n: c.size - n]
        out += [head.astype(np.float32), body]
        if not last:
            tail = c[c.size - n - tail_shift: c.size - tail_shift]
    return np.concatenate(out).astype(np.float32) if out else np.zeros(0, np.float32)


def emitted(N, up, down, half, last):
    """outputs a stream of N samples has emitted, by definition: those whose whole sum is there (all of them after the last push)"""
    k = np.arange(rr.out_len(N, up, down), dtype=np.int64)
    if up == 1 and down == 1 or last:
        return int(k.size)
    return int(np.count_nonzero((k * down + half) // up <= N - 1))


def first_input(k, up, down, half):
    """the first input index of output k's sum"""
    return max(0, -((-(k * down - half)) // up))


def pieces(chunks, n, up, down, h, early=0, short=0):
    """[fp32 piece per push]: the streaming emission of the joined stream, the last chunk being the last push"""
    x = joined(chunks, n)
    Ns = joined_lengths([np.asarray(c).size for c in chunks], n)
    assert Ns[-1] == x.size if chunks else True
    half = (np.asarray(h).size - 1) // 2
    out, k_prev, n_prev = [], 0, 0
    for i, N in enumerate(Ns):
        last = i == len(Ns) - 1
        if up == 1 and down == 1:
            out.append(x[n_prev:N].copy())
            n_prev = N
            continue
        k = emitted(N, up, down, half, last)
        if not last and early:
            if k * down + half == N * up:   # output k lacks only the sample that meets the end tap h[0], a zero of the sinc
                k += 1                      # (1e-19): no bit depends on it, so the variant goes one further
            k = min(k + early, rr.out_len(N, up, down))
        seen = x[:N].copy()
        if short and k > k_prev and n_prev > 0:
            j = first_input(k_prev, up, down, half)
            if half + k_prev * down - j * up == 2 * half:   # that sample meets the end tap, a zero of the sinc (1e-19): no bit
                j += 1                                      # depends on it, so the variant forgets the next one
            seen[j] = 0.0
        y = rr.emulate_fp32(seen, up, down, h) if N else np.zeros(0, np.float32)
        out.append(y[k_prev:k].copy())
        k_prev, n_prev = k, N
    return out


def history_used(lengths, n, up, down, half):
    """per push that emits something: the input samples from before the push that its first output still reads"""
    used, k_prev, n_prev = [], 0, 0
    for i, N in enumerate(joined_lengths(lengths, n)):
        k = emitted(N, up, down, half, i == len(lengths) - 1)
        if k > k_prev:
            used.append(max(0, n_prev - first_input(k_prev, up, down, half)))
        k_prev, n_prev = k, N
    return used


def random_cuts(rng, total, n, m):
    """m chunk lengths of a stream whose joined length is ``total``: a chunk that is not the last has L >= 2n, the last one
    L >= n; each push adds n samples plus a random share (zero included) of the rest to the joined stream"""
    if m == 1:
        return [int(total)]
    spare = total - n * m
    assert spare >= 0
    cuts = np.sort(rng.integers(0, spare + 1, size=m - 1))
    add = np.diff(np.concatenate([[0], cuts, [spare]])).astype(np.int64) + n
    lengths = [int(a) + n for a in add[:-1]] + [int(add[-1])]
    assert joined_lengths(lengths, n)[-1] == total
    return lengths
