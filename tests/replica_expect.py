"""Replicated-resample helpers of the GPU parity tests: a few distinct resamples spread over many slots, so that a
slot computed from the wrong operand, group or split shows as a replica that differs from its twins.  Shared by
tests/test_gpu_timed_geometry.py and tests/test_gpu_boot_followers.py; not a test module."""
import numpy as np


def slot_map(n, nd, boundaries, seed):
    """slot -> distinct resample: seeded random, every distinct one used, and different resamples on the two sides
    of every boundary b (slots b - 1 and b) and in the first and last slot."""
    rs = np.random.RandomState(seed)
    which = rs.randint(nd, size=n)
    which[:nd] = rs.permutation(nd)                     # (every distinct resample at least once)
    rs.shuffle(which)
    for b in sorted(set(boundaries) | {n - 1}):
        if 0 < b < n and which[b] == which[b - 1]:
            taken = {which[b - 1]} | ({which[b + 1]} if b + 1 < n else set())
            which[b] = min(set(range(nd)) - taken)
    assert which[0] != which[-1] and len(np.unique(which)) == nd
    for b in boundaries:
        assert which[b] != which[b - 1], b
    return which


def rel_per_column(a, b):
    """max |a - b| / max |b| of every trailing-axis column."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    axes = tuple(range(a.ndim - 1))
    return np.max(np.abs(a - b), axis=axes) / np.max(np.abs(b), axis=axes)


def assert_replicas(vals, which, rtol, what):
    """vals (n, ...): slots that hold the same resample agree to rtol of that resample's own scale (per LV when the
    last axis is the LV axis)."""
    for d in np.unique(which):
        slots = np.flatnonzero(which == d)
        v = vals[slots]
        err = np.max(np.abs(v - v[:1]), axis=tuple(range(v.ndim - 1)))
        scale = np.max(np.abs(v[0]), axis=tuple(range(v.ndim - 2))) if v.ndim > 2 else np.abs(v[0])
        bad = err > rtol * scale
        assert not np.any(bad), '{}: resample {} differs between its slots {} (LVs {}, max rel err {:.3e})'.format(
            what, d, slots[np.argmax(np.max(np.abs(v - v[:1]).reshape(len(slots), -1), axis=1))],
            np.flatnonzero(bad), float(np.max(err / scale)))


def synth(S, B, T, seed=0):
    """bench.py synth() -- X = randn(S, B), Y = randn(S, T) + 0.3 X[:, :T] -- also where B < T (the signal then goes
    into the first B behaviours only; the same draws and values as bench.py's wherever B >= T)."""
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    Y = rs.randn(S, T)
    k = min(T, B)
    Y[:, :k] = Y[:, :k] + 0.3 * X[:, :k]
    return X, Y
