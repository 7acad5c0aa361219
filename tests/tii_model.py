"""Transmitter identification (include/dabhip.h, "TII") restated in plain numpy and Python integers: the patterns and carriers, the counting rule,
the de-rotated fixed-point 2048-point transform and the exact fold that the GPU's sums are compared with bit for bit, and the rule that turns the
sums into identifiers (Python integers throughout: no width to overflow).  Written from the header's text.  Only the NCO table is taken from the
library (dab.ingest_tune_nco): test_tune_model.py holds it to its conditions."""
import functools

import numpy as np

import dabtools_amd as dab

S = 2048
REV = np.array([int(format(i, "011b")[::-1], 2) for i in range(S)])
PATTERNS = [w for w in range(256) if bin(w).count("1") == 4]
QUARTERS = (-768, -384, 1, 385)
SHADOW = 1
W0, MAX_SHIFT = 304, 304
NULL_SAMPLES, TF_SAMPLES = 2656, 196608


def carriers(p, c):
    """The 32 carriers of transmitter (p, c): quarter after quarter, ascending within each."""
    out = []
    for base in QUARTERS:
        for b in range(8):
            if PATTERNS[p] >> (7 - b) & 1:
                out += [base + 2 * c + 48 * b, base + 2 * c + 48 * b + 1]
    return out


@functools.lru_cache(maxsize=None)
def slot_of_bin():
    """bin of the transform -> 8 c + b, -1 where no carrier lies."""
    slot = np.full(S, -1)
    for c in range(24):
        for b in range(8):
            for base in QUARTERS:
                for e in (0, 1):
                    slot[(base + 2 * c + 48 * b + e) % S] = 8 * c + b
    return slot


@functools.lru_cache(maxsize=None)
def nco():
    cs = dab.ingest_tune_nco().astype(np.int64)
    return cs[:, 0], cs[:, 1]


def counted(ok, fine_timeshift, fine_freq_shift):
    """Step 1: does a call count?"""
    return bool(ok) and abs(int(fine_timeshift)) <= MAX_SHIFT and abs(float(fine_freq_shift)) < 1024000.0


def step_of(coarse_freq_shift, fine_freq_shift, nco_hz=0):
    """Step 3's step: doubles, left to right."""
    f = 1000.0 * int(coarse_freq_shift) + float(fine_freq_shift) + float(int(nco_hz))
    return int(np.rint(f * 4294967296.0 / 2048000.0)) % (1 << 32)


def derotate(window, step, wide=False):
    """Steps 2 and 3 on windows [n][2048][2] of bytes with one step each -> y [n][2048][2]."""
    kind = object if wide else np.int64
    x = ((np.asarray(window).astype(np.int64) - 127) * 128).astype(kind)
    step = np.asarray(step, dtype=np.uint64).reshape(-1, 1)
    theta = (step * np.arange(S, dtype=np.uint64)) % np.uint64(1 << 32)
    i = (((theta + np.uint64(1 << 19)) % np.uint64(1 << 32)) >> np.uint64(20)).astype(np.int64)
    c, s = (t.astype(kind) for t in nco())
    return np.stack([(x[..., 0] * c[i] + x[..., 1] * s[i] + 8192) >> 14, (x[..., 1] * c[i] - x[..., 0] * s[i] + 8192) >> 14], axis=-1)


def transform(y, watch=None, wide=False):
    """Step 4 on [n][2048][2] -> X [n][2048][2], int64 (wide: Python integers in object arrays).  watch: a list that receives, first for the input
    and then after every stage, (the largest magnitude of a rail, the largest magnitude of a product sum of that stage with its 8192)."""
    kind = object if wide else np.int64
    y = np.asarray(y).astype(kind)
    n = y.shape[0]
    c, s = (t.astype(kind) for t in nco())
    v = y[:, REV, :]
    if watch is not None:
        watch.append((int(np.abs(v).max()), 0))
    h = 1
    while h < S:
        v = v.reshape(n, S // (2 * h), 2, h, 2)
        a, b = v[:, :, 0], v[:, :, 1]
        t = np.arange(h) * (2048 // h)
        pi = b[..., 0] * c[t] + b[..., 1] * s[t] + 8192
        pq = b[..., 1] * c[t] - b[..., 0] * s[t] + 8192
        tw = np.stack([pi >> 14, pq >> 14], axis=-1)
        v = np.stack([(a + tw + 1) >> 1, (a - tw + 1) >> 1], axis=2).reshape(n, S, 2)
        if watch is not None:
            watch.append((int(np.abs(v).max()), int(max(np.abs(pi).max(), np.abs(pq).max()))))
        h *= 2
    return v


def fold(X):
    """Step 6 of spectra [n][2048][2]: uint64 [n][192], one T per window."""
    p = (X * X).sum(axis=2)
    T = np.zeros((X.shape[0], 192), np.int64)
    slot = slot_of_bin()
    for k in np.nonzero(slot >= 0)[0]:
        T[:, slot[k]] += p[:, k]
    return T.astype(np.uint64)


def window_sums(window, step):
    """Steps 2 - 6: windows [n][2048][2] of bytes, one step each -> uint64 [n][192]."""
    window = np.asarray(window)
    if window.shape[0] == 0:
        return np.zeros((0, 192), np.uint64)
    return fold(transform(derotate(window, step)))


def frame_sums(frames, w0, step):
    """The stage entry: contiguous frames (bytes) with a window start and a step each."""
    frames = np.asarray(frames, dtype=np.uint8).reshape(len(w0), TF_SAMPLES, 2)
    return window_sums(np.stack([f[int(a):int(a) + S] for f, a in zip(frames, w0)]), step)


def aligned_capture_sums(iq, ntf, fine=0, step=0):
    """T of a capture whose frames lie back to back from its first sample on: every frame counts, window at 304 + fine."""
    return frame_sums(np.asarray(iq)[:ntf * TF_SAMPLES * 2], [W0 + fine] * ntf, [step] * ntf).sum(axis=0, dtype=np.uint64)


def detect(T):
    """The host rule in Python integers: a list of records as dab.tii_detect gives them."""
    T = [int(v) for v in np.asarray(T).reshape(-1)]
    found = []
    for c in range(24):
        v = T[8 * c:8 * c + 8]
        order = sorted(range(8), key=lambda b: (-v[b], b))
        s, n = sum(v[b] for b in order[:4]), sum(v[b] for b in order[4:])
        if not (s > 2 * n and v[order[3]] > 2 * v[order[4]]):
            continue
        word = sum(1 << (7 - b) for b in order[:4])
        found.append({"main": PATTERNS.index(word), "sub": c, "shadow": False, "strong": s, "weak": n})
    for r in found:
        r["shadow"] = any(o is not r and o["main"] == r["main"] and o["strong"] > 64 * r["strong"] for o in found)
    for r in found:
        r["strong"], r["weak"] = min(r["strong"], 2 ** 64 - 1), min(r["weak"], 2 ** 64 - 1)
    return found
