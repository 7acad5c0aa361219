"""The block scan (include/dabhip.h, "block scan") restated in plain numpy and Python integers: the fixed-point 4096-point transform and the exact
power spectrum that the GPU's are compared with bit for bit, the bookkeeping of the window across pushes, and the rule that turns a spectrum into
blocks (Python integers throughout: no width to overflow).  Written from the header's text.  Only the NCO table is taken from the library
(dab.ingest_tune_nco): test_tune_model.py holds it to its conditions."""
import functools

import numpy as np

import dabtools_amd as dab
import ingest_model as im

S = 4096
REV = np.array([int(format(i, "012b")[::-1], 2) for i in range(S)])
MIN_WIDTH, MAX_WIDTH, SNAP = 1436000, 1636000, 32000
RASTER = {}
for _n, _khz in zip(range(5, 13), (174928, 181936, 188928, 195936, 202928, 209936, 216928, 223936)):
    for _l in range(4):
        RASTER["%d%s" % (_n, "ABCD"[_l])] = (_khz + 1712 * _l) * 1000
for _l, _khz in zip("ABCDEF", (230784, 232496, 234208, 235776, 237488, 239200)):
    RASTER["13" + _l] = _khz * 1000


@functools.lru_cache(maxsize=None)
def nco():
    cs = dab.ingest_tune_nco().astype(np.int64)
    return cs[:, 0], cs[:, 1]


def transform(x, watch=None, wide=False):
    """Step 2 on segments: [nseg][4096][2] in the 16-bit domain -> X [nseg][4096][2], int64 (wide: Python integers in object arrays).  watch: a list
    that receives, first for the input and then after every stage, (the largest magnitude of a rail, the largest magnitude of a product sum
    b c +- b s + 8192 of that stage)."""
    kind = object if wide else np.int64
    x = np.asarray(x).astype(kind)
    nseg = x.shape[0]
    c, s = (t.astype(kind) for t in nco())
    v = x[:, REV, :]
    if watch is not None:
        watch.append((int(np.abs(v).max()), 0))
    h = 1
    while h < S:
        v = v.reshape(nseg, S // (2 * h), 2, h, 2)
        a, b = v[:, :, 0], v[:, :, 1]
        t = np.arange(h) * (2048 // h)
        pi = b[..., 0] * c[t] + b[..., 1] * s[t] + 8192
        pq = b[..., 1] * c[t] - b[..., 0] * s[t] + 8192
        tw = np.stack([pi >> 14, pq >> 14], axis=-1)
        v = np.stack([(a + tw + 1) >> 1, (a - tw + 1) >> 1], axis=2).reshape(nseg, S, 2)
        if watch is not None:
            watch.append((int(np.abs(v).max()), int(max(np.abs(pi).max(), np.abs(pq).max()))))
        h *= 2
    return v


def power(x):
    """Step 3 of segments [nseg][4096][2]: uint64 [4096]."""
    X = transform(x)
    return (X * X).sum(axis=(0, 2)).astype(np.uint64)


class ScanModel:
    """One stream.  push(raw) -> segments accumulated by that push."""

    def __init__(self, fmt, nsegments=64):
        self.fmt, self.nsegments = fmt, int(nsegments)
        self.P = np.zeros(S, np.uint64)
        self.done = 0
        self.rest = np.zeros((0, 2), np.int64)

    def push(self, raw):
        x = np.concatenate([self.rest, im.to_16bit(self.fmt, raw)])
        n = min(len(x) // S, self.nsegments - self.done)
        if n:
            self.P = self.P + power(x[:n * S].reshape(n, S, 2))
        self.done += n
        self.rest = x[n * S:] if self.done < self.nsegments else x[:0]
        return n


def spectrum(fmt, raw, nsegments=64):
    m = ScanModel(fmt, nsegments)
    m.push(raw)
    return m.P, m.done


class TooManyBlocks(Exception):
    pass


def detect(P, rate, center=0):
    """The host rule in Python integers: a list of records as dab.scan_detect gives them."""
    P = [int(v) for v in P]
    Fin = int(rate)
    sh = [P[(b + S // 2) % S] for b in range(S)]
    pre = [0]
    for v in sh:
        pre.append(pre[-1] + v)
    ni, a0, a1 = 700000 * S // Fin, -(-800000 * S // Fin), 900000 * S // Fin
    w = max(1, 16000 * S // Fin)
    nin, ng = 2 * ni + 1, a1 - a0 + 1

    def total(lo, hi):                                    # bins [lo, hi]
        return pre[hi + 1] - pre[lo]

    def inband(c):
        return total(c - ni, c + ni)

    cand = [c for c in range(a1, S - a1)
            if inband(c) * ng > 4 * total(c - a1, c - a0) * nin and inband(c) * ng > 4 * total(c + a0, c + a1) * nin]
    runs = []
    for c in cand:
        if runs and runs[-1][1] == c - 1:
            runs[-1][1] = c
        else:
            runs.append([c, c])
    found = []
    for a, b in runs:
        c = (a + b) // 2
        inb = inband(c)
        edge = {}
        for d in (-1, 1):
            j = c + d * ni
            while True:
                lo, hi = max(0, j - w), min(S, j + w + 1)
                if (pre[hi] - pre[lo]) * nin * 4 < inb * (hi - lo) or j == 0 or j == S - 1:
                    break
                j += d
            edge[d] = j
        rec = {"offset_hz": ((edge[-1] + edge[1] - S) * Fin + S) // (2 * S), "raw_center_hz": ((a + b - S) * Fin + S) // (2 * S),
               "width_hz": (edge[1] - edge[-1]) * Fin // S, "name": "", "in": min(inb, 2 ** 64 - 1), "lo": min(total(c - a1, c - a0), 2 ** 64 - 1),
               "hi": min(total(c + a0, c + a1), 2 ** 64 - 1), "nin": nin, "ng": ng}
        if not MIN_WIDTH <= rec["width_hz"] <= MAX_WIDTH:
            continue
        if center > 0:
            f = center + rec["offset_hz"]
            name = min(RASTER, key=lambda k: abs(RASTER[k] - f))
            if abs(RASTER[name] - f) <= SNAP:
                rec["offset_hz"], rec["name"] = RASTER[name] - center, name
        found.append(rec)
    if len(found) > 16:
        raise TooManyBlocks(len(found))
    return sorted(found, key=lambda r: r["offset_hz"])
