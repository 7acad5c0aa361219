"""The ingest stage's arithmetic (include/dabhip.h, "ingest stage") restated in plain numpy: what the GPU's bytes are compared with.  Written from the
header's text, phase by phase over strided slices (the kernel goes output by output over a tile in LDS).  Only the tap table is taken from the
library (dab.ingest_taps): its floating-point design need not be reproduced bit for bit, and test_ingest_model.py holds it to its conditions."""
import math

import numpy as np

import dabtools_amd as dab

OUT_RATE = 2048000
W = 65536
DTYPES = {"cu8": np.uint8, "cs8": np.int8, "cs16": np.dtype("<i2"), "cf32": np.dtype("<f4")}
SAMPLE_BYTES = {"cu8": 2, "cs8": 2, "cs16": 4, "cf32": 8}


def to_16bit(fmt, raw):
    """Step 1: an array of 2 n components (I, Q, I, Q, ...) in the format's dtype -> int64 [n][2]."""
    a = np.asarray(raw, dtype=DTYPES[fmt]).reshape(-1, 2)
    if fmt == "cu8":
        return (a.astype(np.int64) - 127) * 256
    if fmt == "cs8":
        return a.astype(np.int64) * 256
    if fmt == "cs16":
        return a.astype(np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        v = a.astype(np.float32) * np.float32(32768.0)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.rint(np.clip(v, np.float32(-32768.0), np.float32(32767.0))).astype(np.int64)


def requantise(v, g):
    """Step 3."""
    return np.clip(127 + ((v * int(g) + 32768) >> 16), 0, 255).astype(np.uint8)


def auto_gain(energy):
    """Step 4, from the exact energy of the first W samples."""
    if energy == 0:
        return 256
    g = math.floor(32.0 * 65536.0 / math.sqrt(energy / (2.0 * W)) + 0.5)
    return int(min(max(g, 1), (1 << 24) - 1))


class IngestModel:
    """One stream.  push(raw) -> the cu8 bytes that push completes."""

    def __init__(self, fmt, rate, gain=0):
        self.fmt, self.rate = fmt, int(rate)
        self.taps, self.L, self.M, self.T = dab.ingest_taps(fmt, rate)
        self.taps = self.taps.astype(np.int64)
        self.g = int(gain)                       # 0: the window is open
        self.x = np.zeros((0, 2), np.int64)      # input samples [base, base + len) in the 16-bit domain; everything below base is zero or out of reach
        self.base = 0
        self.produced = 0

    @property
    def pushed(self):
        return self.base + len(self.x)

    def complete(self):
        """Outputs that exist: m with floor(m M / L) + T/2 <= pushed - 1."""
        k = self.pushed - 1 - self.T // 2
        return 0 if k < 0 else ((k + 1) * self.L - 1) // self.M + 1

    def _outputs(self, m0, m1):
        """v of outputs [m0, m1) (step 2)."""
        L, M, T = self.L, self.M, self.T
        if T == 0:
            return self.x[m0 - self.base:m1 - self.base]
        v = np.zeros((m1 - m0, 2), np.int64)
        pad = T + 2
        xp = np.concatenate([np.zeros((pad, 2), np.int64), self.x])      # xp[i] = x[base - pad + i]
        for r in range(min(L, m1 - m0)):         # outputs m0 + r, m0 + r + L, ...: one phase, n0 moves by M
            m = m0 + r
            p, n0 = (m * M) % L, (m * M) // L
            cnt = (m1 - m + L - 1) // L
            acc = np.zeros((cnt, 2), np.int64)
            for k in range(T):
                first = n0 + T // 2 - k - (self.base - pad)
                assert first >= 0                # the zeros in front stand for x[n] = 0, n < 0
                acc += self.taps[p, k] * xp[first::M][:cnt]
            assert np.abs(acc).max(initial=0) < 1 << 31
            v[r::L] = (acc + 8192) >> 14
        return v

    def push(self, raw):
        self.x = np.concatenate([self.x, to_16bit(self.fmt, raw)])
        if self.g == 0:
            if self.pushed < W:
                return np.zeros(0, np.uint8)
            e = self.x[:W]
            self.g = auto_gain(int((e * e).sum()))
        total = self.complete()
        out = requantise(self._outputs(self.produced, total), self.g).reshape(-1)
        self.produced = total
        return out

    def skip(self, n):
        """n samples of value zero whose outputs are dropped.  Far more than T of them: everything the filter can still reach is zero."""
        assert self.g != 0
        far = 4 * max(self.T, 1)
        if n > 2 * far:
            end = self.pushed + n
            self.x = np.zeros((far, 2), np.int64)
            self.base = end - far
        else:
            self.x = np.concatenate([self.x, np.zeros((n, 2), np.int64)])
        self.produced = self.complete()


def one_shot(fmt, rate, gain, raw):
    m = IngestModel(fmt, rate, gain)
    return m.push(raw), m.g
