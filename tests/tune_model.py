"""The ingest stage's tuned mode (include/dabhip.h, "ingest stage, tuned mode") restated in plain numpy on top of ingest_model.IngestModel: one
object is one output stream, that is one channel of one input stream.  Written from the header's text.  Only the two tables are taken from the
library (dab.ingest_tune_taps, dab.ingest_tune_nco): test_tune_model.py holds them to their conditions."""
import numpy as np

import dabtools_amd as dab
import ingest_model as im
from ingest_model import W

M32 = (1 << 32) - 1


def step_rule(rate, f):
    """Step 2's step in Python integers: // floors towards minus infinity, % gives 0 .. 2^32 - 1."""
    return ((2 * int(f) * (1 << 32) + int(rate)) // (2 * int(rate))) % (1 << 32)


class TuneModel(im.IngestModel):
    """One channel of one stream.  push(raw) -> the cu8 bytes that push completes."""

    def __init__(self, fmt, rate, offset, gain=0):
        super().__init__(fmt, rate, gain)
        taps, self.L, self.M, self.T = dab.ingest_tune_taps(fmt, rate)
        self.taps = taps.astype(np.int64)
        self.nco = dab.ingest_tune_nco().astype(np.int64)
        self.step = step_rule(rate, offset)

    def mix(self, x, n0):
        """Step 2 on the samples at positions n0, n0 + 1, ..."""
        n = np.arange(len(x), dtype=np.uint64) + np.uint64(n0 & M32)          # n mod 2^32 is enough: theta is taken mod 2^32
        theta = ((n & np.uint64(M32)) * np.uint64(self.step)) & np.uint64(M32)
        i = (((theta + np.uint64(1 << 19)) & np.uint64(M32)) >> np.uint64(20)).astype(np.int64)
        c, s = self.nco[i, 0], self.nco[i, 1]
        yi = (x[:, 0] * c + x[:, 1] * s + 8192) >> 14
        yq = (x[:, 1] * c - x[:, 0] * s + 8192) >> 14
        return np.clip(np.stack([yi, yq], axis=1), -32768, 32767)

    def push(self, raw):
        x = im.to_16bit(self.fmt, raw)
        self.x = np.concatenate([self.x, self.mix(x, self.pushed)])      # the filter's input is y
        if self.g == 0:
            if self.complete() < W:                                      # step 5: held back until output W - 1 exists
                return np.zeros(0, np.uint8)
            v = self._outputs(0, W)
            self.g = im.auto_gain(int((v * v).sum()))
        total = self.complete()
        out = im.requantise(self._outputs(self.produced, total), self.g).reshape(-1)
        self.produced = total
        return out


def one_shot(fmt, rate, gain, raw, offsets):
    """[(bytes, gain)] per channel of one stream pushed at once."""
    res = []
    for f in offsets:
        m = TuneModel(fmt, rate, f, gain)
        res.append((m.push(raw), m.g))
    return res
