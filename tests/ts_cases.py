"""Crafted inputs for the MPEG-2 TS stage, shared by test_ts_model.py (CPU: the model against the independent decoder, a FIFO interleaver and the
construction) and test_gpu_ts.py (the kernels against the model): transport packets and their code words, interleaved streams from any phase,
Reed-Solomon error patterns at the decoder's edges (packet_cases.rs_cases: the code is the same), byte streams at the edges of the sync rule,
every kind of break, and the ETI frames that carry the bytes."""
import numpy as np

import packet_cases as pcs
import ts_model as m
from dabplus_cases import raw_frame

N, K = m.N, m.K


class Source:
    """Code words of transport packets on a few PIDs with null packets in between, a continuity counter per PID, random payloads."""

    def __init__(self, rng, pids=(0x31, 0x132, 0x1ABC)):
        self.rng, self.pids = rng, pids
        self.cc = dict.fromkeys(pids, 0)

    def word(self):
        rng = self.rng
        d = rng.integers(0, 256, K, dtype=np.uint8)
        d[0] = m.SYNC
        if rng.integers(5) == 0:
            pid, cc, pusi = m.NULL_PID, 0, 0
        else:
            pid = self.pids[int(rng.integers(len(self.pids)))]
            cc = self.cc[pid] = (self.cc[pid] + 1) % 16
            pusi = int(rng.integers(6) == 0)
        d[1] = (pusi << 6) | (pid >> 8)
        d[2] = pid & 0xFF
        d[3] = 0x10 | cc
        return m.codeword(d)

    def words(self, n):
        return np.stack([self.word() for _ in range(n)])


def clean_stream(rng, length, phase, errors=None):
    """`length` bytes of an interleaved stream whose slots start at 204 n + phase -> (bytes, words, first): words[i] is code word first + i as
    sent.  errors = {n: 204-byte pattern} is added to the words before the interleaver."""
    first, count = m.words_needed(phase, length)
    words = Source(rng).words(count)
    sent = words.copy()
    for n, e in (errors or {}).items():
        sent[n - first] ^= e
    return m.interleave(sent, first, phase, length), words, first


def junk(rng, n):
    """n random bytes, none of them 0x47."""
    b = rng.integers(0, 256, n, dtype=np.uint8)
    b[b == m.SYNC] = 0x48
    return b


def frames_of_bytes(fct0, subs, nframes=None, ficf=1):
    """subs = [(SubChId, STL, bytes)] -> ETI frames carrying 8 STL bytes of each per frame, as many as the shortest allows (bytes left over at
    the end are not sent)."""
    n = min(len(b) // (8 * stl) for _, stl, b in subs)
    n = n if nframes is None else min(n, nframes)
    return [raw_frame((fct0 + f) % 250, [(scid, stl, b[f * 8 * stl:(f + 1) * 8 * stl]) for scid, stl, b in subs], ficf=ficf) for f in range(n)]


def rs_patterns():
    """The error patterns of every crafted Reed-Solomon word (classes clean, e1, e8, e9, parity, miscorrect, shortened, beyond)."""
    return pcs.error_patterns(pcs.rs_cases())


def rs_stream(rng, stl=204, phase=333):
    """Every crafted error pattern on a code word of its own, a clean word between any two of them (so that errors in byte 0 never make three
    misses in a row), as whole ETI frames' worth of bytes of a sub-channel of this STL."""
    pats = rs_patterns()
    nslots = 2 * len(pats) + 8
    per = 8 * stl
    length = -(-(phase + nslots * m.SLOT + m.LOOK) // per) * per
    errors = {4 + 2 * i: e for i, e in enumerate(pats)}
    return clean_stream(rng, length, phase, errors)[0], len(pats)


# ---- byte streams at the edges of the sync rule ------------------------------------------------------------------------------------------------
SYNC_STL = 51                                            # 408 bytes per ETI frame: exactly two slots
SYNC_ID = 9


def _slot(phase, n):
    return phase + m.SLOT * n


def sync_streams(seed=17):
    """{class: (bytes of a sub-channel of STL 51 in whole frames, {statistic: value} the construction fixes)}"""
    rng = np.random.default_rng(seed)
    per = 8 * SYNC_STL
    out = {}

    def after_junk(nj, nframes=40):
        s, _, _ = clean_stream(rng, nframes * per - nj, 0)
        return np.concatenate([junk(rng, nj), s])

    def ready(length, phase):                            # slots with their look-ahead
        return (length - phase - m.LOOK) // m.SLOT + 1

    # the 5th byte of the first run is byte 3 * 408 - 1: the last one on hand after three frames (decided there), or the first of frame 4 (carried)
    for name, nj in (("run ends with the push", 3 * per - m.RUN_SPAN - 1), ("run ends one byte later", 3 * per - m.RUN_SPAN)):
        out[name] = (after_junk(nj), dict(bytes_skipped=nj, sync_losses=0, packets=ready(40 * per, nj), from_missed_slots=0))
    s = after_junk(1000)
    s[100:100 + 4 * m.SLOT:m.SLOT] = m.SYNC              # 0x47 at 100, 304, 508 and 712; not at 916
    out["false run of 4"] = (s, dict(bytes_skipped=1000, sync_losses=0, packets=ready(40 * per, 1000)))
    for k in (1, 2, 3):
        s, _, _ = clean_stream(rng, 40 * per, 60)
        for n in range(20, 20 + k):
            s[_slot(60, n)] ^= 0xFF
        want = dict(sync_losses=int(k == 3), from_missed_slots=min(k, 2), bytes_skipped=60 + (m.SLOT if k == 3 else 0),
                    packets=ready(40 * per, 60) - int(k == 3))
        out["%d misses in a row" % k] = (s, want)
    s, _, _ = clean_stream(rng, 40 * per + 5, 60)
    at = _slot(60, 25) + 50
    out["slip of 5 bytes"] = (np.concatenate([s[:at], s[at + 5:]]), dict(sync_losses=1, from_missed_slots=2))
    s, _, _ = clean_stream(rng, 40 * per, 60)
    for n in (20, 21, 23, 24, 26):
        s[_slot(60, n)] ^= 0xFF                         # misses, but never three in a row
    out["misses apart"] = (s, dict(sync_losses=0, from_missed_slots=5, bytes_skipped=60, packets=ready(40 * per, 60)))
    return out


def sync_frames(stream_bytes, fct0=0):
    return frames_of_bytes(fct0, [(SYNC_ID, SYNC_STL, stream_bytes)])


def broken_frames(seed=23):
    """Frames of SubChId 9 at STL 51 with every kind of break between stretches long enough to sync and give packets -> (frames, sync losses)"""
    rng = np.random.default_rng(seed)
    per = 8 * SYNC_STL
    s, _, _ = clean_stream(rng, 150 * per, 11)
    frames = sync_frames(s)
    other, _, _ = clean_stream(rng, 30 * 8 * 26, 5)
    frames[20] = raw_frame(20, [(8, SYNC_STL, s[:per])])                                      # the id is missing
    frames[45] = raw_frame(45, [(SYNC_ID, 0, None), (8, SYNC_STL, s[:per])])                  # listed with STL 0
    frames[70] = raw_frame(70, [(8, 750, None), (SYNC_ID, SYNC_STL, s[:per])])                # its payload runs past byte 6144
    frames[71] = raw_frame(71, [(SYNC_ID, SYNC_STL, s[71 * per:72 * per]), (SYNC_ID, 26, other[:208])])   # listed twice: the first entry counts
    frames[95:125] = frames_of_bytes(95, [(SYNC_ID, 26, other)])                              # another STL, then back: two more breaks
    frames[126] = raw_frame(126, [(SYNC_ID, 0, None)])                                        # a break one frame after the last: no sync to lose
    return frames, 5
