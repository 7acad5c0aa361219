"""The MPEG-2 TS stage (include/dabhip.h: dabhip_ts) restated in plain numpy, one lane at a time and serially: the byte stream of a
(stream, SubChId) with its breaks, the slot sync rule byte for byte as the header words it, the closed-form de-interleaver, RS(204,188) and the
record.  The kernels (k_ts.hip) must agree with this bit for bit.  The code is the packet stage's, so its field and its decoder are
packet_model's; tests/rs204_reference.py is the independent check of both."""
import numpy as np

from packet_model import ETI_BYTES, K, N, rs_decode, rs_parity, syndromes_many  # noqa: F401  (re-exported)

SLOT, RUN, LOOK, MISS_LIMIT, SYNC = 204, 5, 2448, 3, 0x47
RUN_SPAN = SLOT * (RUN - 1)                              # 816
CARRY = LOOK - 1
NULL_PID = 0x1FFF
FROM_MISS, RS_FAILED, TEI, PUSI, BAD_SYNC = 1, 2, 4, 8, 16
STATS = ("packets", "from_missed_slots", "sync_losses", "bytes_skipped", "rs_corrected_bytes", "rs_failed_words", "bad_sync_packets", "null_packets")
STL_MAX = (ETI_BYTES - 16) // 8                          # 766: NST = 1, no FIC

# byte k of the code word whose slot starts at P lies at P + GATHER[k]
GATHER = np.arange(N) + SLOT * (np.arange(N) % 12)
assert GATHER.max() == LOOK - 1


def codeword(data):
    """188 TS bytes -> the 204-byte code word."""
    data = np.asarray(data, dtype=np.uint8)
    assert data.size == K
    return np.concatenate([data, rs_parity(data)])


def interleave(words, first, phase, length):
    """The first `length` bytes of the stream in which the slot of code word n starts at position 204 n + phase; words[i] is word first + i, and
    every word that has a byte in the range must be among them."""
    x = np.arange(length, dtype=np.int64) - phase
    k = x % SLOT
    n = (x - k) // SLOT - k % 12
    assert length == 0 or (n.min() >= first and n.max() < first + len(words)), (n.min(), n.max(), first, len(words))
    return np.asarray(words, dtype=np.uint8)[n - first, k]


def words_needed(phase, length):
    """(first, count) of the code words interleave() needs for these bytes."""
    first = (0 - phase - (SLOT - 1)) // SLOT - 11
    last = (length - 1 - phase) // SLOT
    return first, last - first + 1


def locate(frame, scid):
    """(STL of the first STC entry with this id, its payload or None) -- (0, None) when the frame lacks the id."""
    f = np.asarray(frame, dtype=np.uint8)
    ficf, nst = int(f[5]) >> 7, int(f[5]) & 0x7F
    off = 12 + 4 * nst + 96 * ficf
    for i in range(nst):
        sid = int(f[8 + 4 * i]) >> 2
        stl = (int(f[8 + 4 * i + 2]) & 3) << 8 | int(f[8 + 4 * i + 3])
        if sid == scid:
            if stl > 0 and off + 8 * stl <= ETI_BYTES:
                return stl, f[off:off + 8 * stl]
            return stl, None
        off += 8 * stl
        if off > ETI_BYTES:
            break
    return 0, None


_DECODED = {}


def decode_words(words):
    """[n][204] received words -> ([n][204] after decoding, [n] symbols corrected or -1)."""
    words = np.asarray(words, dtype=np.uint8).reshape(-1, N)
    out, count = words.copy(), np.zeros(len(words), dtype=np.int64)
    if len(words) == 0:
        return out, count
    dirty = np.flatnonzero(syndromes_many(words).any(axis=1))
    for i in dirty:
        key = words[i].tobytes()
        if key not in _DECODED:
            _DECODED[key] = rs_decode(words[i])
        out[i], count[i] = _DECODED[key]
    return out, count


def record(pos, word, corrected, from_miss):
    """(pos, pid, continuity, flags, corrected) of a word after decoding (corrected = -1: failed, as received)."""
    b0, b1, b2, b3 = (int(v) for v in word[:4])
    flags = (FROM_MISS if from_miss else 0) | (RS_FAILED if corrected < 0 else 0) | (TEI if b1 & 0x80 else 0) | (PUSI if b1 & 0x40 else 0) | \
        (BAD_SYNC if b0 != SYNC else 0)
    return (int(pos), ((b1 & 0x1F) << 8) | b2, b3 & 15, flags, max(int(corrected), 0))


class Lane:
    """One (stream, sub-channel): push(frames) -> (records, [n][188] bytes) of that push; .stat_list() as dabhip_ts_stats."""

    def __init__(self, scid):
        self.scid = scid
        self.buf = np.zeros(0, dtype=np.uint8)             # the unconsumed bytes of the unbroken stream
        self.base = 0                                      # position of buf[0]
        self.synced, self.misses, self.stl = False, 0, 0
        self.stats = dict.fromkeys(STATS, 0)
        self.max_carry = 0

    def stat_list(self):
        return [self.stats[k] for k in STATS]

    def _rule(self, new, taken):
        """The sync rule over the bytes on hand; the slots it takes go to `taken` as (pos, word, from_miss)."""
        buf = np.concatenate([self.buf] + new) if new else self.buf
        end, q, st = len(buf), 0, self.stats
        while True:
            if not self.synced:
                n = end - RUN_SPAN - q                      # candidates p = q .. end - 817: p + 816 < end
                run = np.zeros(0, dtype=bool)
                if n > 0:
                    run = np.ones(n, dtype=bool)
                    for i in range(RUN):
                        run &= buf[q + SLOT * i:q + SLOT * i + n] == SYNC
                if run.any():
                    p = q + int(np.argmax(run))
                    st["bytes_skipped"] += p - q
                    q, self.synced, self.misses = p, True, 0
                else:
                    wait = max(q, end - RUN_SPAN)
                    st["bytes_skipped"] += wait - q
                    q = wait
                    break
            else:
                if q + LOOK > end:
                    break
                hit = buf[q] == SYNC
                self.misses = 0 if hit else self.misses + 1
                if self.misses == MISS_LIMIT:
                    st["sync_losses"] += 1
                    st["bytes_skipped"] += 1
                    self.synced, self.misses = False, 0
                    q += 1
                    continue
                taken.append((self.base + q, buf[q + GATHER], not hit))
                q += SLOT
        self.base += q
        self.buf = buf[q:]

    def _break(self):
        st = self.stats
        st["bytes_skipped"] += len(self.buf)
        if self.synced:
            st["sync_losses"] += 1
        self.base += len(self.buf)
        self.buf = np.zeros(0, dtype=np.uint8)
        self.synced, self.misses, self.stl = False, 0, 0

    def push(self, frames):
        taken, new = [], []
        for f in frames:
            stl, pay = locate(f, self.scid)
            if pay is None or (self.stl and stl != self.stl):
                self._rule(new, taken)
                new = []
                self._break()
            if pay is None:
                continue
            self.stl = stl
            new.append(pay)
        self._rule(new, taken)
        self.max_carry = max(self.max_carry, len(self.buf))
        assert len(self.buf) <= CARRY
        words, counts = decode_words([w for _, w, _ in taken])
        recs = [record(pos, w, c, miss) for (pos, _, miss), w, c in zip(taken, words, counts)]
        st = self.stats
        st["packets"] += len(recs)
        for r, c in zip(recs, counts):
            st["from_missed_slots"] += bool(r[3] & FROM_MISS)
            st["rs_corrected_bytes"] += max(int(c), 0)
            st["rs_failed_words"] += c < 0
            st["bad_sync_packets"] += bool(r[3] & BAD_SYNC)
            st["null_packets"] += r[1] == NULL_PID
        self.stats = {k: int(v) for k, v in st.items()}
        return recs, words[:, :K].copy()
