"""Crafted inputs for the packet-mode stage, shared by test_packet_model.py (CPU: the model against the independent decoder and against the
construction) and test_gpu_packet.py (the kernels against the model): Reed-Solomon words at the decoder's edges, cell streams at the edges of
the FEC sync rule, tables at the edges of the walk, a source of data groups cut into packets, and the ETI frames that carry cells."""
import numpy as np

import packet_model as m
import rs204_reference as ref
from dabplus_cases import raw_frame

N, K = m.N, m.K


# ---- Reed-Solomon words ----------------------------------------------------------------------------------------------------------------------------
def codeword(rng):
    data = rng.integers(0, 256, K, dtype=np.uint8)
    return np.concatenate([data, ref.encode(data)])


def _flip(rng, word, positions):
    rx = word.copy()
    rx[positions] ^= rng.integers(1, 256, len(positions)).astype(np.uint8)
    return rx


def _x_power_mod_gen(p, v):
    """v x^p modulo the generator: 16 bytes, highest degree first (the parity positions of a word)."""
    rem = [0] * 15 + [v]
    for _ in range(p):
        fb, rem = rem[0], rem[1:] + [0]
        if fb:
            rem = [c ^ ref.mul(fb, g) for c, g in zip(rem, ref.GEN[1:])]
    return np.array(rem, dtype=np.uint8)


_RS = None


def rs_cases(seed=204):
    """{class: [(label, received word, expected word or None, expected count or None, error pattern)]}: None where only a decoder can say
    (classes e9, beyond).  The error pattern added to any other code word gives a word with the same fate."""
    global _RS
    if _RS is not None:
        return _RS
    rng = np.random.default_rng(seed)
    out = {c: [] for c in ("clean", "e1", "e8", "e9", "parity", "miscorrect", "shortened", "beyond")}
    for i in range(3):
        w = codeword(rng)
        out["clean"].append(("clean %d" % i, w, w, 0, w))
    for p in (0, 1, 187, 188, 203):
        w = codeword(rng)
        out["e1"].append(("one error at %d" % p, _flip(rng, w, [p]), w, 1, w))
    for i in range(12):
        w = codeword(rng)
        pos = rng.choice(N, 8, replace=False) if i else np.array([0, 1, 2, 186, 187, 188, 202, 203])
        out["e8"].append(("eight errors %d" % i, _flip(rng, w, pos), w, 8, w))
    for i in range(12):
        w = codeword(rng)
        out["e9"].append(("nine errors %d" % i, _flip(rng, w, rng.choice(N, 9, replace=False)), None, None, w))
    for n in (1, 4, 8):
        w = codeword(rng)
        out["parity"].append(("%d errors in the parity" % n, _flip(rng, w, K + rng.choice(16, n, replace=False)), w, n, w))
    for i in range(8):
        # a code word of weight 17 (one data byte and its parity: the code is MDS) added to w gives the nearest other code word; 9 of its 17
        # bytes put w at distance 9 and the other at distance 8
        w = codeword(rng)
        unit = np.zeros(K, dtype=np.uint8)
        unit[int(rng.integers(K))] = int(rng.integers(1, 256))
        low = np.concatenate([unit, ref.encode(unit)])
        support = np.flatnonzero(low)
        assert len(support) == 17
        take = rng.choice(support, 9, replace=False)
        rx = w.copy()
        rx[take] ^= low[take]
        out["miscorrect"].append(("miscorrection %d" % i, rx, w ^ low, 8, w))
    for i in range(10):
        # t errors of the full-length (255) code, one of them among the 51 positions the shortening removed: what that one adds to the syndromes
        # is added through the parity bytes instead, so the locator the decoder finds has a root where no byte is
        w = codeword(rng)
        t = 1 + i % 8
        live = rng.choice(N, t - 1, replace=False)
        rx = _flip(rng, w, live) if t > 1 else w.copy()
        p = int(rng.integers(N, 255))
        rx[K:] ^= _x_power_mod_gen(p, int(rng.integers(1, 256)))
        out["shortened"].append(("root at power %d, %d errors" % (p, t), rx, rx, -1, w))
    for i in range(300):
        w = codeword(rng)
        n = int(rng.integers(9, 40))
        out["beyond"].append(("%d errors, %d" % (n, i), _flip(rng, w, rng.choice(N, n, replace=False)), None, None, w))
    # the word each case started from -> its error pattern
    _RS = {cls: [(label, rx, want, n, rx ^ w) for label, rx, want, n, w in cases] for cls, cases in out.items()}
    return _RS


def error_patterns(cases):
    """The error patterns of rs_cases(), class after class."""
    return [c[4] for cls in sorted(cases) for c in cases[cls]]


def add_error(frame, r, err):
    """Error pattern err (204 bytes) added to code word r of an FEC frame of 103 cells, in place."""
    frame[:m.TABLE].reshape(K, m.ROWS)[:, r] ^= err[:K]
    fec = frame.reshape(m.FRAME_CELLS, m.CELL)[m.DATA_CELLS:]
    pay = fec[:, 2:].reshape(-1).copy()
    pay[:16 * m.ROWS].reshape(16, m.ROWS)[:, r] ^= err[K:]
    fec[:, 2:] = pay.reshape(m.FEC_CELLS, 22)


def frames_with_errors(src, patterns):
    """FEC frames of packets from a TableSource with the error patterns on their code words, 12 to a frame -> [103 received cells each]"""
    frames = []
    for at in range(0, len(patterns), m.ROWS):
        f = m.fec_frame(src.unit())
        for r, err in enumerate(patterns[at:at + m.ROWS]):
            add_error(f, r, err)
        frames.append(f)
    return frames


# ---- tables of packets and the data groups in them -------------------------------------------------------------------------------------------------
class TableSource:
    """Data groups with random lengths and flags on a few addresses, cut into packets of mixed lengths, command packets in between, padding to
    fill each unit exactly.  .groups: every completed group (address, bytes) in the order their last packets go out."""

    def __init__(self, rng, addresses=(5, 600, 1021), max_group=300):
        self.rng, self.addresses, self.max_group = rng, addresses, max_group
        self.pending = {a: None for a in addresses}               # [bytes, offset]
        self.ci = {a: 0 for a in addresses}
        self.groups = []

    def _packet(self, room):
        rng = self.rng
        L = int(rng.integers(1, min(4, room) + 1))
        cap = m.CELL * L - 5
        kind = int(rng.integers(10))
        if kind == 0:                                             # padding
            return m.make_packet(L, 0, 3, 0, 0, b"", fill=int(rng.integers(256)))
        a = self.addresses[int(rng.integers(len(self.addresses)))]
        if kind == 1:                                             # a command packet: not part of any group, keeps no continuity
            return m.make_packet(L, int(rng.integers(4)), 3, a, 1, bytes(rng.integers(0, 256, int(rng.integers(cap + 1)), dtype=np.uint8)))
        first = self.pending[a] is None
        if first:
            size = int(rng.integers(24, self.max_group))
            self.pending[a] = [m.make_group(rng, size), 0]
        g, at = self.pending[a]
        n = min(cap if rng.integers(4) else int(rng.integers(1, cap + 1)), len(g) - at)
        last = at + n == len(g)
        self.ci[a] = (self.ci[a] + 1) % 4
        pk = m.make_packet(L, self.ci[a], (2 if first else 0) | (1 if last else 0), a, 0, g[at:at + n], fill=int(rng.integers(256)))
        self.pending[a] = None if last else [g, at + n]
        if last:
            self.groups.append((a, g))
        return pk

    def unit(self, ncells=m.DATA_CELLS):
        cells, room = [], ncells
        while room:
            pk = self._packet(room)
            cells.append(pk)
            room -= len(pk) // m.CELL
        return np.concatenate(cells)


def unit_groups(cells):
    """The data groups of the packets of one unit's cells, by the model: [(address, bytes)]; every cell must belong to a good packet."""
    recs, data, bad = m.walk(cells, 0, 0)
    assert bad == 0
    g = m.Groups()
    done = g.push(recs, data)
    assert g.stats["dropped"] == 0 and g.stats["orphan_packets"] == 0 and g.stats["crc_fails"] == 0 and not g.open
    return recs, [(r["address"], b) for r, b in done]


def walk_table(rng):
    """A table at the walk's edges -> (2256 bytes, [(cell, address, length)] of the packets the walk must take, bad cells)."""
    cells, want, bad = [], [], 0
    bad_crc = m.make_packet(4, 1, 3, 77, 0, b"bad crc")
    bad_crc[50] ^= 1
    cells.append(bad_crc[:m.CELL])                                # cell 0: a length-4 header whose CRC fails ...
    bad += 1
    cells.append(m.make_packet(2, 2, 3, 77, 0, b"a good packet one cell later"))       # ... and a good packet at cell 1
    want.append((1, 77, 2))
    long_useful = m.make_packet(1, 0, 3, 9, 0, b"", useful_length=20)                  # good CRC, useful length above 24 - 5
    cells.append(long_useful)
    bad += 1
    k = 4
    while k < m.DATA_CELLS - 2:
        L = min(int(rng.integers(1, 5)), m.DATA_CELLS - 2 - k)
        addr = 0 if rng.integers(3) == 0 else 33                  # padding packets among them
        cells.append(m.make_packet(L, k & 3, 3, addr, 0, bytes(rng.integers(0, 256, int(rng.integers(m.CELL * L - 4)), dtype=np.uint8)), fill=0xA5))
        want.append((k, addr, L))
        k += L
    cells.append(m.make_packet(3, 0, 3, 44, 0, b"runs past the unit")[:m.CELL])       # cell 92: a length that runs past the unit
    bad += 1
    cells.append(m.make_packet(1, 3, 3, 44, 0, b"last cell"))
    want.append((m.DATA_CELLS - 1, 44, 1))
    table = np.concatenate(cells)
    assert table.size == m.TABLE
    return table, want, bad


# ---- cell streams at the edges of the sync rule ----------------------------------------------------------------------------------------------------
def _break_headers(frame, which):
    f = frame.reshape(m.FRAME_CELLS, m.CELL).copy()
    for i in which:
        f[m.DATA_CELLS + i, 1] ^= 0x40
    return f.reshape(-1)


def sync_streams(seed=7):
    """{class: (cells as one byte array, {statistic: value} the construction fixes)}"""
    rng = np.random.default_rng(seed)
    src = TableSource(rng)
    frame = lambda: m.fec_frame(src.unit())
    out = {}
    fr = [frame() for _ in range(4)]
    out["run before cell 94"] = (np.concatenate([fr[0][64 * m.CELL:]] + fr[1:]), dict(units=3, cells_skipped=39, sync_losses=0))
    fake = np.concatenate([m.fec_cells(np.zeros(192, np.uint8))[:8 * m.CELL], src.unit(1)])      # FEC headers 0..7, then a packet
    fr = [frame() for _ in range(3)]
    out["false run of 8"] = (np.concatenate([fake] + fr), dict(units=3, cells_skipped=9, sync_losses=0))
    fr = [frame() for _ in range(4)]
    fr[1] = _break_headers(fr[1], (0, 2, 4, 6))                   # 5 good headers: a hit
    fr[2] = _break_headers(fr[2], (1, 3, 5, 7, 8))                # 4 good headers: a miss
    out["4 and 5 good headers"] = (np.concatenate(fr), dict(units=4, missed_frames=1, sync_losses=0, cells_skipped=0))
    fr = [frame() for _ in range(7)]
    for i in (1, 2, 3):
        fr[i] = _break_headers(fr[i], range(9))
    out["third miss"] = (np.concatenate(fr), dict(units=6, missed_frames=2, sync_losses=1, cells_skipped=103))
    fr = [frame() for _ in range(8)]
    cut = np.concatenate(fr)
    cut = np.concatenate([cut[:(2 * 103 + 20) * m.CELL], cut[(2 * 103 + 31) * m.CELL:]])        # 11 cells lost in frame 2
    out["slip of 11 cells"] = (cut, dict(missed_frames=2, sync_losses=1))
    fr = [frame() for _ in range(5)]
    for i in (1, 3):
        fr[i] = _break_headers(fr[i], range(9))                   # two misses, but never three in a row
    out["misses apart"] = (np.concatenate(fr), dict(units=5, missed_frames=2, sync_losses=0, cells_skipped=0))
    return out


def sent_whole(cells, s, seed=1):
    """cells with good FEC frames behind them, up to whole ETI frames of s cells: frames_of_cells() then sends every cell given (the frames added
    change the units a stream gives, not its misses, losses or skipped cells)."""
    src = TableSource(np.random.default_rng(seed))
    more = np.concatenate([m.fec_frame(src.unit()) for _ in range(s // m.FRAME_CELLS + 2)])
    ncells = len(cells) // m.CELL
    return np.concatenate([cells, more[:(-ncells % s) * m.CELL]])


# ---- ETI frames ------------------------------------------------------------------------------------------------------------------------------------
def frames_of_cells(fct0, subs, nframes=None):
    """subs = [(SubChId, s, cells as one byte array)] -> ETI frames carrying s cells of each per frame, as many as the shortest allows (cells left
    over at the end are not sent)."""
    n = min(len(c) // (m.CELL * s) for _, s, c in subs)
    n = n if nframes is None else min(n, nframes)
    return [raw_frame((fct0 + f) % 250, [(scid, 3 * s, c[f * m.CELL * s:(f + 1) * m.CELL * s]) for scid, s, c in subs]) for f in range(n)]
