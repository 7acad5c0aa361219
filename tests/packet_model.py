"""Plain-numpy restatement of the packet-mode stage (include/dabhip.h: dabhip_packet, dabhip_packet_groups; ETSI EN 300 401 clauses 5.3.2,
5.3.3, 5.3.5): cells out of ETI frames, the packet header and CRC, the FEC frame of the enhanced packet mode with RS(204,188) by
Berlekamp-Massey, Chien and Forney on log / exp tables, FEC frame sync, the walk and the data-group rule.  It works on whole lists of cells
and searches them directly, where the kernels take a cell at a time.  tests/rs204_reference.py decides the same RS question with nothing shared."""
import numpy as np

ETI_BYTES = 6144
CELL = 24
DATA_CELLS, FEC_CELLS, FRAME_CELLS = 94, 9, 103
TABLE = DATA_CELLS * CELL
ROWS, N, K, NROOTS, T = 12, 204, 188, 16, 8
FEC_ADDRESS = 1022
CARRY = 102
FROM_FEC, FROM_MISS = 1, 2
MAX_GROUP = 8208

# ---- GF(256), 0x11D, alpha = 2 -------------------------------------------------------------------------------------------------------------------
EXP = np.zeros(512, dtype=np.int64)
LOG = np.zeros(256, dtype=np.int64)
_x = 1
for _i in range(255):
    EXP[_i] = EXP[_i + 255] = _x
    LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11D
EXP[510], EXP[511] = EXP[0], EXP[1]


def gmul(a, b):
    return int(EXP[LOG[a] + LOG[b]]) if a and b else 0


def ginv(a):
    return int(EXP[255 - LOG[a]])


def generator():
    """prod (x + alpha^i), i = 0..15, highest degree first."""
    g = [1]
    for i in range(NROOTS):
        root = int(EXP[i])
        g = [a ^ b for a, b in zip(g + [0], [0] + [gmul(c, root) for c in g])]
    return g


GEN = generator()


def rs_parity(data):
    """188 data bytes -> 16 parity bytes (LFSR division by the generator)."""
    reg = [0] * NROOTS
    for b in data:
        fb = int(b) ^ reg[0]
        reg = [reg[i + 1] ^ gmul(fb, GEN[i + 1]) for i in range(NROOTS - 1)] + [gmul(fb, GEN[NROOTS])]
    return np.array(reg, dtype=np.uint8)


def syndromes(word):
    out = []
    for i in range(NROOTS):
        s, a = 0, int(EXP[i])
        for b in word:
            s = gmul(s, a) ^ int(b)
        out.append(s)
    return out


def syndromes_many(words):
    """[n][204] -> [n][16], all words at once."""
    w = np.asarray(words, dtype=np.int64)
    S = np.zeros((w.shape[0], NROOTS), dtype=np.int64)
    for c in range(N):
        b = w[:, c]
        for i in range(NROOTS):
            s = S[:, i]
            S[:, i] = np.where(s != 0, EXP[(LOG[s] + i) % 255], 0) ^ b
    return S


def rs_decode(word):
    """(code word, symbols corrected) when a code word lies within distance 8, else (word unchanged, -1)."""
    r = np.array(word, dtype=np.uint8)
    S = syndromes(r)
    if not any(S):
        return r, 0
    lam, B, L, m, b = [1], [1], 0, 1, 1
    for n in range(NROOTS):
        d = S[n]
        for i in range(1, L + 1):
            if i < len(lam):
                d ^= gmul(lam[i], S[n - i])
        if d == 0:
            m += 1
            continue
        coef = gmul(d, ginv(b))
        shifted = [0] * m + [gmul(coef, c) for c in B]
        new = [(lam[i] if i < len(lam) else 0) ^ (shifted[i] if i < len(shifted) else 0) for i in range(max(len(lam), len(shifted)))]
        if 2 * L <= n:
            B, b, L, m = lam, d, n + 1 - L, 1
        else:
            m += 1
        lam = new
    while lam and lam[-1] == 0:
        lam.pop()
    deg = len(lam) - 1
    if deg > T or deg != L:
        return r, -1
    roots = []                                            # powers p with lambda(alpha^-p) = 0
    for p in range(255):
        v = 0
        for i, c in enumerate(lam):
            if c:
                v ^= int(EXP[(LOG[c] + (255 - p) * i) % 255])
        if v == 0:
            roots.append(p)
    if len(roots) != deg or any(p >= N for p in roots):
        return r, -1
    omega = [0] * NROOTS
    for i in range(NROOTS):
        for j in range(min(i, deg) + 1):
            omega[i] ^= gmul(S[i - j], lam[j])
    out = r.copy()
    for p in roots:
        X, Xi = int(EXP[p]), int(EXP[(255 - p) % 255])
        num = den = 0
        for i in range(NROOTS):
            num ^= gmul(omega[i], int(EXP[(LOG[Xi] * i) % 255]))
        for i in range(1, deg + 1, 2):
            den ^= gmul(lam[i], int(EXP[(LOG[Xi] * (i - 1)) % 255]))
        if den == 0:
            return r, -1
        e = gmul(X, gmul(num, ginv(den)))
        if e == 0:
            return r, -1
        out[N - 1 - p] ^= e
    if any(syndromes(out)):
        return r, -1
    return out, deg


# ---- packets and FEC frames ----------------------------------------------------------------------------------------------------------------------
def _crc_byte(v):
    c = v << 8
    for _ in range(8):
        c = ((c << 1) ^ 0x1021) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


_CRC = [_crc_byte(v) for v in range(256)]


def crc16(data, crc=0xFFFF):
    """x^16 + x^12 + x^5 + 1, most significant bit first, from 0xFFFF (not complemented here)."""
    for b in bytes(data):
        crc = _CRC[(crc >> 8) ^ b] ^ ((crc << 8) & 0xFFFF)
    return crc


def make_packet(length, ci, first_last, address, command, useful, fill=0, useful_length=None):
    """A packet of `length` cells (24 length bytes) with the complemented CRC."""
    useful = bytes(useful)
    n = CELL * length
    assert 1 <= length <= 4 and len(useful) <= n - 5
    ul = len(useful) if useful_length is None else useful_length
    p = bytearray([fill]) * n
    p[0] = ((length - 1) << 6) | ((ci & 3) << 4) | ((first_last & 3) << 2) | ((address >> 8) & 3)
    p[1] = address & 0xFF
    p[2] = ((command & 1) << 7) | (ul & 0x7F)
    p[3:3 + len(useful)] = useful
    c = crc16(p[:n - 2]) ^ 0xFFFF
    p[n - 2], p[n - 1] = c >> 8, c & 0xFF
    return np.frombuffer(bytes(p), dtype=np.uint8).copy()


def fec_counter(cell):
    b0, b1 = int(cell[0]), int(cell[1])
    cnt = (b0 >> 2) & 15
    return cnt if (b0 >> 6) == 0 and (b0 & 3) == 3 and b1 == 0xFE and cnt < FEC_CELLS else None


def table_parity(table):
    """The 2256-byte application table -> 192 parity bytes: code word r is Z[r + 12 c]."""
    t = np.asarray(table, dtype=np.uint8).reshape(K, ROWS)
    par = np.zeros((NROOTS, ROWS), dtype=np.uint8)
    for r in range(ROWS):
        par[:, r] = rs_parity(t[:, r])
    return par.reshape(-1)


def fec_cells(parity):
    """192 parity bytes -> the 9 FEC cells (as one array of 216 bytes)."""
    rs = np.concatenate([np.asarray(parity, dtype=np.uint8), np.zeros(6, np.uint8)]).reshape(FEC_CELLS, 22)
    out = np.zeros((FEC_CELLS, CELL), dtype=np.uint8)
    for i in range(FEC_CELLS):
        out[i, 0] = (i << 2) | (FEC_ADDRESS >> 8)
        out[i, 1] = FEC_ADDRESS & 0xFF
        out[i, 2:] = rs[i]
    return out.reshape(-1)


def fec_frame(table):
    """The 103 cells of the FEC frame of a table."""
    return np.concatenate([np.asarray(table, dtype=np.uint8), fec_cells(table_parity(table))])


def decode_frame(cells):
    """103 received cells -> (the 94 data cells after correction, symbols corrected, code words failed)."""
    cells = np.asarray(cells, dtype=np.uint8).reshape(FRAME_CELLS, CELL)
    parity = cells[DATA_CELLS:, 2:].reshape(-1)[:NROOTS * ROWS]
    z = np.concatenate([cells[:DATA_CELLS].reshape(-1), parity]).reshape(N, ROWS)
    dirty = np.flatnonzero(syndromes_many(z.T).any(axis=1))
    fixed = failed = 0
    for r in dirty:
        word, n = rs_decode(z[:, r])
        if n < 0:
            failed += 1
        else:
            fixed += n
            z[:, r] = word
    return z[:K].reshape(DATA_CELLS, CELL), fixed, failed


def walk(cells, cell_index, flags):
    """The walk over the cells of a unit -> ([records], [useful bytes], bad cells).  A record: (cell, address, length, continuity, first/last,
    command, useful length, flags)."""
    cells = np.asarray(cells, dtype=np.uint8).reshape(-1, CELL)
    recs, data, bad, k = [], [], 0, 0
    while k < len(cells):
        p = cells[k]
        L = (int(p[0]) >> 6) + 1
        ul = int(p[2]) & 0x7F
        ok = k + L <= len(cells) and ul <= CELL * L - 5
        if ok:
            body = cells[k:k + L].reshape(-1)
            ok = (crc16(body[:-2]) ^ 0xFFFF) == (int(body[-2]) << 8 | int(body[-1]))
        if not ok:
            bad += 1
            k += 1
            continue
        recs.append((cell_index + k, (int(p[0]) & 3) << 8 | int(p[1]), L, (int(p[0]) >> 4) & 3, (int(p[0]) >> 2) & 3, int(p[2]) >> 7, ul, flags))
        data.append(body[3:3 + ul].copy())
        k += L
    return recs, data, bad


def locate(frame, scid):
    """(STL of the first STC entry with this id, its payload or None) -- (0, None) when the frame lacks the id."""
    f = np.asarray(frame, dtype=np.uint8)
    ficf, nst = int(f[5]) >> 7, int(f[5]) & 0x7F
    off = 12 + 4 * nst + 96 * ficf
    for i in range(nst):
        sid = int(f[8 + 4 * i]) >> 2
        stl = (int(f[8 + 4 * i + 2]) & 3) << 8 | int(f[8 + 4 * i + 3])
        if sid == scid:
            if stl > 0 and stl % 3 == 0 and off + 8 * stl <= ETI_BYTES:
                return stl, f[off:off + 8 * stl]
            return stl, None
        off += 8 * stl
        if off > ETI_BYTES:
            break
    return 0, None


STATS = ("units", "missed_frames", "sync_losses", "cells_skipped", "bad_cells", "packets", "rs_corrected_bytes", "rs_failed_codewords")


class Lane:
    """One (stream, sub-channel): push(frames) -> (records, useful bytes per record) of that push; .stats as dabhip_packet_stats."""

    def __init__(self, scid, fec):
        self.scid, self.fec = scid, bool(fec)
        self.cells = []                                   # the unconsumed cells of the unbroken stream
        self.first = 0                                    # index since creation of cells[0]
        self.stl = 0
        self.synced, self.misses, self.search = False, 0, 0
        self.stats = dict.fromkeys(STATS, 0)
        self.decoder = decode_frame

    def _drop(self, n):
        del self.cells[:n]
        self.first += n

    def _break(self):
        self.stats["cells_skipped"] += len(self.cells)
        self.stats["sync_losses"] += 1 if self.synced else 0
        self._drop(len(self.cells))
        self.synced, self.misses, self.search, self.stl = False, 0, 0, 0

    def _unit(self, cells, flags, out):
        if flags & FROM_FEC:
            cells, fixed, failed = self.decoder(cells)
            self.stats["rs_corrected_bytes"] += fixed
            self.stats["rs_failed_codewords"] += failed
        recs, data, bad = walk(np.asarray(cells).reshape(-1, CELL)[:DATA_CELLS] if flags else cells, self.first, flags)
        self.stats["units"] += 1
        self.stats["missed_frames"] += 1 if flags & FROM_MISS else 0
        self.stats["bad_cells"] += bad
        self.stats["packets"] += len(recs)
        out[0].extend(recs)
        out[1].extend(data)

    def _run_at(self, k):
        return all(fec_counter(self.cells[k + i]) == i for i in range(FEC_CELLS))

    def _advance(self, out):
        while True:
            if self.synced:
                if len(self.cells) < FRAME_CELLS:
                    return
                good = sum(fec_counter(self.cells[DATA_CELLS + i]) == i for i in range(FEC_CELLS))
                if good >= 5:
                    self.misses = 0
                    self._unit(np.array(self.cells[:FRAME_CELLS]), FROM_FEC, out)
                    self._drop(FRAME_CELLS)
                elif self.misses == 2:
                    self.synced, self.misses, self.search = False, 0, 1
                    self.stats["sync_losses"] += 1
                else:
                    self.misses += 1
                    self._unit(np.array(self.cells[:FRAME_CELLS]), FROM_MISS, out)
                    self._drop(FRAME_CELLS)
            else:
                k = self.search
                while k + FEC_CELLS <= len(self.cells) and not self._run_at(k):
                    k += 1
                if k + FEC_CELLS > len(self.cells):
                    self.search = k
                    return
                if k >= DATA_CELLS:
                    self.stats["cells_skipped"] += k - DATA_CELLS
                    self._drop(k - DATA_CELLS)
                    self._unit(np.array(self.cells[:FRAME_CELLS]), FROM_FEC, out)
                    self._drop(FRAME_CELLS)
                else:
                    self.stats["cells_skipped"] += k + FEC_CELLS
                    self._drop(k + FEC_CELLS)
                self.synced, self.misses, self.search = True, 0, 0

    def push(self, frames):
        out = ([], [])
        for f in frames:
            stl, pay = locate(f, self.scid)
            if pay is None or (self.stl and stl != self.stl):
                self._break()
            if pay is None:
                continue
            self.stl = stl
            cells = list(np.asarray(pay, dtype=np.uint8).reshape(-1, CELL))
            if not self.fec:
                self.cells = cells
                self._unit(np.array(cells), 0, out)
                self._drop(len(cells))
                continue
            self.cells.extend(cells)
            self._advance(out)
        if self.fec and not self.synced and len(self.cells) > CARRY:
            d = len(self.cells) - CARRY
            self.stats["cells_skipped"] += d
            self._drop(d)
            self.search = max(0, self.search - d)
        return out

    def stat_list(self):
        return [self.stats[k] for k in STATS]


# ---- data groups ---------------------------------------------------------------------------------------------------------------------------------
def make_group(rng, size, gtype=None, ext=None, crc=None, seg=None, ua=None, tid=None, ci=0, rep=0):
    """A data group of `size` bytes in all with the given (or random) header flags; the body is random."""
    pick = lambda v: int(rng.integers(2)) if v is None else int(v)
    ext, crc, seg, ua = pick(ext), pick(crc), pick(seg), pick(ua)
    gtype = int(rng.integers(16)) if gtype is None else gtype
    h = [ext << 7 | crc << 6 | seg << 5 | ua << 4 | gtype, (ci & 15) << 4 | (rep & 15)]
    if ext:
        h += [int(rng.integers(256)), int(rng.integers(256))]
    if seg:
        n = int(rng.integers(1 << 16))
        h += [n >> 8, n & 0xFF]
    if ua:
        t = pick(tid)
        extra = int(rng.integers(0, 4))
        li = (2 if t else 0) + extra
        h += [int(rng.integers(8)) << 5 | t << 4 | li] + [int(x) for x in rng.integers(0, 256, li)]
    body = size - len(h) - (2 if crc else 0)
    assert body >= 0, (size, len(h))
    g = bytes(h) + bytes(rng.integers(0, 256, body, dtype=np.uint8))
    if crc:
        c = crc16(g) ^ 0xFFFF
        g += bytes([c >> 8, c & 0xFF])
    return np.frombuffer(g, dtype=np.uint8).copy()


def parse_group(address, b):
    """The record of a complete group: a dict with the fields of dabhip_packet_group."""
    b = [int(x) for x in b]
    g = dict(address=address, length=len(b), ext_flag=0, crc_flag=0, seg_flag=0, ua_flag=0, type=0, continuity=0, repetition=0, crc_ok=0, ext_field=0,
             last_segment=0, header_ok=0, segment_number=-1, transport_id=-1)
    if len(b) < 2:
        return g
    g.update(ext_flag=b[0] >> 7, crc_flag=b[0] >> 6 & 1, seg_flag=b[0] >> 5 & 1, ua_flag=b[0] >> 4 & 1, type=b[0] & 15, continuity=b[1] >> 4, repetition=b[1] & 15)
    if g["crc_flag"] and len(b) >= 4:
        g["crc_ok"] = int((crc16(b[:-2]) ^ 0xFFFF) == (b[-2] << 8 | b[-1]))
    end = len(b) - (2 if g["crc_flag"] else 0)
    at = 2
    if at + 2 * g["ext_flag"] + 2 * g["seg_flag"] + g["ua_flag"] > end:
        return g
    f = {}
    if g["ext_flag"]:
        f["ext_field"] = b[at] << 8 | b[at + 1]
        at += 2
    if g["seg_flag"]:
        f["last_segment"], f["segment_number"] = b[at] >> 7, (b[at] & 0x7F) << 8 | b[at + 1]
        at += 2
    if g["ua_flag"]:
        tflag, li = b[at] >> 4 & 1, b[at] & 15
        at += 1
        if at + li > end or (tflag and li < 2):
            return g
        if tflag:
            f["transport_id"] = b[at] << 8 | b[at + 1]
    g.update(f, header_ok=1)
    return g


GROUP_STATS = ("groups", "dropped", "orphan_packets", "crc_fails")


class Groups:
    """The data-group rule over the records of one lane: push(records, data) -> [(record dict, bytes)]."""

    def __init__(self):
        self.open = {}
        self.stats = dict.fromkeys(GROUP_STATS, 0)

    def push(self, recs, data):
        done = []
        for (_, address, _, ci, fl, cmd, ul, _), useful in zip(recs, data):
            assert len(useful) == ul
            if address == 0 or cmd:
                continue
            if fl & 2:
                if address in self.open:
                    self.stats["dropped"] += 1
                self.open[address] = [b"", ci]
            elif address not in self.open:
                self.stats["orphan_packets"] += 1
                continue
            elif (self.open[address][1] + 1) % 4 != ci:
                self.stats["dropped"] += 1
                del self.open[address]
                continue
            o = self.open[address]
            o[1] = ci
            if len(o[0]) + ul > MAX_GROUP:
                self.stats["dropped"] += 1
                del self.open[address]
                continue
            o[0] += bytes(useful)
            if fl & 1:
                g = parse_group(address, o[0])
                self.stats["groups"] += 1
                self.stats["crc_fails"] += 1 if g["crc_flag"] and not g["crc_ok"] else 0
                done.append((g, np.frombuffer(o[0], dtype=np.uint8).copy()))
                del self.open[address]
        return done

    def stat_list(self):
        return [self.stats[k] for k in GROUP_STATS]
