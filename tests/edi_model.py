"""EDI out of ETI (dabhip.h: dabhip_edi) restated in plain numpy, in two halves that share no code.

pack: ETI frames -> the bytes, records and counters the GPU stage must give (class Stream), with the size rule (plan) and the pieces the
known-answer tests look at (crc16, GEN, rs_parity).  Arithmetic by tables: a 256-entry CRC table, exp / log tables of GF(256).

unpack: the bytes -> what a receiver sees.  It reads the PF headers, de-interleaves, finds c = floor(f s / (k + 48)) from the header alone,
checks every code word by its 48 syndromes (shift-and-reduce arithmetic, no tables), checks HCRC and the AF CRC bit by bit, parses the TAG
items and rebuilds the carried fields of every ETI frame; carried() reads the same fields from a frame for the comparison.

The rules were written from ETSI TS 102 693 and TS 102 821 as remembered; there is no copy of either nor a second EDI implementation behind
this file.  What dabhip.h, this model and the kernels agree on is what counts."""
import numpy as np

ETI_BYTES = 6144
MST_END = 6140
RS_N, RS_K, RS_P = 255, 207, 48
STATS = ("frames", "frames_skipped", "frames_without_fic", "packets", "bytes_out", "chunks_encoded")
MAX_L = 6620

# ================================================================ pack ============================================================================
_CRC_TABLE = np.zeros(256, np.uint16)
for _v in range(256):
    _r = _v << 8
    for _ in range(8):
        _r = ((_r << 1) ^ 0x1021) & 0xFFFF if _r & 0x8000 else (_r << 1) & 0xFFFF
    _CRC_TABLE[_v] = _r


def crc16(data):
    r = 0xFFFF
    for b in bytes(data):
        r = ((r << 8) & 0xFFFF) ^ int(_CRC_TABLE[(r >> 8) ^ b])
    return r ^ 0xFFFF


def _crc16_many(packets):
    """crc16 of every byte string, all at once: one table step per byte position"""
    if not packets:
        return []
    lens = np.array([len(p) for p in packets])
    buf = np.zeros((len(packets), int(lens.max())), np.uint8)
    for i, p in enumerate(packets):
        buf[i, :len(p)] = np.frombuffer(p, np.uint8)
    r = np.full(len(packets), 0xFFFF, np.uint16)
    for pos in range(buf.shape[1]):
        nxt = ((r << 8) & 0xFFFF) ^ _CRC_TABLE[(r >> 8) ^ buf[:, pos]]
        r = np.where(pos < lens, nxt, r).astype(np.uint16)
    return [int(x) ^ 0xFFFF for x in r]


_EXP = np.zeros(512, np.int64)
_LOG = np.zeros(256, np.int64)
_x = 1
for _i in range(255):
    _EXP[_i] = _x
    _LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11D
_EXP[255:510] = _EXP[:255]


def _mul(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.where((a == 0) | (b == 0), 0, _EXP[_LOG[a] + _LOG[b]]).astype(np.uint8)


def _generator():
    g = np.array([1], np.uint8)                       # g[i] = coefficient of x^i
    for i in range(RS_P):
        root = _EXP[i]
        g = np.concatenate([[0], g]).astype(np.uint8) ^ np.concatenate([_mul(g, root), [0]]).astype(np.uint8)
    return g


GEN = _generator()                                     # 49 coefficients, GEN[48] = 1


def rs_parity(chunks):
    """chunks: (n, k) bytes, k <= 207 -> (n, 48) parity bytes of (chunk, 207 - k zeros) x^48 mod g, by the feedback register"""
    chunks = np.atleast_2d(np.asarray(chunks, np.uint8))
    n, k = chunks.shape
    msg = np.zeros((n, RS_K), np.uint8)
    msg[:, :k] = chunks
    low = GEN[RS_P - 1::-1]                            # coefficients of x^47 .. x^0
    reg = np.zeros((n, RS_P), np.uint8)
    for i in range(RS_K):
        fb = msg[:, i] ^ reg[:, 0]
        reg = np.concatenate([reg[:, 1:], np.zeros((n, 1), np.uint8)], axis=1) ^ _mul(fb[:, None], low[None, :])
    return reg


def plan(l, mode, recover=0, max_frag=1400):
    """(c, k, z, B, f, s) of an AF packet of l bytes"""
    if mode == 0:
        return 0, 0, 0, l, 1, l
    if mode == 1:
        return 0, 0, 0, l, -(-l // max_frag), min(l, max_frag)
    c = -(-l // RS_K)
    k = -(-l // c)
    z = c * k - l
    B = c * (k + RS_P)
    s_max = min(RS_P * c // (recover + 1), max_frag)
    f = -(-B // s_max)
    s = -(-B // f)
    return c, k, z, B, f, s


def plan_refused(l, mode, recover, max_frag):
    """which argument dabhip_edi_plan refuses (1 l, 2 mode, 3 recover, 4 max_frag), 0: none"""
    if not 13 <= l <= 1 << 20:
        return 1
    if mode not in (0, 1, 2):
        return 2
    if mode == 2 and not 0 <= recover <= 5:
        return 3
    if mode >= 1 and not 64 <= max_frag <= 1472:
        return 4
    return 0


def _be(v, n):
    return int(v).to_bytes(n, "big")


def _item(name, value):
    return name + _be(8 * len(value), 4) + value


def accepted(f):
    """the frame's (FICF, NST, [STL]) or None when it is skipped"""
    ficf, nst, mid = int(f[5]) >> 7, int(f[5]) & 0x7F, (int(f[6]) >> 3) & 3
    if nst > 64 or (ficf and mid != 1):
        return None
    stl = [((int(f[8 + 4 * i + 2]) & 3) << 8) | int(f[8 + 4 * i + 3]) for i in range(nst)]
    if 12 + 4 * nst + 96 * ficf + 8 * sum(stl) > MST_END:
        return None
    return int(ficf), int(nst), stl


def af_body(f, fcth, seq):
    """the AF packet of an accepted frame without its CRC"""
    f = np.asarray(f, np.uint8)
    ficf, nst, stl = accepted(f)
    raw = f.tobytes()
    at = 12 + 4 * nst
    mnsc = (raw[8 + 4 * nst] << 8) | raw[8 + 4 * nst + 1]
    deti = _be((ficf << 14) | (fcth << 8) | raw[4], 2) + _be((raw[0] << 24) | (((raw[6] >> 3) & 3) << 22) | ((raw[6] >> 5) << 19) | mnsc, 4)
    if ficf:
        deti += raw[at:at + 96]
        at += 96
    tag = _item(b"*ptr", b"DETI" + bytes(4)) + _item(b"deti", deti)
    for i in range(nst):
        e = raw[8 + 4 * i:12 + 4 * i]
        scid, sad, tpl = e[0] >> 2, ((e[0] & 3) << 8) | e[1], e[2] >> 2
        tag += _item(b"est" + bytes([i + 1]), _be((scid << 18) | (sad << 8) | (tpl << 2), 3) + raw[at:at + 8 * stl[i]])
        at += 8 * stl[i]
    tag += bytes(-len(tag) % 8)
    return b"AF" + _be(len(tag), 4) + _be(seq, 2) + b"\x90T" + tag


def pf_header(pseq, findex, fcount, fec, plen, rsk=0, rsz=0):
    h = b"PF" + _be(pseq, 2) + _be(findex, 3) + _be(fcount, 3) + _be((0x8000 if fec else 0) | plen, 2)
    if fec:
        h += bytes([rsk, rsz])
    return h + _be(crc16(h), 2)


class Stream:
    """One stream of the stage: push(frames) -> (bytes, [(offset, length, frame, seq, findex, fcount)]) of that push"""

    def __init__(self, mode=0, recover=0, max_frag=1400, seq0=0):
        self.mode, self.recover, self.max_frag, self.seq0 = mode, recover, max_frag, seq0
        self.nframes = 0
        self.stats = dict.fromkeys(STATS, 0)
        self.reset()

    def reset(self):
        self.started, self.last_fct, self.fcth, self.seq = False, 0, 0, self.seq0

    def stat_list(self):
        return [self.stats[k] for k in STATS]

    def push(self, frames):
        bodies, numbers, seqs = [], [], []
        for f in frames:
            number = self.nframes
            self.nframes += 1
            self.stats["frames"] += 1
            a = accepted(f)
            if a is None:
                self.stats["frames_skipped"] += 1
                continue
            fct = int(f[4])
            if self.started and fct < self.last_fct:
                self.fcth = (self.fcth + 1) % 20
            self.started, self.last_fct = True, fct
            self.stats["frames_without_fic"] += 1 - a[0]
            bodies.append(af_body(f, self.fcth, self.seq))
            numbers.append(number)
            seqs.append(self.seq)
            self.seq = (self.seq + 1) & 0xFFFF
        packets = [b + _be(c, 2) for b, c in zip(bodies, _crc16_many(bodies))]
        parity = self._parity(packets) if self.mode == 2 else None
        out, recs = [], []
        at = 0
        for n, (af, number, seq) in enumerate(zip(packets, numbers, seqs)):
            l = len(af)
            c, k, z, B, f, s = plan(l, self.mode, self.recover, self.max_frag)
            if self.mode == 0:
                frags = [af]
            elif self.mode == 1:
                frags = [pf_header(seq, i, f, 0, len(af[i * s:(i + 1) * s])) + af[i * s:(i + 1) * s] for i in range(f)]
            else:
                data = np.frombuffer(af + bytes(z), np.uint8).reshape(c, k)
                block = np.concatenate([data, parity[n]], axis=1).reshape(-1)
                grid = np.concatenate([block, np.zeros(f * s - B, np.uint8)]).reshape(s, f)
                frags = [pf_header(seq, i, f, 1, s, k, z) + grid[:, i].tobytes() for i in range(f)]
                self.stats["chunks_encoded"] += c
            for i, p in enumerate(frags):
                recs.append((at, len(p), number, seq, i, len(frags)))
                at += len(p)
            out += frags
        self.stats["packets"] += len(recs)
        self.stats["bytes_out"] += at
        return np.frombuffer(b"".join(out), np.uint8), recs

    def _parity(self, packets):
        """per packet its (c, 48) parity bytes; the chunks of one k go through the register together"""
        by_k, out = {}, [None] * len(packets)
        for n, af in enumerate(packets):
            c, k, z = plan(len(af), 2, self.recover, self.max_frag)[:3]
            by_k.setdefault(k, []).append((n, np.frombuffer(af + bytes(z), np.uint8).reshape(c, k)))
        for k, group in by_k.items():
            par = rs_parity(np.concatenate([d for _, d in group]))
            at = 0
            for n, d in group:
                out[n] = par[at:at + len(d)]
                at += len(d)
        return out


def pack(frames, mode=0, recover=0, max_frag=1400, seq0=0):
    return Stream(mode, recover, max_frag, seq0).push(frames)


# ================================================================ unpack ==========================================================================
def _bit_crc(rows, lens):
    """the complemented CRC register of every row's first lens[i] bytes, bit by bit"""
    r = np.full(len(rows), 0xFFFF, np.uint32)
    for pos in range(rows.shape[1]):
        live = pos < lens
        x = r ^ (rows[:, pos].astype(np.uint32) << 8)
        for _ in range(8):
            x = np.where(x & 0x8000, (x << 1) ^ 0x1021, x << 1) & 0xFFFF
        r = np.where(live, x, r)
    return r ^ 0xFFFF


def _check_crcs(messages, what):
    """every message ends with the CRC of what is in front of it"""
    if not messages:
        return
    lens = np.array([len(m) - 2 for m in messages])
    rows = np.zeros((len(messages), int(lens.max())), np.uint8)
    for i, m in enumerate(messages):
        rows[i, :lens[i]] = np.frombuffer(m[:-2], np.uint8)
    got = _bit_crc(rows, lens)
    want = np.array([(m[-2] << 8) | m[-1] for m in messages])
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s CRC fails at %s" % (what, bad[:5])


_SYNDROME_BITS = None


def _syndrome_bits():
    """Multiplying by a constant is linear over GF(2): bit b of byte j of a word adds alpha^b alpha^(i (254 - j)) to syndrome i.  Those constants,
    from alpha by shifting and reducing (x <- 2 x, minus 0x11D when it passes 8 bits), as a 0/1 matrix: (255 * 8 word bits) x (48 * 8 syndrome bits)."""
    global _SYNDROME_BITS
    if _SYNDROME_BITS is None:
        powers, x = [], 1
        for _ in range(255):
            powers.append(x)
            x <<= 1
            if x & 0x100:
                x ^= 0x11D
        assert x == 1 and len(set(powers)) == 255
        powers = np.array(powers, np.uint8)
        j, b, i = np.meshgrid(np.arange(RS_N), np.arange(8), np.arange(RS_P), indexing="ij")
        consts = powers[(i * (RS_N - 1 - j) + b) % 255].reshape(RS_N * 8, RS_P)
        _SYNDROME_BITS = np.unpackbits(consts[:, :, None], axis=2, bitorder="little").reshape(RS_N * 8, RS_P * 8).astype(np.float32)
    return _SYNDROME_BITS


def syndromes(words):
    """(n, 255) -> (n, 48): word(alpha^i), i = 0..47, byte j the coefficient of x^(254 - j)"""
    words = np.asarray(words, np.uint8).reshape(-1, RS_N)
    bits = np.unpackbits(words[:, :, None], axis=2, bitorder="little").reshape(len(words), RS_N * 8).astype(np.float32)
    sums = bits @ _syndrome_bits()                     # at most 2040 ones per sum: exact in float32
    return np.packbits((sums.astype(np.int64) & 1).astype(np.uint8).reshape(len(words), RS_P, 8), axis=2, bitorder="little").reshape(len(words), RS_P)


def _u(b):
    return int.from_bytes(b, "big")


def split_packets(data, mode):
    """the byte stream -> [(offset, bytes)] of its packets, by their own length fields"""
    data = bytes(data)
    out, at = [], 0
    while at < len(data):
        if mode == 0:
            assert data[at:at + 2] == b"AF", at
            n = _u(data[at + 2:at + 6]) + 12
        else:
            assert data[at:at + 2] == b"PF", at
            word = _u(data[at + 10:at + 12])
            assert bool(word & 0x8000) == (mode == 2) and not word & 0x4000, at
            n = (16 if mode == 2 else 14) + (word & 0x3FFF)
        assert at + n <= len(data), "a packet runs past the end"
        out.append((at, data[at:at + n]))
        at += n
    return out


def reassemble(data, mode):
    """-> ([AF packets], [(offset, length, seq, findex, fcount)] per packet of the stream); checks HCRC and every code word"""
    packets = split_packets(data, mode)
    if mode == 0:
        return [p for _, p in packets], [(at, len(p), _u(p[6:8]), 0, 1) for at, p in packets]
    hlen = 16 if mode == 2 else 14
    _check_crcs([p[:hlen] for _, p in packets], "PF header")
    infos, afs, words, group = [], [], [], []
    for at, p in packets:
        pseq, findex, fcount = _u(p[2:4]), _u(p[4:7]), _u(p[7:10])
        infos.append((at, len(p), pseq, findex, fcount))
        assert findex == len(group) and (not group or (pseq, fcount) == group[0][:2]), ("fragment order", at)
        group.append((pseq, fcount, p))
        if len(group) < fcount:
            continue
        payload = [q[hlen:] for _, _, q in group]
        if mode == 1:
            assert all(len(x) == len(payload[0]) for x in payload[:-1]) and len(payload[-1]) <= len(payload[0])
            afs.append(b"".join(payload))
        else:
            k, z, s = p[12], p[13], len(payload[0])
            assert all(len(x) == s and q[12:14] == p[12:14] for x, (_, _, q) in zip(payload, group))
            block = np.stack([np.frombuffer(x, np.uint8) for x in payload], axis=1).reshape(-1)      # byte j of fragment i -> j f + i
            c = fcount * s // (k + RS_P)
            assert c >= 1 and not block[c * (k + RS_P):].any(), "bytes behind the RS block"
            rows = block[:c * (k + RS_P)].reshape(c, k + RS_P)
            word = np.zeros((c, RS_N), np.uint8)
            word[:, :k] = rows[:, :k]
            word[:, RS_K:] = rows[:, k:]
            words.append(word)
            flat = rows[:, :k].reshape(-1)
            assert z < c and not flat[c * k - z:].any(), "RSz"
            afs.append(flat[:c * k - z].tobytes())
        group = []
    assert not group, "a packet is short of fragments"
    if words:
        assert not syndromes(np.concatenate(words)).any(), "a code word has a syndrome"
    return afs, infos


def parse_af(af):
    """the fields an AF packet carries (its CRC is checked by the caller)"""
    assert af[:2] == b"AF" and af[8:10] == b"\x90T" and _u(af[2:6]) + 12 == len(af)
    out = {"seq": _u(af[6:8]), "stc": [], "sub": []}
    at, end = 10, len(af) - 2
    names = []
    while end - at >= 8:
        name, bits = af[at:at + 4], _u(af[at + 4:at + 8])
        assert bits % 8 == 0 and at + 8 + bits // 8 <= end, name
        value = af[at + 8:at + 8 + bits // 8]
        at += 8 + bits // 8
        names.append(name)
        if name == b"*ptr":
            assert value == b"DETI" + bytes(4)
        elif name == b"deti":
            a, b = _u(value[:2]), _u(value[2:6])
            assert not a & 0xA000 and not b & 0x30000 and len(value) == (102 if a & 0x4000 else 6)
            out.update(ficf=(a >> 14) & 1, fcth=(a >> 8) & 31, fct=a & 255, err=b >> 24, mid=(b >> 22) & 3, fp=(b >> 19) & 7, mnsc=b & 0xFFFF, fic=value[6:])
        else:
            assert name[:3] == b"est" and name[3] == len(out["stc"]) + 1 and (len(value) - 3) % 8 == 0
            w = _u(value[:3])
            assert not w & 3
            out["stc"].append((w >> 18, (w >> 8) & 0x3FF, (w >> 2) & 0x3F, (len(value) - 3) // 8))
            out["sub"].append(value[3:])
    assert names[:2] == [b"*ptr", b"deti"] and not any(af[at:end]) and len(af[10:end]) % 8 == 0, "TAG packet order / padding"
    out["nst"] = len(out["stc"])
    return out


def unpack(data, mode):
    """-> ([fields of every frame the stream carries], [(offset, length, seq, findex, fcount)] of its packets)"""
    afs, infos = reassemble(data, mode)
    _check_crcs(afs, "AF")
    return [parse_af(a) for a in afs], infos


def carried(f):
    """the same fields read from an ETI frame (without fcth and seq)"""
    f = bytes(np.asarray(f, np.uint8))
    ficf, nst = f[5] >> 7, f[5] & 0x7F
    out = {"err": f[0], "fct": f[4], "ficf": ficf, "nst": nst, "fp": f[6] >> 5, "mid": (f[6] >> 3) & 3, "mnsc": _u(f[8 + 4 * nst:10 + 4 * nst]), "stc": [], "sub": []}
    at = 12 + 4 * nst
    out["fic"] = f[at:at + 96 * ficf]
    at += 96 * ficf
    for i in range(nst):
        w = _u(f[8 + 4 * i:12 + 4 * i])
        out["stc"].append((w >> 26, (w >> 16) & 0x3FF, (w >> 10) & 0x3F, w & 0x3FF))
        out["sub"].append(f[at:at + 8 * (w & 0x3FF)])
        at += 8 * (w & 0x3FF)
    return out


def same_fields(got, frame):
    want = carried(frame)
    return all(got[k] == want[k] for k in want)
