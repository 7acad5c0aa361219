"""Plain-numpy restatement of the DAB+ audio stage (ETSI TS 102 563): the GF(256) arithmetic and the Reed-Solomon RS(120,110) code of the
audio superframe, its virtual interleaving, the fire code, the AU CRC, the superframe header, the superframe sync rule of libdabhip's DAB+
consumer (csrc/dabplus.hpp, include/dabhip.h) and ADTS framing.  Written independently of the HIP kernels and the synthetic modulator; the tests hold
both of them against it."""
import numpy as np

PRIM = 0x11D                          # x^8 + x^4 + x^3 + x^2 + 1
NROOTS = 10                           # generator prod (x + alpha^i), i = 0..9
T = NROOTS // 2
N_SHORT = 120                         # RS(120,110), shortened from RS(255,245)
K_SHORT = 110
SYNC_FAIL_LIMIT = 3                   # K: consecutive candidates with a failing raw fire code lose sync
FCT_MOD = 250
ETI_BYTES = 6144

EXP = np.zeros(512, dtype=np.int64)
LOG = np.zeros(256, dtype=np.int64)
_x = 1
for _i in range(255):
    EXP[_i] = _x
    LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= PRIM
EXP[255:510] = EXP[0:255]
LOG[0] = -1


def gmul(a, b):
    if a == 0 or b == 0:
        return 0
    return int(EXP[LOG[a] + LOG[b]])


def ginv(a):
    return int(EXP[255 - LOG[a]])


def gpow(a, n):
    if a == 0:
        return 0
    return int(EXP[(LOG[a] * n) % 255])


def poly_eval(p, x):
    """p[0] highest degree."""
    y = 0
    for c in p:
        y = gmul(y, x) ^ int(c)
    return y


def generator():
    """g(x) = prod_{i=0..9} (x + alpha^i), highest degree first (monic, 11 coefficients)."""
    g = [1]
    for i in range(NROOTS):
        r = int(EXP[i])
        out = g + [0]
        for k in range(1, len(out)):
            out[k] ^= gmul(g[k - 1], r)
        g = out
    return g


GEN = generator()


def rs_encode(data):
    """110 data bytes -> the 10 parity bytes (systematic: codeword = data + parity, data[0] the highest-degree coefficient)."""
    data = [int(b) for b in data]
    assert len(data) == K_SHORT
    rem = [0] * NROOTS
    for d in data:
        fb = d ^ rem[0]
        rem = rem[1:] + [0]
        if fb:
            for k in range(NROOTS):
                rem[k] ^= gmul(fb, GEN[k + 1])
    return np.array(rem, dtype=np.uint8)


def syndromes(cw):
    """S_i = r(alpha^i), i = 0..9, byte 0 = coefficient of x^119."""
    return [poly_eval(cw, int(EXP[i])) for i in range(NROOTS)]


def rs_decode(cw):
    """Bounded-distance decoding: (corrected codeword, symbols corrected) when a codeword lies within Hamming distance 5 of cw, else (cw
    unchanged, -1).  Berlekamp-Massey, Chien search over the 120 live positions, Forney; the result is checked by its syndromes."""
    r = [int(b) for b in cw]
    assert len(r) == N_SHORT
    S = syndromes(r)
    if not any(S):
        return np.array(r, dtype=np.uint8), 0
    # Berlekamp-Massey (lambda lowest degree first)
    lam = [1] + [0] * NROOTS
    B = [1] + [0] * NROOTS
    L, m, b = 0, 1, 1
    for n in range(NROOTS):
        d = S[n]
        for i in range(1, L + 1):
            d ^= gmul(lam[i], S[n - i])
        if d == 0:
            m += 1
            continue
        coef = gmul(d, ginv(b))
        Tl = list(lam)
        for i in range(m, NROOTS + 1):
            lam[i] ^= gmul(coef, B[i - m])
        if 2 * L <= n:
            L, B, b, m = n + 1 - L, Tl, d, 1
        else:
            m += 1
    deg = max(i for i in range(NROOTS + 1) if lam[i])
    if deg > T or deg != L:
        return np.array(cw, dtype=np.uint8), -1
    # Chien search: position k (coefficient of x^(119-k)) is in error iff lambda(alpha^-(119-k)) = 0
    roots = []
    for k in range(N_SHORT):
        p = 119 - k
        xinv = int(EXP[(255 - p) % 255])
        v = 0
        for i in range(deg, -1, -1):
            v = gmul(v, xinv) ^ lam[i]
        if v == 0:
            roots.append(k)
    if len(roots) != deg:
        return np.array(cw, dtype=np.uint8), -1
    # Forney (first consecutive root 0): e = X omega(X^-1) / lambda'(X^-1), omega = S lambda mod x^10
    omega = [0] * NROOTS
    for i in range(NROOTS):
        for j in range(0, min(i, deg) + 1):
            omega[i] ^= gmul(S[i - j], lam[j])
    out = list(r)
    for k in roots:
        p = 119 - k
        X = int(EXP[p])
        xinv = int(EXP[(255 - p) % 255])
        num = 0
        for i in range(NROOTS - 1, -1, -1):
            num = gmul(num, xinv) ^ omega[i]
        den = 0
        for i in range(1, deg + 1, 2):               # formal derivative: odd terms, lambda_i x^(i-1)
            den ^= gmul(lam[i], gpow(xinv, i - 1))
        if den == 0:
            return np.array(cw, dtype=np.uint8), -1
        out[k] ^= gmul(X, gmul(num, ginv(den)))
    if any(syndromes(out)):
        return np.array(cw, dtype=np.uint8), -1
    return np.array(out, dtype=np.uint8), len(roots)


# ---- CRCs --------------------------------------------------------------------------------------------
def _crc16(data, poly, init):
    c = init
    for byte in bytes(data):
        c ^= byte << 8
        for _ in range(8):
            c = ((c << 1) ^ poly) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


def fire_code(b2_10):
    """Fire code of superframe bytes 2..10: x^16+x^14+x^13+x^12+x^11+x^5+x^3+x^2+x+1, init 0, no inversion."""
    return _crc16(b2_10, 0x782F, 0)


def fire_ok(sf):
    sf = bytes(sf[:11])
    return fire_code(sf[2:11]) == (sf[0] << 8 | sf[1])


def au_crc(data):
    """CRC-16/GENIBUS (x^16+x^12+x^5+1, init 0xFFFF, inverted): the AU CRC and the FIB CRC."""
    return _crc16(data, 0x1021, 0xFFFF) ^ 0xFFFF


# ---- superframe ------------------------------------------------------------------------------------
AU_LAYOUT = {(0, 1): (2, 5), (0, 0): (4, 8), (1, 1): (3, 6), (1, 0): (6, 11)}   # (dac_rate, sbr_flag) -> (num_aus, start of AU 0)


def pack_superframe(aus, s, dac_rate, sbr_flag, aac_channel_mode=0, ps_flag=0, mpeg_surround_config=0, rfa=0):
    """AU payloads (without their CRC) -> the 110 s unprotected bytes: fire code, header, au_start, AUs each followed by its CRC."""
    n, start0 = AU_LAYOUT[(dac_rate, sbr_flag)]
    assert len(aus) == n
    out = bytearray(K_SHORT * s)
    out[2] = (rfa << 7) | (dac_rate << 6) | (sbr_flag << 5) | (aac_channel_mode << 4) | (ps_flag << 3) | (mpeg_surround_config & 7)
    starts, pos = [], start0
    for a in aus:
        starts.append(pos)
        pos += len(a) + 2
    assert pos == K_SHORT * s, "AUs must fill the superframe"
    bits = 0
    for st in starts[1:]:
        bits = (bits << 12) | st
    nb = 12 * (n - 1)
    nbytes = (nb + 7) // 8
    bits <<= 8 * nbytes - nb
    out[3:3 + nbytes] = bits.to_bytes(nbytes, "big")
    for st, a in zip(starts, aus):
        out[st:st + len(a)] = bytes(a)
        c = au_crc(a)
        out[st + len(a)] = c >> 8
        out[st + len(a) + 1] = c & 0xFF
    f = fire_code(out[2:11])
    out[0], out[1] = f >> 8, f & 0xFF
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


def protect(data):
    """110 s bytes -> 120 s bytes: RS parity of the s interleaved codewords (codeword j = bytes j + k s)."""
    data = np.asarray(data, dtype=np.uint8)
    s = data.size // K_SHORT
    out = np.zeros(N_SHORT * s, dtype=np.uint8)
    out[: K_SHORT * s] = data
    for j in range(s):
        out[K_SHORT * s + j::s] = rs_encode(data[j::s])
    return out


def correct(sf):
    """120 s received bytes -> (110 s data bytes after correction, corrected symbols, failed codewords)."""
    sf = np.asarray(sf, dtype=np.uint8)
    s = sf.size // N_SHORT
    out = sf.copy()
    fixed = failed = 0
    for j in range(s):
        cw, n = rs_decode(sf[j::s])
        if n < 0:
            failed += 1
        else:
            fixed += n
            out[j::s] = cw
    return out[: K_SHORT * s], fixed, failed


def parse(data):
    """110 s corrected bytes -> the record fields: dict(fire_ok, layout_ok, rfa, dac_rate, sbr_flag, aac_channel_mode, ps_flag,
    mpeg_surround_config, num_aus, au_start[6], au_len[6] (AU length including its CRC), crc_ok (bit per AU)).  AUs are only laid out when the fire
    code passes and au_start is strictly increasing with every AU >= 3 bytes inside 110 s."""
    data = np.asarray(data, dtype=np.uint8)
    total = data.size
    b2 = int(data[2])
    r = dict(fire_ok=int(fire_ok(data)), layout_ok=0, rfa=b2 >> 7, dac_rate=(b2 >> 6) & 1, sbr_flag=(b2 >> 5) & 1, aac_channel_mode=(b2 >> 4) & 1,
             ps_flag=(b2 >> 3) & 1, mpeg_surround_config=b2 & 7, au_start=[0] * 6, au_len=[0] * 6, crc_ok=0)
    n, start0 = AU_LAYOUT[(r["dac_rate"], r["sbr_flag"])]
    r["num_aus"] = n
    if not r["fire_ok"]:
        return r
    starts = [start0]
    for i in range(1, n):
        bit = 24 + 12 * (i - 1)
        v = (int(data[bit // 8]) << 8 | int(data[bit // 8 + 1]))
        v = (v >> 4) & 0xFFF if bit % 8 == 0 else v & 0xFFF
        starts.append(v)
    starts.append(total)
    for i in range(n):
        if starts[i + 1] - starts[i] < 3 or starts[i + 1] > total:
            return r
    r["layout_ok"] = 1
    for i in range(n):
        a, e = starts[i], starts[i + 1]
        r["au_start"][i], r["au_len"][i] = a, e - a
        if au_crc(data[a:e - 2]) == (int(data[e - 2]) << 8 | int(data[e - 1])):
            r["crc_ok"] |= 1 << i
    return r


def good_aus(data, rec):
    """The payloads (CRC stripped) of the AUs whose CRC is good, in order."""
    return [bytes(data[rec["au_start"][i]:rec["au_start"][i] + rec["au_len"][i] - 2]) for i in range(rec["num_aus"]) if rec["crc_ok"] >> i & 1]


# ---- ETI frames and the sync rule ---------------------------------------------------------------------
def eti_frame(fct, subs, fill=0x55, ficf=1):
    """An ETI(NI) frame with FCT fct and sub-channels subs = [(SubChId, payload bytes (8 STL of them))]; ficf = 1: 96 FIC bytes (fill) before
    the sub-channels, ficf = 0: none."""
    f = bytearray([fill]) * ETI_BYTES
    odd = fct & 1
    f[0:4] = bytes([0xFF, 0xF8, 0xC5, 0x49]) if odd else bytes([0xFF, 0x07, 0x3A, 0xB6])
    f[4] = fct % FCT_MOD
    nst = len(subs)
    f[5] = (ficf << 7) | nst
    pos = 12 + 4 * nst + 96 * ficf
    for i, (scid, pay) in enumerate(subs):
        stl = len(pay) // 8
        assert len(pay) == 8 * stl
        f[8 + 4 * i] = (scid << 2) & 0xFF
        f[8 + 4 * i + 1] = 0
        f[8 + 4 * i + 2] = (stl >> 8) & 3
        f[8 + 4 * i + 3] = stl & 0xFF
        f[pos:pos + len(pay)] = bytes(pay)
        pos += len(pay)
    assert pos <= ETI_BYTES - 8
    return np.frombuffer(bytes(f), dtype=np.uint8).copy()


def locate(frame, subchid):
    """(present, fct, stl, payload bytes) of a sub-channel in an ETI frame, as the locate kernel reads it.  Present only for a DAB+-capable
    sub-channel: STL > 0, a multiple of 3, at most 216 (s <= 72), and inside the frame."""
    f = np.asarray(frame, dtype=np.uint8)
    fct = int(f[4])
    ficf, nst = int(f[5]) >> 7, int(f[5]) & 0x7F
    off = 12 + 4 * nst + 96 * ficf
    for i in range(nst):
        scid = int(f[8 + 4 * i]) >> 2
        stl = (int(f[8 + 4 * i + 2]) & 3) << 8 | int(f[8 + 4 * i + 3])
        if scid == subchid:
            if stl == 0 or stl % 3 or stl > 216 or off + 8 * stl > ETI_BYTES:
                return False, fct, stl, None
            return True, fct, stl, f[off:off + 8 * stl]
        off += 8 * stl
    return False, fct, 0, None


class SyncModel:
    """The superframe sync of one (stream, sub-channel), carried from push to push.  Unsynced: frame f starts a superframe if its raw fire code
    passes and frames f..f+4 are present with the same STL and consecutive FCT.  Synced: every 5th frame is a candidate, its frames present with
    the locked STL and FCTs continuing the last superframe's; sync is lost on a gap / STL change (search restarts at the candidate's first frame)
    or on the K-th consecutive candidate whose raw fire code fails (search restarts at the next frame).  That candidate is not emitted."""

    def __init__(self, subchid):
        self.subchid = subchid
        self.synced = False
        self.fails = 0
        self.stl = 0
        self.last_fct = -1
        self.pending = []              # frames not yet consumed (at most 4)
        self.losses = 0

    def push(self, frames):
        """frames: the stream's new ETI frames -> list of (first frame's FCT, s, 120 s received bytes) for the superframes it starts."""
        fr = self.pending + [locate(f, self.subchid) for f in frames]
        out = []
        f = 0
        while f + 4 < len(fr):
            win = fr[f:f + 5]
            present = all(w[0] for w in win)
            same = present and all(w[2] == win[0][2] for w in win) and all((win[i][1] + 1) % FCT_MOD == win[i + 1][1] for i in range(4))
            raw = present and fire_ok(win[0][3])
            if not self.synced:
                if same and raw:
                    self.synced, self.fails, self.stl = True, 0, win[0][2]
                    out.append((win[0][1], win[0][2] // 3, np.concatenate([w[3] for w in win])))
                    self.last_fct = win[4][1]
                    f += 5
                else:
                    f += 1
                continue
            if not same or win[0][2] != self.stl or (self.last_fct + 1) % FCT_MOD != win[0][1]:
                self.synced, self.losses = False, self.losses + 1
                continue                                   # search again from this frame
            self.fails = 0 if raw else self.fails + 1
            if self.fails >= SYNC_FAIL_LIMIT:
                self.synced, self.losses = False, self.losses + 1
                f += 1
                continue
            out.append((win[0][1], win[0][2] // 3, np.concatenate([w[3] for w in win])))
            self.last_fct = win[4][1]
            f += 5
        self.pending = fr[f:]
        return out


def stage(sync, frames):
    """The whole stage for one (stream, sub-channel) and one push: [(record dict incl. fct, s, rs_corrected, rs_failed, data bytes)]."""
    recs = []
    for fct, s, raw in sync.push(frames):
        data, fixed, failed = correct(raw)
        r = parse(data)
        r.update(fct=fct, s=s, rs_corrected=fixed, rs_failed=failed, data=data)
        recs.append(r)
    return recs


# ---- ADTS ------------------------------------------------------------------------------------------
def adts_header(au_len, dac_rate, sbr_flag, aac_channel_mode):
    """7-byte ADTS header (MPEG-4, AAC LC, no CRC) in front of an AU of au_len bytes: sampling index of the AAC core rate."""
    core = {(0, 0): 32000, (1, 0): 48000, (0, 1): 16000, (1, 1): 24000}[(dac_rate, sbr_flag)]
    sfi = {48000: 3, 32000: 5, 24000: 6, 16000: 8}[core]
    ch = 2 if aac_channel_mode else 1
    flen = au_len + 7
    return bytes([0xFF, 0xF1, (1 << 6) | (sfi << 2) | (ch >> 2), ((ch & 3) << 6) | ((flen >> 11) & 3), (flen >> 3) & 0xFF,
                  ((flen & 7) << 5) | 0x1F, 0xFC])


def adts_stream(recs):
    """ADTS of every good AU of the records, in order."""
    out = bytearray()
    for r in recs:
        for a in good_aus(r["data"], r):
            out += adts_header(len(a), r["dac_rate"], r["sbr_flag"], r["aac_channel_mode"]) + a
    return bytes(out)
