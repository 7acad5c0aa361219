"""EDI in (dabhip.h: dabhip_edirx) restated in plain numpy / Python: what makes a packet, the window over sequence numbers, PFT reassembly,
RS(255,207) erasure recovery, the AF checks, the TAG walk and the rebuild of the ETI(NI) frame.  It shares no code with edi_model.unpack nor
with csrc/edirx_plan.hpp.  The erasure decoder differs in method from the kernel's (locator and Forney): it solves the 48 syndrome equations
for the unknown bytes by elimination over GF(256); an inconsistent system is what the kernel sees as a syndrome left after filling.

Receiver is one stream: push(packets) / flush() -> [(frame bytes, record)] in output order, .stats the counters; record = (frame number, seq,
fcth, fct, fragments received, fragments expected, words filled, erasures filled)."""
import numpy as np

ETI_BYTES = 6144
STATS = ("packets", "bad_packets", "late", "duplicates", "mismatched", "missing", "groups_incomplete", "groups_rs_failed", "groups_crc_failed",
         "groups_refused", "words_filled", "erasures_filled", "items_ignored", "with_atst", "frames")
MAX_PAYLOAD = 8160 + 256

# ---- arithmetic ------------------------------------------------------------------------------------------------------------------------------------
_CRC = []
for _v in range(256):
    _r = _v << 8
    for _ in range(8):
        _r = ((_r << 1) ^ 0x1021) & 0xFFFF if _r & 0x8000 else (_r << 1) & 0xFFFF
    _CRC.append(_r)


def crc(data):
    r = 0xFFFF
    for b in data:
        r = ((r << 8) & 0xFFFF) ^ _CRC[(r >> 8) ^ b]
    return r ^ 0xFFFF


ALOG = np.zeros(255, np.int64)                         # alpha^i
LOG = np.zeros(256, np.int64)
_x = 1
for _i in range(255):
    ALOG[_i] = _x
    LOG[_x] = _i
    _x = (_x << 1) ^ (0x11D if _x & 0x80 else 0)


def gmul(a, b):
    """element-wise product in GF(256)"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.where((a == 0) | (b == 0), 0, ALOG[(LOG[a] + LOG[b]) % 255])


# row i: the weight of byte j (the coefficient of x^(254 - j)) in syndrome i: alpha^(i (254 - j))
WEIGHT = ALOG[(np.arange(48)[:, None] * (254 - np.arange(255))[None, :]) % 255]


def syndromes(word):
    return np.bitwise_xor.reduce(gmul(WEIGHT, np.asarray(word, np.int64)[None, :]), axis=1)


def fill_erasures(word, places):
    """word: 255 bytes with anything at `places`; -> the word with those bytes solved from the 48 syndrome equations, or None when they
    contradict each other (an error beside the erasures).  More than 48 places cannot be asked for."""
    places = list(places)
    if len(places) > 48:
        raise ValueError("more than 48 erasures")
    word = np.array(word, np.int64)
    word[places] = 0
    n = len(places)
    m = np.concatenate([WEIGHT[:, places], syndromes(word)[:, None]], axis=1)       # 48 equations, n unknowns, the right side last
    row = 0
    for col in range(n):
        piv = next((r for r in range(row, 48) if m[r, col]), None)
        if piv is None:
            return None                                # (cannot happen: the columns are independent)
        m[[row, piv]] = m[[piv, row]]
        inv = ALOG[(255 - LOG[m[row, col]]) % 255]
        m[row] = gmul(m[row], inv)
        factor = m[:, col].copy()
        factor[row] = 0
        m ^= gmul(m[row][None, :], factor[:, None])
        row += 1
    if m[n:, n].any():
        return None
    word[places] = m[:n, n]
    return word.astype(np.uint8)


def _u(b):
    return int.from_bytes(b, "big")


# ---- a packet --------------------------------------------------------------------------------------------------------------------------------------
def check_packet(p):
    """-> dict(kind 'AF' | 'PF' | 'FEC', q, findex, fcount, plen, rsk, rsz, payload) or None"""
    p = bytes(p)
    n = len(p)
    if n < 12:
        return None
    if p[:2] == b"AF":
        if _u(p[2:6]) + 12 != n or p[8] & 0xF0 != 0x90 or p[9:10] != b"T":
            return None
        return dict(kind="AF", q=_u(p[6:8]), findex=0, fcount=1, plen=n, rsk=0, rsz=0, payload=p)
    if p[:2] != b"PF" or n < 14:
        return None
    word = _u(p[10:12])
    fec, addr, plen = word >> 15, (word >> 14) & 1, word & 0x3FFF
    head = 16 if fec else 14
    findex, fcount = _u(p[4:7]), _u(p[7:10])
    if n != head + plen or addr or not 1 <= plen <= 1472 or not 1 <= fcount <= 256 or findex >= fcount:
        return None
    if crc(p[:head - 2]) != _u(p[head - 2:head]):
        return None
    rsk = rsz = 0
    if fec:
        rsk, rsz = p[12], p[13]
        if not 1 <= rsk <= 207:
            return None
        c = fcount * plen // (rsk + 48)
        if not 1 <= c <= 32 or rsz >= c:
            return None
    return dict(kind="FEC" if fec else "PF", q=_u(p[2:4]), findex=findex, fcount=fcount, plen=plen, rsk=rsk, rsz=rsz, payload=p[head:])


def m_max(rsk, fcount):
    return 48 // -(-(rsk + 48) // fcount)


def word_erasures(held, fcount, rsk, w):
    """the places (0..254) of code word w's bytes that lie in fragments not held"""
    cw = rsk + 48
    out = []
    for t in range(cw):
        if (w * cw + t) % fcount not in held:
            out.append(t if t < rsk else 207 + t - rsk)
    return out


# ---- the TAG walk and the frame --------------------------------------------------------------------------------------------------------------------
def walk(af):
    """the fields of an AF packet whose "AF", LEN and CRC are right, as edi_model.carried gives them for a frame (and fcth, atstf, ignored);
    None when it is refused"""
    af = bytes(af)
    at, end = 10, len(af) - 2
    d = {"stc": [], "sub": [], "ignored": 0}
    while end - at >= 8:
        name, bits = af[at:at + 4], _u(af[at + 4:at + 8])
        if bits % 8 or at + 8 + bits // 8 > end:
            return None
        v = af[at + 8:at + 8 + bits // 8]
        at += 8 + len(v)
        if name == b"*ptr":
            if len(v) != 8 or v[:4] != b"DETI":
                return None
        elif name == b"deti":
            if "fct" in d or len(v) < 6:
                return None
            a, b = _u(v[:2]), _u(v[2:6])
            atstf, ficf, rfudf = a >> 15, (a >> 14) & 1, (a >> 13) & 1
            if len(v) != 6 + 8 * atstf + 96 * ficf + 3 * rfudf:
                return None
            d.update(atstf=atstf, ficf=ficf, fcth=(a >> 8) & 31, fct=a & 255, err=b >> 24, mid=(b >> 22) & 3, fp=(b >> 19) & 7, mnsc=b & 0xFFFF,
                     fic=v[6 + 8 * atstf:6 + 8 * atstf + 96 * ficf])
        elif name[:3] == b"est":
            if name[3] != len(d["stc"]) + 1 or len(d["stc"]) >= 64 or len(v) < 3 or (len(v) - 3) % 8 or (len(v) - 3) // 8 > 1023:
                return None
            w = _u(v[:3])
            d["stc"].append((w >> 18, (w >> 8) & 0x3FF, (w >> 2) & 0x3F, (len(v) - 3) // 8))
            d["sub"].append(v[3:])
        else:
            d["ignored"] += 1
    if any(af[at:end]) or "fct" not in d or (d["ficf"] and d["mid"] != 1):
        return None
    d["nst"] = len(d["stc"])
    if 12 + 4 * d["nst"] + 96 * d["ficf"] + 8 * sum(s[3] for s in d["stc"]) > 6140:
        return None
    return d


def rebuild(d):
    """the ETI(NI) frame of the fields (edi_model.carried's keys)"""
    fct, nst = d["fct"], d["nst"]
    fl = nst + 1 + 24 * d["ficf"] + 2 * sum(s[3] for s in d["stc"])
    head = bytes([fct, (d["ficf"] << 7) | nst, (d["fp"] << 5) | (d["mid"] << 3) | (fl >> 8), fl & 255])
    for scid, sad, tpl, stl in d["stc"]:
        head += ((scid << 26) | (sad << 16) | (tpl << 10) | stl).to_bytes(4, "big")
    head += d["mnsc"].to_bytes(2, "big")
    mst = bytes(d["fic"]) + b"".join(bytes(s) for s in d["sub"])
    f = bytes([d["err"]]) + (b"\xf8\xc5\x49" if fct & 1 else b"\x07\x3a\xb6") + head + crc(head).to_bytes(2, "big") + mst + crc(mst).to_bytes(2, "big") + b"\xff" * 6
    f = (f + b"\x55" * ETI_BYTES)[:ETI_BYTES]
    return np.frombuffer(f, np.uint8)


def af_to_frame(af):
    """(verdict, fields): 'crc' | 'refused' | 'frame'"""
    af = bytes(af)
    if len(af) < 12 or af[:2] != b"AF" or _u(af[2:6]) + 12 != len(af) or af[8] & 0xF0 != 0x90 or af[9:10] != b"T" or crc(af[:-2]) != _u(af[-2:]):
        return "crc", None
    d = walk(af)
    return ("refused", None) if d is None else ("frame", d)


# ---- one stream ------------------------------------------------------------------------------------------------------------------------------------
class Receiver:
    def __init__(self, depth=4):
        self.depth = depth
        self.stats = dict.fromkeys(STATS, 0)
        self.reset()

    def reset(self):
        self.next, self.groups = None, {}

    def stat_list(self):
        return [self.stats[k] for k in STATS]

    def push(self, packets):
        out = []
        for p in packets:
            self._packet(bytes(p), out)
        return out

    def flush(self):
        out = []
        order = sorted(self.groups, key=lambda s: (s - self.next) % 65536)
        for s in order:
            self._finalise(s, out)
        if order:
            self.next = (order[-1] + 1) % 65536
        return out

    @staticmethod
    def _ready(g):
        if g["kind"] == "FEC":
            return len(g["frags"]) >= g["fcount"] - m_max(g["rsk"], g["fcount"])
        return len(g["frags"]) == g["fcount"]

    def _packet(self, p, out):
        st = self.stats
        st["packets"] += 1
        h = check_packet(p)
        if h is None:
            st["bad_packets"] += 1
            return
        q = h["q"]
        if self.next is None:
            self.next = q
        d = (q - self.next) % 65536
        if d >= 32768:
            st["late"] += 1
            return
        if d >= self.depth:
            n = d - self.depth + 1
            leaving = sorted((s for s in self.groups if (s - self.next) % 65536 < n), key=lambda s: (s - self.next) % 65536)
            for s in leaving:
                self._finalise(s, out)
            st["missing"] += n - len(leaving)
            self.next = (self.next + n) % 65536
        g = self.groups.get(q)
        fixed = (h["kind"], h["fcount"], h["rsk"], h["rsz"], h["plen"] if h["kind"] == "FEC" else 0)
        last = h["kind"] == "PF" and h["fcount"] > 1 and h["findex"] == h["fcount"] - 1
        reach = h["fcount"] * h["plen"] if h["kind"] == "FEC" else 0 if last else (h["findex"] + 1) * h["plen"]
        if g is not None and g["fixed"] != fixed:
            st["mismatched"] += 1
        elif g is not None and h["findex"] in g["frags"]:
            st["duplicates"] += 1
        elif reach > MAX_PAYLOAD:
            st["mismatched"] += 1
        else:
            if g is None:
                g = self.groups[q] = dict(fixed=fixed, kind=h["kind"], fcount=h["fcount"], rsk=h["rsk"], rsz=h["rsz"], plen=h["plen"], seq=q, frags={})
            g["frags"][h["findex"]] = h["payload"]
        while self.next in self.groups and len(self.groups[self.next]["frags"]) == self.groups[self.next]["fcount"]:
            self._finalise(self.next, out)
            self.next = (self.next + 1) % 65536

    def _finalise(self, s, out):
        st = self.stats
        g = self.groups.pop(s)
        if not self._ready(g):
            st["groups_incomplete"] += 1
            return
        f, frags = g["fcount"], g["frags"]
        words = erasures = 0
        if g["kind"] == "AF":
            af = frags[0]
        elif g["kind"] == "PF":
            parts = [frags[i] for i in range(f)]
            if f > 1 and (len({len(x) for x in parts[:-1]}) != 1 or len(parts[-1]) > len(parts[0]) or sum(len(x) for x in parts) > MAX_PAYLOAD):
                st["groups_refused"] += 1
                return
            af = b"".join(parts)
        else:
            k, plen = g["rsk"], g["plen"]
            cw = k + 48
            c = f * plen // cw
            block = np.zeros(f * plen, np.uint8)
            for i, x in frags.items():
                block[i::f] = np.frombuffer(x, np.uint8)
            held = set(frags)
            data = []
            for w in range(c):
                word = np.zeros(255, np.uint8)
                word[:k] = block[w * cw:w * cw + k]
                word[207:] = block[w * cw + k:(w + 1) * cw]
                places = word_erasures(held, f, k, w) if len(held) < f else []
                if places:
                    word = fill_erasures(word, places)
                    if word is None:
                        st["groups_rs_failed"] += 1
                        return
                    words += 1
                    erasures += len(places)
                data.append(word[:k].tobytes())
            af = b"".join(data)
            af = af[:len(af) - g["rsz"]]
            st["words_filled"] += words
            st["erasures_filled"] += erasures
        verdict, d = af_to_frame(af)
        if verdict == "crc":
            st["groups_crc_failed"] += 1
            return
        if verdict == "refused":
            st["groups_refused"] += 1
            return
        st["items_ignored"] += d["ignored"]
        st["with_atst"] += d["atstf"]
        out.append((rebuild(d), (st["frames"], g["seq"], d["fcth"], d["fct"], len(frags), f, words, erasures)))
        st["frames"] += 1


def receive(packets, depth=4):
    """one stream pushed whole and flushed -> ([frames], [records], stats)"""
    r = Receiver(depth)
    out = r.push(packets) + r.flush()
    return [x[0] for x in out], [x[1] for x in out], r.stat_list()
