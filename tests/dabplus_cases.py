"""Crafted inputs for the DAB+ audio stage (ETSI TS 102 563), each with the result known from how it was built: Reed-Solomon words at the
decoder's edges, superframes at the AU kernel's edges, ETI frames at the locate kernel's refusals.  test_dabplus_reference.py holds the CPU
model (dabplus_model.py) and the independent decoder (rs_reference.py) against these expectations, test_gpu_dabplus_edges.py the kernels.

Nothing here calls the model's or the kernels' decoder.  The field arithmetic is a product table made by shift-and-reduce (no log / exp), the
CRCs are byte-wise tables made by polynomial division of small integers; the classes marked "dagger" take their expectation from
rs_reference.decode, every other one from the construction alone."""
import numpy as np

import rs_reference as ref

N, K, NROOTS = 120, 110, 10
ETI_BYTES = 6144
AU_LAYOUT = {(0, 1): (2, 5), (0, 0): (4, 8), (1, 1): (3, 6), (1, 0): (6, 11)}   # (dac_rate, sbr_flag) -> (num_aus, start of AU 0)
LAYOUTS = ((0, 1), (0, 0), (1, 1), (1, 0))
RATES = (1, 2, 3, 11, 12, 71, 72)


# ---- GF(256), vectorised ------------------------------------------------------------------------------------------------------------------
def _mul_table():
    a = np.repeat(np.arange(256, dtype=np.uint16)[:, None], 256, axis=1)
    b = np.arange(256, dtype=np.uint16)[None, :]
    r = np.zeros((256, 256), dtype=np.uint16)
    for bit in range(8):
        r ^= np.where((b >> bit) & 1, a, 0).astype(np.uint16)
        a = a << 1
        a ^= np.where(a & 0x100, 0x11D, 0).astype(np.uint16)
    return r.astype(np.uint8)


MUL = _mul_table()                                     # MUL[a, b] = a b in GF(256)
ALPHA = [ref.power(2, i) for i in range(255)]


def encode_many(data):
    """(n, 110) data bytes -> (n, 10) parity bytes: the systematic encoder's shift register on all rows at once."""
    data = np.asarray(data, dtype=np.uint8).reshape(-1, K)
    rem = np.zeros((data.shape[0], NROOTS), dtype=np.uint8)
    for k in range(K):
        fb = data[:, k] ^ rem[:, 0]
        rem = np.concatenate([rem[:, 1:], np.zeros((data.shape[0], 1), np.uint8)], axis=1)
        for t in range(NROOTS):
            rem[:, t] ^= MUL[fb, ref.GEN[t + 1]]
    return rem


def syndromes_many(words):
    """(n, 120) words -> (n, 10) syndromes S_i = word(alpha^i)."""
    words = np.asarray(words, dtype=np.uint8).reshape(-1, N)
    out = np.zeros((words.shape[0], NROOTS), dtype=np.uint8)
    for i in range(NROOTS):
        row = MUL[ALPHA[i]]
        s = np.zeros(words.shape[0], dtype=np.uint8)
        for k in range(N):
            s = row[s] ^ words[:, k]
        out[:, i] = s
    return out


def protect_many(datas):
    """Unprotected superframes (110 s bytes each, any mix of s) -> protected ones (120 s bytes): codeword j is bytes j + k s."""
    rows = np.concatenate([np.asarray(d, np.uint8).reshape(K, -1).T for d in datas])
    par = encode_many(rows)
    out, at = [], 0
    for d in datas:
        s = len(d) // K
        out.append(np.concatenate([np.asarray(d, np.uint8), par[at:at + s].T.reshape(-1)]))
        at += s
    return out


def codeword(rng):
    d = rng.integers(0, 256, K).astype(np.uint8)
    return np.concatenate([d, ref.encode(d)])


# ---- RS classes -------------------------------------------------------------------------------------------------------------------------------
class RsCase:
    """received = sent ^ pattern.  Expected: dagger -> rs_reference.decode(received); n < 0 -> failure, received unchanged; else the codeword
    sent ^ delta with n symbols corrected (delta is a codeword: zero unless the word is built to be miscorrected)."""

    def __init__(self, cls, label, pattern, n, delta=None, dagger=False):
        self.cls, self.label, self.n, self.dagger = cls, label, n, dagger
        self.pattern = np.asarray(pattern, dtype=np.uint8)
        self.delta = np.zeros(N, np.uint8) if delta is None else np.asarray(delta, dtype=np.uint8)

    def apply(self, sent):
        """-> (received, expected word, expected n)"""
        rx = np.asarray(sent, np.uint8) ^ self.pattern
        if self.dagger:
            w, n = ref.decode(rx)
            return rx, w, n
        if self.n < 0:
            return rx, rx.copy(), -1
        return rx, np.asarray(sent, np.uint8) ^ self.delta, self.n


def _pattern(pos, vals):
    p = np.zeros(N, np.uint8)
    for k, v in zip(pos, vals):
        p[int(k)] = int(v)
    return p


def syndromes_of_virtual(powers, vals):
    """Syndromes of errors vals at locators alpha^powers (powers up to 254: the full-length code's positions)."""
    out = []
    for i in range(NROOTS):
        s = 0
        for p, v in zip(powers, vals):
            s ^= ref.mul(int(v), ref.power(ALPHA[int(p) % 255], i))
        out.append(s)
    return out


def parity_pattern(S):
    """The change of the ten parity bytes alone (powers 0..9, bytes 119..110) that has syndromes S: a Vandermonde solve."""
    d = ref.solve([[ref.power(ALPHA[j], i) for j in range(NROOTS)] for i in range(NROOTS)], list(S))
    assert d is not None
    return _pattern([N - 1 - j for j in range(NROOTS)], d)


# Random 6- and 7-error patterns (positions, values) kept from a search of 30000 draws because they lie within distance 5 of another
# codeword (about 2e-4 of such draws do): class f must show both outcomes, and a fresh draw of this size would show failures only.
RANDOM_MISCORRECTIONS = (
    ((79, 42, 112, 43, 44, 117), (77, 153, 31, 93, 101, 196)),
    ((28, 27, 35, 86, 69, 103, 67), (253, 48, 105, 229, 178, 99, 164)),
    ((52, 84, 72, 101, 58, 48), (140, 118, 124, 42, 121, 1)),
    ((8, 82, 115, 4, 7, 69), (103, 177, 98, 166, 123, 83)),
    ((22, 42, 81, 12, 59, 8, 75), (122, 162, 155, 209, 106, 2, 205)),
    ((34, 70, 10, 116, 114, 99, 0), (41, 115, 87, 122, 140, 89, 68)),
    ((88, 85, 91, 16, 31, 98, 19), (106, 106, 100, 240, 33, 145, 151)),
)


def rs_cases(seed=20240611):
    """{class: [RsCase]} for the classes a..g."""
    rng = np.random.default_rng(seed)
    out = {c: [] for c in "abcdefg"}
    # a: single errors, every position, values covering 1..255
    for k in range(N):
        for j in range(3):
            v = (3 * k + j) % 255 + 1
            out["a"].append(RsCase("a", "pos %d val %d" % (k, v), _pattern([k], [v]), 1))
    assert {int(c.pattern.max()) for c in out["a"]} == set(range(1, 256))
    # b: pairs at the ends and across the data / parity border
    for pair in ((0, 1), (0, 119), (118, 119), (109, 110)):
        for _ in range(3):
            out["b"].append(RsCase("b", "pair %s" % (pair,), _pattern(pair, rng.integers(1, 256, 2)), 2))
    # c: five errors
    sets = {"parity even": (110, 112, 114, 116, 118), "parity low": (110, 111, 112, 113, 114), "parity high": (115, 116, 117, 118, 119),
            "first five": (0, 1, 2, 3, 4), "last five": (115, 116, 117, 118, 119), "spaced from 0": (0, 29, 58, 87, 116),
            "spaced to 119": (3, 32, 61, 90, 119), "spaced 24": (0, 24, 48, 72, 96), "spaced 24 to 119": (23, 47, 71, 95, 119)}
    for name, pos in sets.items():
        out["c"].append(RsCase("c", name, _pattern(pos, rng.integers(1, 256, 5)), 5))
    for name in ("first five", "spaced from 0", "parity even"):
        out["c"].append(RsCase("c", name + ", equal values", _pattern(sets[name], [int(rng.integers(1, 256))] * 5), 5))
    for _ in range(3):
        out["c"].append(RsCase("c", "random places, equal values", _pattern(rng.choice(N, 5, replace=False), [int(rng.integers(1, 256))] * 5), 5))
    # d: sent + 6 of the 11 non-zero bytes of a weight-11 codeword g: the nearest codeword is sent + g, at distance 5
    for kd in (0, 57, 109):
        for trial in range(4):
            d = np.zeros(K, np.uint8)
            d[kd] = int(rng.integers(1, 256))
            g = np.concatenate([d, ref.encode(d)])
            supp = np.flatnonzero(g)
            assert supp.size == 11 and supp[0] == kd                    # MDS: weight exactly n - k + 1
            par = supp[1:]
            keep = rng.choice(par, 5 if trial % 2 == 0 else 6, replace=False)
            if trial % 2 == 0:
                keep = np.concatenate([[kd], keep])                      # the data byte among the 6 received: 5 parity bytes get "corrected"
            pat = np.zeros(N, np.uint8)
            pat[keep] = g[keep]
            out["d"].append(RsCase("d", "data byte %d %s" % (kd, "kept" if trial % 2 == 0 else "dropped"), pat, 5, delta=g))
    # e: the syndromes of 1..5 errors of the full-length code with at least one in the shortened positions (powers 120..254), realised by the
    # parity bytes alone.  Two error patterns of weight <= 5 and <= 5 cannot share syndromes (d = 11), so no live pattern explains them.
    for v in (1, 2, 3, 4, 5):
        for nout in sorted({1, (v + 1) // 2, v}):
            for p_out in ((120, 254), (121, 200), (180, 253))[: 2 if v > 1 else 3]:
                outside = list(rng.choice(np.arange(p_out[0] + 1, p_out[1]), nout, replace=False))
                if nout >= 1:
                    outside[0] = p_out[0]
                if nout >= 2:
                    outside[1] = p_out[1]
                inside = list(rng.choice(N, v - nout, replace=False))
                S = syndromes_of_virtual(outside + inside, rng.integers(1, 256, v))
                out["e"].append(RsCase("e", "%d virtual errors, powers %s" % (v, sorted(int(p) for p in outside + inside)), parity_pattern(S), -1))
    # f (dagger): beyond the bound
    for ne in (6, 7, 8, 60):
        for _ in range(12 if ne < 60 else 4):
            out["f"].append(RsCase("f", "%d errors" % ne, _pattern(rng.choice(N, ne, replace=False), rng.integers(1, 256, ne)), None, dagger=True))
    for _ in range(8):
        out["f"].append(RsCase("f", "uniformly random word", rng.integers(0, 256, N), None, dagger=True))
    for pos, vals in RANDOM_MISCORRECTIONS:
        out["f"].append(RsCase("f", "%d random errors that land near another codeword" % len(pos), _pattern(pos, vals), None, dagger=True))
    # g (dagger): zero discrepancies in Berlekamp-Massey: S0 = 0 (error values that sum to zero, or any syndromes through the parity bytes),
    # and S0..S4 = 0 with the rest non-zero
    for ne in (2, 3, 4, 5):
        for _ in range(3):
            vals = list(rng.integers(1, 256, ne - 1))
            last = int(np.bitwise_xor.reduce(np.array(vals)))
            if last == 0:
                vals[0] ^= 1
                last = 1
            out["g"].append(RsCase("g", "%d errors whose values sum to zero" % ne, _pattern(rng.choice(N, ne, replace=False), vals + [last]), None,
                                   dagger=True))
    for _ in range(6):
        out["g"].append(RsCase("g", "S0 = 0, others random", parity_pattern([0] + list(rng.integers(1, 256, 9))), None, dagger=True))
    for _ in range(6):
        out["g"].append(RsCase("g", "S0..S4 = 0", parity_pattern([0] * 5 + list(rng.integers(1, 256, 5))), None, dagger=True))
    for _ in range(3):
        out["g"].append(RsCase("g", "S0..S4 = 0, S6 = 0", parity_pattern([0] * 5 + [int(rng.integers(1, 256)), 0] + list(rng.integers(1, 256, 3))), None,
                               dagger=True))
    for c in out["g"]:
        S = ref.syndromes(c.pattern)
        assert S[0] == 0 and any(S)
    return out


# ---- CRCs, by tables made from polynomial division -----------------------------------------------------------------------------------------
def polymul2(a, b):
    """Carry-less product of two GF(2) polynomials held in ints."""
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        b >>= 1
    return r


def polymod2(a, g):
    n = g.bit_length()
    while a.bit_length() >= n:
        a ^= g << (a.bit_length() - n)
    return a


FIRE_GEN = 0x1782F                                    # x^16+x^14+x^13+x^12+x^11+x^5+x^3+x^2+x+1
CRC_GEN = 0x11021                                     # x^16+x^12+x^5+1
_FIRE_TAB = [polymod2(v << 16, FIRE_GEN) for v in range(256)]
_CRC_TAB = [polymod2(v << 16, CRC_GEN) for v in range(256)]


def _crc(tab, data, c):
    for b in bytes(data):
        c = ((c << 8) & 0xFFFF) ^ tab[(c >> 8) ^ b]
    return c


def fire_code(b2_10):
    return _crc(_FIRE_TAB, b2_10, 0)


def au_crc(data):
    return _crc(_CRC_TAB, data, 0xFFFF) ^ 0xFFFF


# ---- superframe classes ------------------------------------------------------------------------------------------------------------------------
def build_sf(rng, s, dac, sbr, starts, fire_good=True, flip=None):
    """An unprotected superframe (110 s bytes) with the given au_start values (starts[0] is the fixed start of AU 0), random AUs with good
    CRCs when the layout is legal, random bytes otherwise.  flip = ("payload" | "crc", AU index): one bit of that AU's payload or stored CRC
    is flipped afterwards.  -> (bytes, the record fields this must parse to)."""
    n, start0 = AU_LAYOUT[(dac, sbr)]
    total = K * s
    assert len(starts) == n and starts[0] == start0 and all(0 <= v < 4096 for v in starts[1:])
    out = bytearray(rng.integers(0, 256, total).astype(np.uint8).tobytes())
    flags = [int(rng.integers(2)) for _ in range(3)] + [int(rng.integers(8))]
    out[2] = (flags[0] << 7) | (dac << 6) | (sbr << 5) | (flags[1] << 4) | (flags[2] << 3) | flags[3]
    bits = 0
    for v in starts[1:]:
        bits = (bits << 12) | int(v)
    nb = 12 * (n - 1)
    nbytes = (nb + 7) // 8
    out[3:3 + nbytes] = (bits << (8 * nbytes - nb)).to_bytes(nbytes, "big")
    assert 3 + nbytes == start0
    bounds = [int(v) for v in starts] + [total]
    legal = all(bounds[i + 1] - bounds[i] >= 3 and bounds[i + 1] <= total for i in range(n))
    crc_ok = 0
    if legal:
        for i in range(n):
            a, e = bounds[i], bounds[i + 1]
            c = au_crc(out[a:e - 2])
            out[e - 2], out[e - 1] = c >> 8, c & 0xFF
            crc_ok |= 1 << i
        if flip is not None:
            kind, i = flip
            a, e = bounds[i], bounds[i + 1]
            at = int(rng.integers(a, e - 2)) if kind == "payload" else int(rng.integers(e - 2, e))
            out[at] ^= 1 << int(rng.integers(8))
            crc_ok &= ~(1 << i)
    else:
        assert flip is None
    f = fire_code(out[2:11])
    if not fire_good:
        f ^= 1 << int(rng.integers(16))
    out[0], out[1] = f >> 8, f & 0xFF
    exp = dict(fire_ok=int(fire_good), layout_ok=int(fire_good and legal), rfa=flags[0], dac_rate=dac, sbr_flag=sbr, aac_channel_mode=flags[1],
               ps_flag=flags[2], mpeg_surround_config=flags[3], num_aus=n, au_start=[0] * 6, au_len=[0] * 6, crc_ok=0)
    if exp["layout_ok"]:
        for i in range(n):
            exp["au_start"][i], exp["au_len"][i] = bounds[i], bounds[i + 1] - bounds[i]
        exp["crc_ok"] = crc_ok
    return np.frombuffer(bytes(out), dtype=np.uint8).copy(), exp


def last_start_limit(s):
    """The largest legal au_start of the last AU: it is a 12-bit field, and the AU needs 3 bytes."""
    return min(4095, K * s - 3)


def random_starts(rng, s, dac, sbr, fixed=None):
    """A legal au_start list; fixed = {AU index: length} pins the lengths of some AUs."""
    n, start0 = AU_LAYOUT[(dac, sbr)]
    fixed = dict(fixed or {})
    total = K * s
    lo = {i: fixed.get(i, 3) for i in range(n - 1)}
    free = [i for i in range(n - 1) if i not in fixed]
    if n - 1 in fixed:
        L = total - fixed[n - 1] - start0
    else:
        top = last_start_limit(s) - start0
        L = int(rng.integers(sum(lo.values()), top + 1)) if free else sum(lo.values())
    extra = L - sum(lo.values())
    assert extra >= 0 and (free or extra == 0) and start0 + L <= 4095, "no such layout"
    cuts = np.sort(rng.integers(0, extra + 1, max(len(free) - 1, 0)))
    share = np.diff(np.concatenate([[0], cuts, [extra]])) if free else []
    for i, x in zip(free, share):
        lo[i] += int(x)
    starts = [start0]
    for i in range(n - 1):
        starts.append(starts[-1] + lo[i])
    return starts


def slice_len(s):
    """Bytes per lane of the AU kernel's split CRC."""
    return (K * s + 63) // 64


def superframe_cases(rng, s, dac, sbr):
    """{class: [(label, unprotected bytes, expected fields)]} for one (s, dac_rate, sbr_flag)."""
    n, start0 = AU_LAYOUT[(dac, sbr)]
    total = K * s
    out = {}

    def add(cls, label, starts, **kw):
        out.setdefault(cls, []).append((label,) + build_sf(rng, s, dac, sbr, starts, **kw))

    # an AU of exactly 3 bytes in the first, a middle and the last place.  The last AU starts at 110 s - 3, which the 12-bit field holds up to
    # s = 37 only; above that the shortest last AU the format allows (au_start = 4095) stands in.
    add("au3", "first", random_starts(rng, s, dac, sbr, {0: 3}))
    if n > 2:
        add("au3", "middle", random_starts(rng, s, dac, sbr, {n // 2: 3}))
    else:
        add("au3", "first again", random_starts(rng, s, dac, sbr, {0: 3}))
    if total - 3 <= 4095:
        add("au3", "last", random_starts(rng, s, dac, sbr, {n - 1: 3}))
        add("au3", "all but one", random_starts(rng, s, dac, sbr, {i: 3 for i in range(1, n)}))
    else:
        add("au3", "last AU as short as the field allows", random_starts(rng, s, dac, sbr, {n - 1: total - 4095}))
    # au_start on a slice border of the split CRC, and next to it (d = 2 puts the CRC's end on the border)
    sl = slice_len(s)
    first = -(-(start0 + 3 + 1) // sl)                                   # first multiple with room for d = -1
    last = (last_start_limit(s) - 2) // sl
    step = max(1, -(-3 // sl))                                           # multiples far enough apart for 3-byte AUs
    for d in (-1, 0, 1, 2):
        for trial in range(2):
            idx = np.sort(rng.choice(np.arange(first, last + 1, step), n - 1, replace=False))
            add("slice", "d %+d: %s" % (d, list(idx * sl + d)), [start0] + [int(v) * sl + d for v in idx])
    if n > 2:
        k0 = int(rng.integers(first, last - (n - 1) * step))
        add("slice", "consecutive slices", [start0] + [(k0 + i * step) * sl for i in range(n - 1)])
    # one flipped bit in one AU's payload / stored CRC, for each AU
    for i in range(n):
        add("flip", "payload of AU %d" % i, random_starts(rng, s, dac, sbr), flip=("payload", i))
        add("flip", "crc of AU %d" % i, random_starts(rng, s, dac, sbr), flip=("crc", i))
    # a good fire code over an illegal layout
    good = random_starts(rng, s, dac, sbr)
    if n > 2:
        add("layout", "decreasing", [start0] + sorted(good[1:], reverse=True))
        add("layout", "two equal", good[:2] + [good[1]] + good[3:])
        i = int(rng.integers(1, n - 1))
        st = random_starts(rng, s, dac, sbr, {i: 3})
        add("layout", "gap of 2 at AU %d" % i, st[:i + 1] + [v - 1 for v in st[i + 1:]])
    else:
        add("layout", "decreasing (below AU 0)", [start0, start0 - 1])
        add("layout", "two equal (AU 0's start)", [start0, start0])
        add("layout", "gap of 2 after AU 0", [start0, start0 + 2])
    if total - 2 <= 4095:
        st = random_starts(rng, s, dac, sbr, {n - 1: 3})
        add("layout", "last au_start = 110 s - 2", st[:-1] + [st[-1] + 1])
    if total < 4095 + 3:
        add("layout", "au_start = 4095", good[:-1] + [4095])
    for lab, data, exp in out["layout"]:
        assert exp["fire_ok"] == 1 and exp["layout_ok"] == 0, lab
    # a bad fire code over an otherwise perfect superframe
    add("fire", "bad fire code", random_starts(rng, s, dac, sbr), fire_good=False)
    for cls in ("au3", "slice", "flip"):
        for lab, data, exp in out[cls]:
            assert exp["layout_ok"] == 1, (cls, lab)
    return out


def plain_superframes(rng, s, nsf):
    """nsf legal unprotected superframes with random layouts."""
    out = []
    for _ in range(nsf):
        dac, sbr = LAYOUTS[int(rng.integers(4))]
        out.append(build_sf(rng, s, dac, sbr, random_starts(rng, s, dac, sbr))[0])
    return out


# ---- ETI frames ---------------------------------------------------------------------------------------------------------------------------------
def raw_frame(fct, entries, ficf=1, fill=0x55):
    """An ETI(NI) frame whose STC is entries = [(SubChId, STL, payload bytes or None)] exactly as given: any STL, ids repeated, payloads that run
    past the frame (cut at byte 6144)."""
    f = bytearray([fill]) * ETI_BYTES
    f[0:4] = bytes([0xFF, 0xF8, 0xC5, 0x49]) if fct & 1 else bytes([0xFF, 0x07, 0x3A, 0xB6])
    f[4] = fct % 250
    nst = len(entries)
    assert nst < 128
    f[5] = (ficf << 7) | nst
    pos = 12 + 4 * nst + 96 * ficf
    for i, (scid, stl, pay) in enumerate(entries):
        f[8 + 4 * i] = (scid << 2) & 0xFF
        f[8 + 4 * i + 1] = 0
        f[8 + 4 * i + 2] = (stl >> 8) & 3
        f[8 + 4 * i + 3] = stl & 0xFF
        if pay is not None and pos < ETI_BYTES:
            pay = bytes(pay)[:ETI_BYTES - pos]
            f[pos:pos + len(pay)] = pay
        pos += 8 * stl
    return np.frombuffer(bytes(f), dtype=np.uint8).copy()


def piece(sf, f):
    """The 24 s bytes of a protected superframe that ride in its frame f (0..4)."""
    s = len(sf) // N
    return sf[24 * s * (f % 5):24 * s * (f % 5 + 1)]


FRAME_IDS = (5, 9)


def frame_cases(seed=77):
    """[(label, frames, {SubChId: superframes that must come out}, {SubChId: sync losses})] for FRAME_IDS; a fifth element, where present, is
    the protected superframes that id 5 must deliver.  Rule for an id that is listed twice in one frame's STC: the first entry counts."""
    rng = np.random.default_rng(seed)
    out = []

    def sfs(s, nsf=3):
        return protect_many(plain_superframes(rng, s, nsf))

    def rand(stl):
        return rng.integers(0, 256, 8 * stl).astype(np.uint8).tobytes()

    for stl in (0, 1, 2, 3, 4, 216, 219, 1023):
        legal = stl in (3, 216)
        a, b = (sfs(stl // 3) if legal else None), sfs(2)
        frames = [raw_frame(40 + f, [(5, stl, piece(a[f // 5], f) if legal else rand(stl)), (9, 6, piece(b[f // 5], f))]) for f in range(15)]
        out.append(("STL %d, id 9 behind it" % stl, frames, {5: 3 if legal else 0, 9: 0 if stl == 1023 else 3}, {5: 0, 9: 0}))
    for over, lab in ((0, "ends exactly at byte 6144"), (1, "ends 8 bytes past the frame")):
        a = sfs(72)
        frames = [raw_frame(245 + f, [(20, 300, None), (21, 237 + over, None), (5, 216, piece(a[f // 5], f))]) for f in range(15)]
        assert 12 + 4 * 3 + 96 + 8 * (300 + 237 + over + 216) == ETI_BYTES + 8 * over
        out.append(("payload " + lab, frames, {5: 0 if over else 3, 9: 0}, {5: 0, 9: 0}))
    a, b = sfs(2), sfs(1)
    out.append(("FICF = 0", [raw_frame(f, [(5, 6, piece(a[f // 5], f)), (9, 3, piece(b[f // 5], f))], ficf=0) for f in range(15)], {5: 3, 9: 3},
                {5: 0, 9: 0}))
    out.append(("NST = 0", [raw_frame(f, []) for f in range(10)], {5: 0, 9: 0}, {5: 0, 9: 0}))
    a, b = sfs(2, 4), sfs(1, 4)
    frames = [raw_frame(f, [(5, 6, piece(a[f // 5], f)), (9, 3, piece(b[f // 5], f))]) for f in range(10)] + [raw_frame(10, [])]
    frames += [raw_frame(11 + f, [(5, 6, piece(a[2 + f // 5], f)), (9, 3, piece(b[2 + f // 5], f))]) for f in range(10)]
    out.append(("a frame with NST = 0 between superframes", frames, {5: 4, 9: 4}, {5: 1, 9: 1}))
    a, b = sfs(2), sfs(1)
    others = [i for i in range(64) if i not in FRAME_IDS]
    frames = [raw_frame(100 + f, [(5, 6, piece(a[f // 5], f))] + [(i, 3, rand(3)) for i in others] + [(9, 3, piece(b[f // 5], f))]) for f in range(15)]
    out.append(("NST = 64, wanted ids first and last", frames, {5: 3, 9: 3}, {5: 0, 9: 0}))
    a, b = sfs(2), sfs(1)
    frames = [raw_frame(f, [(6 if f == 7 else 5, 6, piece(a[f // 5], f)), (9, 3, piece(b[f // 5], f))]) for f in range(15)]
    out.append(("id absent in one frame of a superframe", frames, {5: 2, 9: 3}, {5: 1, 9: 0}))
    a, b, c = sfs(2), sfs(1), sfs(4)
    out.append(("id twice, both legal: the first counts", [raw_frame(f, [(5, 6, piece(a[f // 5], f)), (5, 3, piece(b[f // 5], f))]) for f in range(15)],
                {5: 3, 9: 0}, {5: 0, 9: 0}, a))
    out.append(("id twice, the first not DAB+", [raw_frame(f, [(5, 4, rand(4)), (5, 3, piece(b[f // 5], f))]) for f in range(15)], {5: 0, 9: 0},
                {5: 0, 9: 0}))
    out.append(("id twice around another id", [raw_frame(f, [(5, 3, piece(b[f // 5], f)), (9, 12, piece(c[f // 5], f)), (5, 6, piece(a[f // 5], f))])
                                               for f in range(15)], {5: 3, 9: 3}, {5: 0, 9: 0}, b))
    return out


# ---- carrying cases through the stage ------------------------------------------------------------------------------------------------------------
def frames_of(fct0, subs, phase=0, count=None):
    """subs = [(SubChId, [protected superframes])], all lists equally long -> the ETI frames carrying them side by side, from frame `phase` on."""
    nf = 5 * len(subs[0][1])
    stop = nf if count is None else min(nf, phase + count)
    return [raw_frame((fct0 + f) % 250, [(scid, len(x[f // 5]) // 40, piece(x[f // 5], f)) for scid, x in subs]) for f in range(phase, stop)]


def rs_lane(cases, seed=5, s=72):
    """The RS cases as codewords 11..s-1 of superframes of rate s (codewords 0..10 hold superframe bytes 0..10, the raw fire code, and stay
    clean, so sync never drops a superframe).  One class per superframe.
    -> [(class, case count, received superframe, expected data bytes, symbols corrected, codewords failed)]"""
    rng = np.random.default_rng(seed)
    per = s - 11
    out = []
    for cls in sorted(cases):
        for at in range(0, len(cases[cls]), per):
            chunk = cases[cls][at:at + per]
            sf = protect_many(plain_superframes(rng, s, 1))[0].reshape(N, s).copy()
            want = sf[:K].copy()
            fixed = failed = 0
            for i, case in enumerate(chunk):
                j = 11 + i
                rx, word, n = case.apply(sf[:, j].copy())
                sf[:, j] = rx
                want[:, j] = word[:K]
                if n < 0:
                    failed += 1
                else:
                    fixed += n
            out.append((cls, len(chunk), sf.reshape(-1), want.reshape(-1), fixed, failed))
    return out


def decode_superframes(raws):
    """[120 s received bytes] -> [(110 s bytes after correction, symbols corrected, codewords failed)]: syndromes of all codewords at once,
    rs_reference.decode on those with errors."""
    if not raws:
        return []
    words = np.concatenate([np.asarray(r, np.uint8).reshape(N, -1).T for r in raws])
    dirty = np.flatnonzero(syndromes_many(words).any(axis=1))
    res = {int(w): ref.decode(words[w]) for w in dirty}
    out, at = [], 0
    for r in raws:
        s = len(r) // N
        grid = np.asarray(r, np.uint8).reshape(N, s).copy()
        fixed = failed = 0
        for j in range(s):
            if at + j in res:
                word, n = res[at + j]
                if n < 0:
                    failed += 1
                else:
                    fixed += n
                    grid[:, j] = word
        out.append((grid[:K].reshape(-1), fixed, failed))
        at += s
    return out
