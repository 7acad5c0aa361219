"""Builders for the ensemble directory's tests: FIGs, FIBs with a valid or a broken CRC, ETI frames by hand with any NST (so the FIC offset moves),
and the directory of a dabtools_amd.Dir as the plain tuples of tests/dir_model.py.  Written from include/dabhip.h."""
import numpy as np

import dir_model as M

ETI_BYTES = 6144


# ---- FIGs ------------------------------------------------------------------------------------------------------------------------------------
def fig(ftype, data, length=None):
    """header byte + data field; `length` overrides the length field (to lie about it)"""
    data = bytes(data)
    return bytes([(ftype << 5) | (len(data) if length is None else length)]) + data


def fig0(ext, body=b"", cn=0, oe=0, pd=0, length=None):
    return fig(0, bytes([cn << 7 | oe << 6 | pd << 5 | ext]) + bytes(body), length)


def e00(eid, change=0, al=0, cif_hi=0, cif_lo=0, extra=b""):
    return bytes([eid >> 8, eid & 255, change << 6 | al << 5 | cif_hi, cif_lo]) + bytes(extra)


def e01_short(subch, start, index, switch=0):
    return bytes([subch << 2 | start >> 8, start & 255, switch << 6 | index])


def e01_long(subch, start, option, level, size):
    return bytes([subch << 2 | start >> 8, start & 255, 0x80 | option << 4 | level << 2 | size >> 8, size & 255])


def comp(tmid, a=0, b=0, ps=1, ca=0):
    """TMId 0 / 1: a = ASCTy / DSCTy, b = SubChId; TMId 3: a = SCId; TMId 2: a = the raw 14 bits"""
    if tmid in (0, 1):
        return bytes([tmid << 6 | a, b << 2 | ps << 1 | ca])
    if tmid == 3:
        return bytes([0xC0 | a >> 6, (a & 63) << 2 | ps << 1 | ca])
    return bytes([0x80 | (a >> 8) & 63, a & 255])


def e02(sid, comps, pd=0, local=0, caid=0, ncomp=None):
    n = len(comps) if ncomp is None else ncomp
    return sid.to_bytes(4 if pd else 2, "big") + bytes([local << 7 | caid << 4 | n]) + b"".join(comps)


def e03(scid, subch, address, dscty=60, dg=1, scca=None, rfa=0, rfu=0):
    out = bytes([scid >> 4, (scid & 15) << 4 | rfa << 1 | (scca is not None), dg << 7 | rfu << 6 | dscty, subch << 2 | address >> 8, address & 255])
    return out + (scca.to_bytes(2, "big") if scca is not None else b"")


def e09(lto, ecc, table, extra=b""):
    return bytes([lto, ecc, table]) + bytes(extra)


def e10(mjd, hours, minutes, seconds=None, ms=0, lsi=0, rfu=0, rfa=0):
    utc = seconds is not None
    word = rfu << 31 | mjd << 14 | lsi << 13 | rfa << 12 | utc << 11 | hours << 6 | minutes
    return word.to_bytes(4, "big") + (bytes([seconds << 2 | ms >> 8, ms & 255]) if utc else b"")


def e14(subch, scheme):
    return bytes([subch << 2 | scheme])


def label(ext, key, text, flags=0xFF00, charset=0, oe=0, length=None):
    """FIG 1/ext: key is the EId (0), the 16-bit SId (1) or the 32-bit SId (5)"""
    text = (text if isinstance(text, bytes) else text.encode("latin-1")).ljust(16)[:16]
    return fig(1, bytes([charset << 4 | oe << 3 | ext]) + key.to_bytes(4 if ext == 5 else 2, "big") + text + flags.to_bytes(2, "big"), length)


# ---- FIBs and frames ---------------------------------------------------------------------------------------------------------------------------
def fib(*figs, crc=True, pad=0xFF, raw=None):
    """the FIGs back to back, padded with `pad` to 30 bytes (or raw: exactly 30 bytes), and the CRC -- valid, or with one bit turned"""
    body = bytes(raw) if raw is not None else b"".join(figs)
    assert len(body) <= 30, len(body)
    body = body + bytes([pad]) * (30 - len(body))
    c = ~M.crc16(body) & 0xFFFF
    if not crc:
        c ^= 0x0100
    return body + bytes([c >> 8, c & 255])


EMPTY_FIB = fib()


def frame(fibs=(), nst=1, ficf=1, mid=1, fill=0x55, seed=None):
    """one ETI frame: only the bytes the directory reads are meaningful (bytes 5, 6 and the FIC at 12 + 4 NST); the rest is `fill` or seeded noise"""
    if seed is None:
        fr = np.full(ETI_BYTES, fill, dtype=np.uint8)
    else:
        fr = np.random.default_rng(seed).integers(0, 256, ETI_BYTES, dtype=np.uint8)
    fr[5] = ficf << 7 | nst
    fr[6] = (int(fr[6]) & ~0x18) | mid << 3
    fibs = list(fibs) + [EMPTY_FIB] * (3 - len(fibs))
    off = 12 + 4 * nst
    if off + 96 <= ETI_BYTES and ficf:
        fr[off:off + 96] = np.frombuffer(b"".join(fibs), dtype=np.uint8)
    return fr


def frames(list_of_fib_lists, **kw):
    if not list_of_fib_lists:
        return np.zeros((0, ETI_BYTES), dtype=np.uint8)
    return np.stack([frame(f, **kw) for f in list_of_fib_lists])


def hostile_fib(rng):
    """30 arbitrary bytes, biased towards FIG headers that parse, under a valid CRC"""
    raw = bytearray(rng.integers(0, 256, 30, dtype=np.uint8).tobytes())
    if rng.random() < 0.8:
        i = 0
        while i < 30:
            length = int(rng.integers(1, 30))
            ftype = int(rng.choice([0, 0, 0, 0, 1, 1, 2, 7]))
            if ftype == 1 and rng.random() < 0.7:
                length = int(rng.choice([20, 21, 21, 21, 22, 23, 23, 23]))
            raw[i] = ftype << 5 | min(length, 31)
            if i + 1 < 30:
                if ftype == 0:
                    raw[i + 1] = int(rng.choice([0, 1, 2, 3, 9, 10, 14, 5])) | (int(rng.integers(0, 8)) << 5 if rng.random() < 0.15 else int(rng.integers(0, 2)) << 5)
                elif ftype == 1:
                    raw[i + 1] = int(rng.choice([0, 1, 5, 4])) | int(rng.integers(0, 16)) << 4 if rng.random() < 0.9 else raw[i + 1]
            i += 1 + length
            if rng.random() < 0.2:
                break
    return fib(raw=bytes(raw))


# ---- a dabtools_amd.Dir's tables as the model's tuples ---------------------------------------------------------------------------------------
def _p01(r):
    return (int(r["form"]), int(r["uep_index"]), int(r["protlev"]), int(r["start_cu"]), int(r["size_cu"]), int(r["bitrate"]))


def _lbl(r):
    return (int(r["charset"]), bytes(r["label"]), int(r["char_flags"]))


def _meta(r):
    return (int(r["first_frame"]), int(r["last_frame"]), int(r["changes"]))


def gpu_tuples(d, stream):
    """(ensemble, sub-channels, services, packet components) of one stream of a Dir, shaped like the model's *_tuples()"""
    e = d.ensemble(stream)
    h = int(e["have"])
    ens = None
    if h:
        ens = ((int(e["eid"]), int(e["change_flag"]), int(e["al"]), int(e["cif_hi"]), int(e["cif_lo"])) if h & 1 else None,
               (int(e["lto"]), int(e["ecc"]), int(e["inter_table"])) if h & 2 else None,
               (int(e["mjd"]), int(e["lsi"]), int(e["utc_flag"]), int(e["hours"]), int(e["minutes"]), int(e["seconds"]), int(e["milliseconds"])) if h & 4 else None,
               ((int(e["label_eid"]),) + _lbl(e)) if h & 8 else None, int(e["time_frame"])) + _meta(e)
    sub = [(int(r["id"]), _p01(r) if r["have"] & 1 else None, (int(r["fec_scheme"]),) if r["have"] & 2 else None) + _meta(r) for r in d.subchannels(stream)]
    svc = [((int(r["pd"]), int(r["sid"])), (int(r["info"]), tuple(int(x) for x in r["comp"][:2 * int(r["ncomp"])])) if r["have"] & 1 else None,
            _lbl(r) if r["have"] & 2 else None) + _meta(r) for r in d.services(stream)]
    pkt = [(int(r["scid"]), (int(r["scca_flag"]), int(r["dg"]), int(r["dscty"]), int(r["subch"]), int(r["address"]), int(r["scca"]))) + _meta(r)
           for r in d.packet_components(stream)]
    return ens, sub, svc, pkt


def model_tuples(m):
    return m.ensemble_tuple(), m.subch_tuples(), m.service_tuples(), m.pkt_tuples()


# ---- hand-written vectors: one per rule of dabhip.h and per walk edge; the expected facts and (figs, truncated, ignored) are written out here by
# hand, not computed.  name -> (FIB, facts, (figs, truncated, ignored)) -------------------------------------------------------------------------
_L16 = b"ABCDEFGHIJKLMNOP"
_C3 = [comp(0, 63, 5), comp(1, 24, 6, ps=0), comp(3, 0x123, ps=0, ca=1)]
_C3_RAW = (0x3F, 0x16, 0x58, 0x18, 0xC4, 0x8D)
VECTORS = {
    "0xff_at_byte_0": (fib(), [], (0, 0, 0)),
    "header_at_byte_29": (fib(fig(7, bytes(28)), b"\x01"), [], (2, 1, 1)),
    "length_0": (fib(b"\x00", fig0(14, e14(1, 1))), [], (1, 1, 0)),
    "ends_exactly_at_29_28_facts": (fib(fig0(14, bytes(k << 2 | (k & 3) for k in range(28)))), [("0/14", k, (k & 3,)) for k in range(28)], (1, 0, 0)),
    "one_past_29": (fib(fig0(14, bytes(28), length=30)), [], (1, 1, 0)),
    "past_29_after_a_good_fig": (fib(fig0(14, e14(9, 2)), fig0(14, bytes(25), length=28)), [("0/14", 9, (2,))], (2, 1, 0)),
    "0/0": (fib(fig0(0, e00(0xCE15, change=2, al=1, cif_hi=19, cif_lo=249))), [("0/0", None, (0xCE15, 2, 1, 19, 249))], (1, 0, 0)),
    "0/0_occurrence_change_skipped": (fib(fig0(0, e00(0x1001, cif_lo=3, extra=b"\x77"))), [("0/0", None, (0x1001, 0, 0, 0, 3))], (1, 0, 0)),
    "0/0_cn_is_not_looked_at": (fib(fig0(0, e00(0x1001), cn=1)), [("0/0", None, (0x1001, 0, 0, 0, 0))], (1, 0, 0)),
    "0/0_one_short": (fib(fig0(0, e00(0x1001)[:3])), [], (1, 1, 0)),
    "0/1_short_and_long": (fib(fig0(1, e01_short(3, 700, 35, switch=1) + e01_long(40, 54, 1, 2, 27 * 4))),
                           [("0/1", 3, (0, 35, 3, 700, 96, 128)), ("0/1", 40, (1, 0, 6, 54, 108, 192))], (1, 0, 0)),
    "0/1_long_a": (fib(fig0(1, e01_long(63, 1023, 0, 3, 4 * 17))), [("0/1", 63, (1, 0, 3, 1023, 68, 136))], (1, 0, 0)),
    "0/1_short_one_short": (fib(fig0(1, e01_short(1, 0, 0) + e01_short(2, 16, 1)[:2])), [("0/1", 1, (0, 0, 5, 0, 16, 32))], (1, 1, 0)),
    "0/1_long_one_short": (fib(fig0(1, e01_short(1, 0, 63) + e01_long(2, 16, 0, 0, 12)[:3])), [("0/1", 1, (0, 63, 1, 0, 416, 384))], (1, 1, 0)),
    "0/1_empty_body": (fib(fig0(1)), [], (1, 0, 0)),
    "0/2_sid16": (fib(fig0(2, e02(0x1234, _C3, local=1, caid=5) + e02(0x1235, [comp(2, 0x2BCD)]))),
                  [("0/2", (0, 0x1234), (0xD3, _C3_RAW)), ("0/2", (0, 0x1235), (0x01, (0xAB, 0xCD)))], (1, 0, 0)),
    "0/2_sid32": (fib(fig0(2, e02(0xE0001234, [comp(3, 0xFFF)], pd=1), pd=1)), [("0/2", (1, 0xE0001234), (0x01, (0xFF, 0xFE)))], (1, 0, 0)),
    "0/2_sid16_one_short": (fib(fig0(2, e02(0x1234, [comp(0, 0, 1)]) + e02(0x1235, _C3)[:-1])), [("0/2", (0, 0x1234), (0x01, (0x00, 0x06)))], (1, 1, 0)),
    "0/2_sid32_one_short": (fib(fig0(2, e02(0xE0001234, [], pd=1)[:4], pd=1)), [], (1, 1, 0)),
    "0/2_no_components": (fib(fig0(2, e02(0x4321, []))), [("0/2", (0, 0x4321), (0x00, ()))], (1, 0, 0)),
    "0/2_12_components_the_most_a_fib_holds": (fib(fig0(2, e02(0x0001, [comp(0, 0, k) for k in range(12)]))),
                                               [("0/2", (0, 1), (0x0C, tuple(x for k in range(12) for x in (0, k << 2 | 2))))], (1, 0, 0)),
    "0/2_15_components_cannot_fit": (fib(fig0(2, e02(0x0001, [comp(0, 0, k) for k in range(12)], ncomp=15))), [], (1, 1, 0)),
    "0/3_without_scca": (fib(fig0(3, e03(0x123, 7, 1000, dscty=60, dg=1, rfa=7, rfu=1))), [("0/3", 0x123, (0, 1, 60, 7, 1000, 0))], (1, 0, 0)),
    "0/3_with_scca": (fib(fig0(3, e03(0xFFF, 63, 1, dscty=5, dg=0, scca=0xBEEF) + e03(0, 0, 0))),
                      [("0/3", 0xFFF, (1, 0, 5, 63, 1, 0xBEEF)), ("0/3", 0, (0, 1, 60, 0, 0, 0))], (1, 0, 0)),
    "0/3_without_scca_one_short": (fib(fig0(3, e03(1, 2, 3)[:4])), [], (1, 1, 0)),
    "0/3_with_scca_one_short": (fib(fig0(3, e03(1, 2, 3) + e03(2, 2, 4, scca=1)[:6])), [("0/3", 1, (0, 1, 60, 2, 3, 0))], (1, 1, 0)),
    "0/9": (fib(fig0(9, e09(0xA2, 0xE1, 0x01, extra=b"\x12\x34"))), [("0/9", None, (0xA2, 0xE1, 0x01))], (1, 0, 0)),
    "0/9_one_short": (fib(fig0(9, e09(1, 2, 3)[:2])), [], (1, 1, 0)),
    "0/10_short": (fib(fig0(10, e10(60000, 23, 59, lsi=1, rfu=1, rfa=1))), [("0/10", None, (60000, 1, 0, 23, 59, 0, 0))], (1, 0, 0)),
    "0/10_utc": (fib(fig0(10, e10(0x1FFFF, 1, 2, seconds=59, ms=999))), [("0/10", None, (0x1FFFF, 0, 1, 1, 2, 59, 999))], (1, 0, 0)),
    "0/10_one_short": (fib(fig0(10, e10(60000, 1, 1)[:3])), [], (1, 1, 0)),
    "0/10_utc_one_short": (fib(fig0(10, e10(60000, 1, 1, seconds=1)[:5])), [], (1, 1, 0)),
    "0/14": (fib(fig0(14, e14(63, 1) + e14(0, 0) + e14(7, 3))), [("0/14", 63, (1,)), ("0/14", 0, (0,)), ("0/14", 7, (3,))], (1, 0, 0)),
    "oe_on_every_handled": (fib(*[fig0(x, b"\x00", oe=1) for x in (0, 1, 2, 3, 9, 10, 14)]), [], (7, 0, 7)),
    "oe_label": (fib(label(0, 1, "x", oe=1)), [], (1, 0, 1)),
    "cn_on_the_lists": (fib(*[fig0(x, e14(1, 1), cn=1) for x in (1, 2, 3, 14)], fig0(9, e09(1, 2, 3), cn=1)), [("0/9", None, (1, 2, 3))], (5, 0, 4)),
    "unhandled_type_0": (fib(*[fig0(x, b"\x01") for x in (4, 5, 6, 7, 8, 11, 12, 13, 15, 31)]), [], (10, 0, 10)),
    "unhandled_types": (fib(*[fig(t, b"\x00") for t in (2, 3, 4, 5, 6, 7)], *[fig(1, bytes([x]) + b"\x00") for x in (2, 3, 4, 6, 7)]), [], (11, 0, 11)),
    "label_ensemble": (fib(label(0, 0xCE15, _L16, flags=0xF0F0, charset=6)), [("ens-label", None, (0xCE15, 6, _L16, 0xF0F0))], (1, 0, 0)),
    "label_sid16": (fib(label(1, 0xD220, b"\x00\x7f\x80\xff" + _L16[4:], flags=1, charset=15)),
                    [("svc-label", (0, 0xD220), (15, b"\x00\x7f\x80\xff" + _L16[4:], 1))], (1, 0, 0)),
    "label_sid32": (fib(label(5, 0xE0D22001, _L16)), [("svc-label", (1, 0xE0D22001), (0, _L16, 0xFF00))], (1, 0, 0)),
    "label_sid16_length_20": (fib(fig(1, label(1, 1, _L16)[1:21]), fig0(14, e14(2, 1))),
                              [("0/14", 2, (1,))], (2, 1, 0)),
    "label_sid16_length_22": (fib(fig(1, label(1, 1, _L16)[1:] + b"\x00")), [], (1, 1, 0)),
    "label_sid32_length_22": (fib(fig(1, label(5, 1, _L16)[1:23])), [], (1, 1, 0)),
    "label_sid32_length_21": (fib(fig(1, label(5, 1, _L16)[1:22])), [], (1, 1, 0)),
    "label_sid16_length_23": (fib(fig(1, label(1, 1, _L16)[1:] + b"\x00\x00")), [], (1, 1, 0)),
}
