"""The ensemble directory's rules (include/dabhip.h, "ensemble directory") restated in plain Python: the model that the kernels, the rule header
(dir_figs.hpp through tests/host_sanitize/dir_units.cpp) and the modulator's si_mode are held to.  Written from that text, not from the kernel."""
import numpy as np

ETI_BYTES = 6144
COUNTERS = ("frames", "frames_without_fic", "frames_skipped", "fibs", "fibs_crc_failed", "figs", "figs_truncated", "figs_ignored", "facts", "facts_changed",
            "overflow_dropped")
KINDS = ("UNKNOWN", "MP2", "DABPLUS", "TS", "STREAM_DATA", "PACKET")
NO_SERVICE, NO_COMPONENT, NO_PKTCOMP, NO_SUBCH = -2, -3, -4, -5

# ETSI table 7: (bit rate, size in CU, protection level) per UEP index
_UEP_RATES = ((32, (16, 21, 24, 29, 35)), (48, (24, 29, 35, 42, 52)), (56, (29, 35, 42, 52)), (64, (32, 42, 48, 58, 70)), (80, (40, 52, 58, 70, 84)),
              (96, (48, 58, 70, 84, 104)), (112, (58, 70, 84, 104)), (128, (64, 84, 96, 116, 140)), (160, (80, 104, 116, 140, 168)),
              (192, (96, 116, 140, 168, 208)), (224, (116, 140, 168, 208, 232)), (256, (128, 168, 192, 232, 280)))
UEP = [(rate, size, 5 - k) for rate, sizes in _UEP_RATES for k, size in enumerate(sizes)]
UEP += [(320, 160, 5), (320, 208, 4), (320, 280, 2), (384, 192, 5), (384, 280, 3), (384, 416, 1)]
assert len(UEP) == 64
EEP_MULTIPLE = (12, 8, 6, 4, 27, 21, 18, 15)


def crc16(data):
    crc = 0xFFFF
    for byte in data:
        crc ^= int(byte) << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def fib_crc_ok(fib):
    want = ~crc16(fib[:30]) & 0xFFFF
    return int(fib[30]) == want >> 8 and int(fib[31]) == want & 0xFF


def walk_fib(fib):
    """The FIG walk of one FIB whose CRC holds.  Returns (facts, figs, truncated, ignored); a fact is (kind, key, fields) with kind one of
    '0/0', '0/1', '0/2', '0/3', '0/9', '0/10', '0/14', 'ens-label', 'svc-label', key None, a SubChId, (pd, SId) or an SCId, and fields a tuple."""
    d30 = [int(x) for x in fib[:30]]
    facts, figs, trunc, ign = [], 0, 0, 0
    i = 0
    while i < 30 and d30[i] != 0xFF:
        ftype, length = d30[i] >> 5, d30[i] & 31
        figs += 1
        if length == 0 or i + 1 + length > 30:
            trunc += 1
            break
        data = d30[i + 1:i + 1 + length]
        i += 1 + length
        body = data[1:]
        if ftype == 0:
            cn, oe, pd, ext = data[0] >> 7, (data[0] >> 6) & 1, (data[0] >> 5) & 1, data[0] & 31
            if oe or (cn and ext in (1, 2, 3, 14)) or ext not in (0, 1, 2, 3, 9, 10, 14):
                ign += 1
            elif ext == 0:
                if len(body) < 4:
                    trunc += 1
                else:
                    facts.append(("0/0", None, (body[0] << 8 | body[1], body[2] >> 6, (body[2] >> 5) & 1, body[2] & 31, body[3])))
            elif ext == 9:
                if len(body) < 3:
                    trunc += 1
                else:
                    facts.append(("0/9", None, tuple(body[:3])))
            elif ext == 10:
                word = (body[0] << 24 | body[1] << 16 | body[2] << 8 | body[3]) if len(body) >= 4 else 0
                utc = (word >> 11) & 1
                if len(body) < 4 or (utc and len(body) < 6):
                    trunc += 1
                else:
                    sec, ms = (body[4] >> 2, (body[4] & 3) << 8 | body[5]) if utc else (0, 0)
                    facts.append(("0/10", None, ((word >> 14) & 0x1FFFF, (word >> 13) & 1, utc, (word >> 6) & 31, word & 63, sec, ms)))
            elif ext == 14:
                facts += [("0/14", b >> 2, (b & 3,)) for b in body]
            else:
                j = 0
                while j < len(body):
                    rest = body[j:]
                    if ext == 1:
                        if len(rest) < 3 or len(rest) < (4 if rest[2] >> 7 else 3):
                            trunc += 1
                            break
                        start = (rest[0] & 3) << 8 | rest[1]
                        if rest[2] >> 7:
                            protlev = ((rest[2] >> 2) & 3) | ((rest[2] >> 4) & 7) << 2
                            size = (rest[2] & 3) << 8 | rest[3]
                            fields = (1, 0, protlev, start, size, size // EEP_MULTIPLE[protlev & 7] * (32 if protlev & 4 else 8))
                            j += 4
                        else:
                            rate, size, level = UEP[rest[2] & 63]
                            fields = (0, rest[2] & 63, level, start, size, rate)
                            j += 3
                        facts.append(("0/1", rest[0] >> 2, fields))
                    elif ext == 2:
                        sl = 4 if pd else 2
                        if len(rest) < sl + 1 or len(rest) < sl + 1 + 2 * (rest[sl] & 15):
                            trunc += 1
                            break
                        nc = rest[sl] & 15
                        facts.append(("0/2", (pd, int.from_bytes(bytes(rest[:sl]), "big")), (rest[sl], tuple(rest[sl + 1:sl + 1 + 2 * nc]))))
                        j += sl + 1 + 2 * nc
                    else:
                        if len(rest) < 2 or len(rest) < (7 if rest[1] & 1 else 5):
                            trunc += 1
                            break
                        flag = rest[1] & 1
                        facts.append(("0/3", rest[0] << 4 | rest[1] >> 4,
                                      (flag, rest[2] >> 7, rest[2] & 63, rest[3] >> 2, (rest[3] & 3) << 8 | rest[4], (rest[5] << 8 | rest[6]) if flag else 0)))
                        j += 7 if flag else 5
        elif ftype == 1:
            charset, oe, ext = data[0] >> 4, (data[0] >> 3) & 1, data[0] & 7
            if oe or ext not in (0, 1, 5):
                ign += 1
            elif length != (23 if ext == 5 else 21):
                trunc += 1
            else:
                kl = 4 if ext == 5 else 2
                key = int.from_bytes(bytes(body[:kl]), "big")
                label = (charset, bytes(body[kl:kl + 16]), body[kl + 16] << 8 | body[kl + 17])
                facts.append(("ens-label", None, (key,) + label) if ext == 0 else ("svc-label", (1 if ext == 5 else 0, key), label))
        else:
            ign += 1
    return facts, figs, trunc, ign


class Entry:
    def __init__(self, key, frame):
        self.key, self.parts, self.first, self.last, self.changes = key, {}, frame, frame, 0


class Stream:
    """The directory of one stream: push(frames) any number of times; the tables are dicts / lists of Entry."""

    def __init__(self):
        self.c = dict.fromkeys(COUNTERS, 0)
        self.reset()

    def reset(self):
        self.ens, self.sub, self.svc, self.pkt = None, {}, [], []

    def counters(self):
        return [self.c[k] for k in COUNTERS]

    def _apply(self, frame, kind, key, fields):
        self.c["facts"] += 1
        if kind in ("0/0", "0/9", "0/10", "ens-label"):
            if self.ens is None:
                self.ens = Entry(None, frame)
            e = self.ens
        elif kind in ("0/1", "0/14"):
            e = self.sub.setdefault(key, Entry(key, frame))
        else:
            table = self.pkt if kind == "0/3" else self.svc
            e = next((x for x in table if x.key == key), None)
            if e is None:
                if len(table) == 64:
                    self.c["overflow_dropped"] += 1
                    return
                e = Entry(key, frame)
                table.append(e)
        part = "label" if kind in ("ens-label", "svc-label") else kind
        if part in e.parts and e.parts[part] != fields:
            e.changes += 1
            self.c["facts_changed"] += 1
        e.parts[part] = fields
        e.last = frame
        if part == "0/10":
            e.time_frame = frame

    def push(self, frames):
        """Returns the FIBs of this push whose CRC held."""
        frames = np.asarray(frames, dtype=np.uint8).reshape(-1, ETI_BYTES)
        good = 0
        for fr in frames:
            number = self.c["frames"]
            self.c["frames"] += 1
            nst, ficf, mid = int(fr[5]) & 0x7F, int(fr[5]) >> 7, (int(fr[6]) >> 3) & 3
            if not ficf:
                self.c["frames_without_fic"] += 1
                continue
            if mid != 1 or nst > 64:
                self.c["frames_skipped"] += 1
                continue
            for q in range(3):
                fib = fr[12 + 4 * nst + 32 * q:][:32]
                self.c["fibs"] += 1
                if not fib_crc_ok(fib):
                    self.c["fibs_crc_failed"] += 1
                    continue
                good += 1
                facts, figs, trunc, ign = walk_fib(fib)
                self.c["figs"] += figs
                self.c["figs_truncated"] += trunc
                self.c["figs_ignored"] += ign
                for kind, key, fields in facts:
                    self._apply(number, kind, key, fields)
        return good

    # ---- complete and resolve ------------------------------------------------------------------------------------------------------------
    def _has_subch(self, sid):
        return sid in self.sub and "0/1" in self.sub[sid].parts

    def resolve_component(self, svc, component):
        """A dict like Dir.resolve's, or one of the NO_* codes."""
        if "0/2" not in svc.parts or not 0 <= component < len(svc.parts["0/2"][1]) // 2:
            return NO_COMPONENT
        c0, c1 = svc.parts["0/2"][1][2 * component:2 * component + 2]
        tmid = c0 >> 6
        t = {"kind": "UNKNOWN", "subch": -1, "address": 0, "dg": 0, "dscty": 0, "fec": False, "scid": -1, "primary": (c1 >> 1) & 1}
        if tmid == 2:
            return t
        if tmid == 3:
            scid = (c0 & 63) << 6 | c1 >> 2
            p = next((x for x in self.pkt if x.key == scid), None)
            if p is None:
                return NO_PKTCOMP
            _, dg, dscty, subch, address, _ = p.parts["0/3"]
            if not self._has_subch(subch):
                return NO_SUBCH
            t.update(kind="PACKET", subch=subch, address=address, dg=dg, dscty=dscty, scid=scid, fec=self.sub[subch].parts.get("0/14") == (1,))
            return t
        ty, subch = c0 & 63, c1 >> 2
        if not self._has_subch(subch):
            return NO_SUBCH
        t["subch"] = subch
        if tmid == 0:
            t["kind"] = {0: "MP2", 63: "DABPLUS"}.get(ty, "UNKNOWN")
        else:
            t["kind"] = "TS" if ty == 24 else "STREAM_DATA"
        return t

    def resolve(self, pd, sid, component):
        svc = next((x for x in self.svc if x.key == (pd, sid)), None)
        return NO_SERVICE if svc is None else self.resolve_component(svc, component)

    def complete(self):
        if self.ens is None or "0/0" not in self.ens.parts or "label" not in self.ens.parts or not self.svc:
            return False
        for s in self.svc:
            if "0/2" not in s.parts or "label" not in s.parts:
                return False
            if any(isinstance(self.resolve_component(s, c), int) for c in range(len(s.parts["0/2"][1]) // 2)):
                return False
        return True

    # ---- the tables as plain tuples, field for field what dabhip.h's records hold (what the GPU tests compare) --------------------------------
    def ensemble_tuple(self):
        e = self.ens
        if e is None:
            return None
        p = e.parts
        return (p.get("0/0"), p.get("0/9"), p.get("0/10"), p.get("label"), getattr(e, "time_frame", -1), e.first, e.last, e.changes)

    def subch_tuples(self):
        return [(k, e.parts.get("0/1"), e.parts.get("0/14"), e.first, e.last, e.changes) for k, e in sorted(self.sub.items())]

    def service_tuples(self):
        return [(e.key, e.parts.get("0/2"), e.parts.get("label"), e.first, e.last, e.changes) for e in self.svc]

    def pkt_tuples(self):
        return [(e.key, e.parts.get("0/3"), e.first, e.last, e.changes) for e in self.pkt]
