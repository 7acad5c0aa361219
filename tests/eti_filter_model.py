"""What the sub-channel filter must produce, written from the ETI(NI) frame layout (misc.c:153-314) as eti_check.py is: a filtered
frame is the unfiltered frame with the STC reduced to the listed SubChIds, NST / FL / HCRC / EOF CRC following from that, and the FIC and the kept
payloads byte-identical (include/dabhip.h).  The unfiltered frames are the reference's (the oracle's replay), so the expected value of every filtered
frame is this host-side rewrite of one of them.  Nothing of the product is used.  Test infrastructure."""
import numpy as np

from eti_check import crc16_ccitt

ETI_BYTES = 6144

# eti_check.crc16_ccitt byte by byte instead of bit by bit (a frame's MST is some thousand bytes, a test filters some hundred frames)
_CRC_TABLE = [crc16_ccitt([b], 0) for b in range(256)]


def crc16(data, crc=0xFFFF):
    for b in bytes(data):
        crc = ((crc << 8) & 0xFFFF) ^ _CRC_TABLE[(crc >> 8) ^ b]
    return crc


def keep_set(ids):
    """The SubChIds a list of ids keeps: None = all.  An empty list as given means all; ids outside 0..63 and duplicates are dropped, and a list left
    empty only by that keeps nothing."""
    if ids is None:
        return None
    ids = list(ids)
    if not ids:
        return None
    return {int(i) for i in ids if 0 <= int(i) < 64}


def split(frame):
    """-> (fc bytes 4..7, [(4 STC bytes, payload bytes)], fic bytes): the parts a rewrite moves about."""
    e = np.asarray(frame, dtype=np.uint8)
    assert e.shape == (ETI_BYTES,) and e[0] == 0xFF
    nst = int(e[5]) & 0x7F
    stc = [e[8 + 4 * k:12 + 4 * k] for k in range(nst)]
    pos = 8 + 4 * nst + 4                                   # SYNC + FC, STC, EOH
    fic = e[pos:pos + 96]
    pos += 96
    subs = []
    for s in stc:
        stl = ((int(s[2]) & 3) << 8) | int(s[3])
        subs.append((s, e[pos:pos + 8 * stl]))
        pos += 8 * stl
    return e[4:8], subs, fic


def filter_frame(frame, keep):
    """One 6144-byte frame -> the frame that carries only the SubChIds in `keep` (a set; None = all)."""
    fc, subs, fic = split(frame)
    if keep is not None:
        subs = [(s, p) for s, p in subs if (int(s[0]) >> 2) in keep]
    nst = len(subs)
    fl = nst + 1 + 24 + sum(p.size // 4 for _, p in subs)   # words of 4 bytes: STC + EOH + FIC + sum of 2 STL
    out = np.full(ETI_BYTES, 0x55, dtype=np.uint8)
    out[0:4] = np.asarray(frame, dtype=np.uint8)[0:4]       # ERR, FSYNC
    out[4] = fc[0]                                          # FCT
    out[5] = 0x80 | nst                                     # FICF, NST
    out[6] = (int(fc[2]) & 0xF8) | (fl >> 8)                # FP and MID as they were, FL
    out[7] = fl & 0xFF
    pos = 8
    for s, _ in subs:
        out[pos:pos + 4] = s
        pos += 4
    out[pos:pos + 2] = 0xFF                                 # MNSC
    hcrc = (~crc16(out[4:pos + 2])) & 0xFFFF
    out[pos + 2], out[pos + 3] = hcrc >> 8, hcrc & 0xFF
    pos += 4
    mst0 = pos
    out[pos:pos + 96] = fic
    pos += 96
    for _, p in subs:
        out[pos:pos + p.size] = p
        pos += p.size
    eof = (~crc16(out[mst0:pos])) & 0xFFFF
    out[pos], out[pos + 1] = eof >> 8, eof & 0xFF
    out[pos + 2:pos + 8] = 0xFF                             # RFU, TIST
    return out


def filter_frames(frames, ids):
    """frames (n x 6144) -> the n frames the sub-channel filter `ids` must produce."""
    frames = np.asarray(frames, dtype=np.uint8).reshape(-1, ETI_BYTES)
    keep = keep_set(ids)
    out = np.zeros_like(frames)
    for i, f in enumerate(frames):
        out[i] = filter_frame(f, keep)
    return out


def with_fic(frame, fic):
    """The frame with other FIC bytes (96) and the EOF CRC that follows from them."""
    out = np.array(frame, dtype=np.uint8)
    _, subs, _ = split(out)
    mst0 = 8 + 4 * len(subs) + 4
    end = mst0 + 96 + sum(p.size for _, p in subs)
    out[mst0:mst0 + 96] = fic
    eof = (~crc16(out[mst0:end])) & 0xFFFF
    out[end], out[end + 1] = eof >> 8, eof & 0xFF
    return out
