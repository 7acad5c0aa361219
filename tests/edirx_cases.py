"""Shapes for the EDI receiving tests (test_edirx_model.py on the CPU, test_gpu_edirx.py on the GPU): packets made by the sending model
(edi_model.pack of the hand-built frames of edi_cases.py), AF packets built by hand with foreign items, fragmenting of any AF packet, drop
patterns that give a named number of erasures, and damaged packets."""
import numpy as np

import edi_cases as ecs
import edi_model as em
import edirx_model as rx

MODES = [(0, 0, 1400), (1, 0, 255), (2, 2, 1400)]      # all three modes


def packets_of(frames, mode, recover=0, max_frag=1400, seq0=0):
    """-> [[packets of frame 0], [packets of frame 1], ..] of the accepted frames, by the sending model"""
    data, recs = em.pack(frames, mode, recover, max_frag, seq0)
    data = data.tobytes()
    out, last = [], None
    for off, n, number, seq, findex, fcount in recs:
        if number != last:
            out.append([])
            last = number
        out[-1].append(data[off:off + n])
    return out


def flat(groups):
    return [p for g in groups for p in g]


def accepted(frames):
    return [f for f in frames if em.accepted(f) is not None]


def expected_frames(frames):
    """what the receiver must give for the frames a sender accepted: the rebuild of the carried fields"""
    return [rx.rebuild(em.carried(f)) for f in accepted(frames)]


def _be(v, n):
    return int(v).to_bytes(n, "big")


def _item(name, value):
    return name + _be(8 * len(value), 4) + value


def make_af(frame, seq, fcth=0, between=(), atst=None, rfud=None, ptr=True, pad_to=8):
    """The AF packet of a frame with whatever a foreign sender may add: items between deti and est, an 8-byte time stamp, 3 RFUD bytes"""
    d = em.carried(frame)
    a = ((atst is not None) << 15) | (d["ficf"] << 14) | ((rfud is not None) << 13) | (fcth << 8) | d["fct"]
    deti = _be(a, 2) + _be((d["err"] << 24) | (d["mid"] << 22) | (d["fp"] << 19) | d["mnsc"], 4) + (atst or b"") + bytes(d["fic"]) + (rfud or b"")
    tag = (_item(b"*ptr", b"DETI" + bytes(4)) if ptr else b"") + _item(b"deti", deti)
    for name, value in between:
        tag += _item(name, value)
    for i, ((scid, sad, tpl, stl), sub) in enumerate(zip(d["stc"], d["sub"])):
        tag += _item(b"est" + bytes([i + 1]), _be((scid << 18) | (sad << 8) | (tpl << 2), 3) + bytes(sub))
    tag += bytes(-len(tag) % pad_to)
    body = b"AF" + _be(len(tag), 4) + _be(seq, 2) + b"\x90T" + tag
    return body + _be(em.crc16(body), 2)


def fragment(af, seq, mode, recover=0, max_frag=1400):
    """any AF packet -> its PFT fragments by the sender's size rule"""
    l = len(af)
    c, k, z, B, f, s = em.plan(l, mode, recover, max_frag)
    if mode == 0:
        return [af]
    if mode == 1:
        return [em.pf_header(seq, i, f, 0, len(af[i * s:(i + 1) * s])) + af[i * s:(i + 1) * s] for i in range(f)]
    data = np.frombuffer(af + bytes(z), np.uint8).reshape(c, k)
    block = np.concatenate([data, em.rs_parity(data)], axis=1).reshape(-1)
    grid = np.concatenate([block, np.zeros(f * s - B, np.uint8)]).reshape(s, f)
    return [em.pf_header(seq, i, f, 1, s, k, z) + grid[:, i].tobytes() for i in range(f)]


def erasure_counts(l, recover, max_frag, dropped):
    """the erasures of every code word when the fragments `dropped` of a packet of l bytes are lost"""
    c, k, z, B, f, s = em.plan(l, 2, recover, max_frag)
    held = set(range(f)) - set(dropped)
    return [len(rx.word_erasures(held, f, k, w)) for w in range(c)]


def drop(group, dropped):
    return [p for i, p in enumerate(group) if i not in set(dropped)]


def with_byte_flipped(p, at, bit=0x10):
    b = bytearray(p)
    b[at] ^= bit
    return bytes(b)


def rehead(p, **fields):
    """a PF packet with header fields replaced and the HCRC made right again"""
    h = rx.check_packet(p)
    fec = h["kind"] == "FEC"
    v = dict(pseq=h["q"], findex=h["findex"], fcount=h["fcount"], plen=h["plen"], rsk=h["rsk"], rsz=h["rsz"])
    v.update(fields)
    return em.pf_header(v["pseq"], v["findex"], v["fcount"], fec, v["plen"], v["rsk"], v["rsz"]) + h["payload"]


def small_stream(n, seed, first_fct=0):
    rng = np.random.default_rng(seed)
    return [ecs.frame(rng, (first_fct + i) % 250, [int(v) for v in rng.integers(0, 9, i % 3)], ficf=i % 2) for i in range(n)]


def cut(items, sizes):
    out, at = [], 0
    for n in sizes:
        out.append(items[at:at + n])
        at += n
    return out
