"""Shapes for the EDI tests (test_edi_model.py on the CPU, test_gpu_edi.py on the GPU): hand-built ETI frames at the borders of the rules of
dabhip.h (dabhip_edi), FCT sequences for the FCTH and SEQ rule, and the grid of the size rule.

An AF packet of this stage has l = 12 + (a multiple of 8) bytes, so l = 4 (mod 8): l = 207 c exists for c = 4 (mod 8) only, and 207 c + 1 never.
The frames below therefore take, for c = 1, 2 and the largest c a frame can give (32), the l nearest to each border on both sides (204 | 212,
412 | 420, 6412 | 6420) and the exact multiples 828 = 207 * 4 and 5796 = 207 * 28; every l, these included, goes through the size rule itself on
the CPU (test_edi_model.py, tests/host_sanitize/edi_units.cpp)."""
import numpy as np

import edi_model as m

GRID_L = range(13, 7001)
GRID_RECOVER = range(6)
GRID_FRAG = (64, 65, 255, 1400, 1472)


def frame(rng, fct=0, stls=(), ficf=1, mid=1, err=0xFF, fp=None, nst=None):
    """An ETI(NI) frame with random STC fields (but the STLs given), MNSC, FIC and sub-channel bytes; nst overrides the NST field alone."""
    f = np.full(m.ETI_BYTES, 0x55, np.uint8)
    n = len(stls)
    f[0] = err
    f[1:4] = (0x07, 0x3A, 0xB6) if fct % 2 == 0 else (0xF8, 0xC5, 0x49)
    f[4] = fct
    f[5] = (ficf << 7) | (n if nst is None else nst)
    f[6] = ((fct % 8 if fp is None else fp) << 5) | (mid << 3) | int(rng.integers(0, 8))
    f[7] = int(rng.integers(0, 256))
    for i, stl in enumerate(stls):
        scid, sad, tpl = int(rng.integers(0, 64)), int(rng.integers(0, 864)), int(rng.integers(0, 64))
        f[8 + 4 * i:12 + 4 * i] = list(((scid << 26) | (sad << 16) | (tpl << 10) | stl).to_bytes(4, "big"))
    used = n if nst is None else nst
    end = min(m.ETI_BYTES, 12 + 4 * used + 96 * ficf + 8 * sum(stls))
    f[8 + 4 * used:end] = rng.integers(0, 256, end - 8 - 4 * used, dtype=np.uint8)
    return f


def frame_of_l(rng, l, fct=0):
    """An accepted frame whose AF packet has l bytes (l = 4 mod 8, l = 44 or 60 <= l <= 6620)"""
    for ficf, nst in ((0, 2), (0, 1), (1, 5), (0, 64), (0, 0)):
        l0 = 12 + -(-(30 + 96 * ficf + 11 * nst) // 8) * 8
        total, rest = divmod(l - l0, 8)
        if rest or total < 0 or 12 + 4 * nst + 96 * ficf + 8 * total > m.MST_END or (nst == 0 and total):
            continue
        stls = [0] * nst
        for i in range(nst):
            stls[i] = min(1023, total - sum(stls)) if i == nst - 1 else int(rng.integers(0, min(1023, total - sum(stls)) + 1))
        if sum(stls) != total:
            stls = [total // nst + (i < total % nst) for i in range(nst)]
        f = frame(rng, fct, stls, ficf)
        assert len(m.af_body(f, 0, 0)) + 2 == l
        return f
    raise ValueError(l)


BORDER_L = (204, 212, 412, 420, 828, 5796, 6412, 6420, 6620)


def border_frames(seed=1):
    """One stream with every border of the frame and TAG rules: NST 0, 1, 2, 64; an entry with STL 0; FICF 0; TAG padding of each of 0..7 bytes
    (NST 0..7); the l of BORDER_L; a main stream ending exactly at byte 6140; and each of the three skip reasons between accepted frames."""
    rng = np.random.default_rng(seed)
    fct = iter(range(10 ** 6))
    nxt = lambda: next(fct) % 250
    frames = [frame(rng, nxt(), [3] * nst) for nst in range(8)]                       # pads 2, 7, 4, 1, 6, 3, 0, 5
    assert sorted((30 + 96 + 11 * nst + 24 * nst) % 8 for nst in range(8)) == list(range(8))   # the unpadded TAG packets' sizes mod 8
    frames.append(frame(rng, nxt(), [5, 0, 7]))                                       # STL 0 between two others
    frames.append(frame(rng, nxt(), [0]))
    frames.append(frame(rng, nxt(), [4, 9], ficf=0, mid=2))                           # FICF 0: any MID
    frames.append(frame(rng, nxt(), [9] * 64))
    frames.append(frame(rng, nxt(), [2] * 65))                                        # skipped: NST 65
    frames.append(frame(rng, nxt(), [1] * 64, ficf=0))
    frames.append(frame(rng, nxt(), [6], mid=2))                                      # skipped: FICF 1 and MID 2
    frames.append(frame(rng, nxt(), [500, 265], ficf=0))                              # 12 + 8 + 8 * 765 = 6140 exactly
    assert m.accepted(frames[-1]) is not None
    frames.append(frame(rng, nxt(), [500, 266], ficf=0))                              # skipped: past 6140 by 8
    frames.append(frame(rng, nxt(), [1023], ficf=1))                                  # skipped: far past the frame
    for l in BORDER_L:
        frames.append(frame_of_l(rng, l, nxt()))
    assert sum(m.accepted(f) is None for f in frames) == 4
    return frames


def size_borders(recover, max_frag):
    """l (4 mod 8) with z = 0 and c > 1, z = c - 1 > 0, f s = B and f s > B under the size rule of mode 2, one each"""
    want = {}
    for l in range(60, m.MAX_L + 1, 8):
        c, k, z, B, f, s = m.plan(l, 2, recover, max_frag)
        for key, hit in (("z0", z == 0 and c > 1), ("zmax", z == c - 1 and c > 2), ("exact", f * s == B and f > 1), ("padded", f * s > B)):
            if hit and key not in want:
                want[key] = l
    assert len(want) == 4, (recover, max_frag, want)
    return want


def small_frame(rng, fct, skipped=False):
    """A frame of NST 1 (56 bytes of AF packet), or one that is skipped"""
    return frame(rng, fct, [2], ficf=0) if not skipped else frame(rng, fct, [2], ficf=1, mid=3)


# FCT sequences (None: a skipped frame, whose own FCT is 249): wraps, repeats, a skipped frame at a wrap, nothing but skipped frames first
FCT_SEQUENCES = {
    "plain": [0, 1, 2, 3, 4, 5],
    "wrap": [247, 248, 249, 0, 1, 2, 249, 0],
    "repeats": [5, 5, 5, 4, 4, 6, 6, 0],
    "skipped at a wrap": [248, 249, None, 1, 2, None, None, 0],
    "skipped first": [None, None, 7, 3, None, 2],
    "every frame wraps": [9, 8, 7, 6, 5, 4, 3],
}


def fct_frames(seq, seed=3):
    rng = np.random.default_rng(seed)
    return [small_frame(rng, 249, True) if v is None else small_frame(rng, v) for v in seq]


def cuttings(n):
    """every way to cut n frames into consecutive pushes of at least one frame, as lists of push sizes"""
    for mask in range(1 << max(n - 1, 0)):
        sizes, run = [], 1
        for i in range(n - 1):
            if mask >> i & 1:
                sizes.append(run)
                run = 1
            else:
                run += 1
        yield sizes + [run] if n else []
