"""tools/models/multilane_soft_model.py -- the soft decoder with two and four lanes per code word in plain Python (the index algebra of
vit_soft_lanes.hpp: 4-step blocks in three variants, compaction numbering, metric words indexed by the lane's code offset, half-records,
chain-back) -- held bit for bit against oracle/or_soft.c: FIC blocks through or_fic_decode_soft, one short and one long MSC code word through
SoftDab (or_dab in soft mode, the ETI frame's bytes); values full-range (-7 .. 7), tie-heavy (-1 .. 1) and all-zero.  And against the model's own
plain one-lane decoder on values that include -8, with the registers checked after every step."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import dabtools_amd as dab
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    spec = importlib.util.spec_from_file_location("multilane_soft_model", os.path.join(ROOT, "tools", "models", "multilane_soft_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


model = _load()


def _values(rng, kind, n):
    if kind == "full":
        return rng.integers(-7, 8, n).astype(np.int8)
    if kind == "ties":
        return rng.integers(-1, 2, n).astype(np.int8)
    return np.zeros(n, np.int8)


def _descrambled(data):
    out = np.frombuffer(data, np.uint8).copy()
    ol.oracle().or_descramble(ol._ptr(out), out.size)
    return out


def _depunctured(keep, received):
    dep = np.zeros(keep.size, np.int64)
    dep[keep] = received
    return [int(x) for x in dep]


@pytest.mark.parametrize("kind", ["full", "ties", "zero"])
def test_fic_blocks_equal_the_oracle(kind):
    O = ol.oracle()
    dep = np.zeros(3096, np.uint8)
    O.or_fic_depuncture(ol._ptr(dep), ol._ptr(np.zeros(2304, np.uint8)))
    keep = dep != 128
    rng = np.random.default_rng({"full": 61, "ties": 62, "zero": 63}[kind])
    fic = _values(rng, kind, 9216)
    want_fib = np.zeros((12, 32), np.uint8)
    want_ok = np.zeros(12, np.uint8)
    O.or_fic_decode_soft(ol._ptr(fic.astype(np.float32), C.c_float), ol.SOFT_Q4, ol._ptr(want_fib), ol._ptr(want_ok))
    for NL, blocks in ((2, (0, 1, 2, 3)), (1, (1, 3))):
        for q in blocks:
            got = _descrambled(model.decode(_depunctured(keep, fic[2304 * q:2304 * (q + 1)]), 774, NL))
            assert np.array_equal(got, want_fib[3 * q:3 * q + 3].ravel()), (kind, NL, q)


# one short and one long code word: EEP 3-A at 8 kbit/s (6 CU, 198 steps) and EEP 1-A at 128 kbit/s (192 CU, 3,078 steps)
SUBCHANNELS = ((2, 6, 8, 0), (0, 192, 128, 6))          # (protection level index, size in CU, kbit/s, start CU)


def _msc_keep(protlev, size, bitrate):
    dep = np.zeros(4 * (24 * bitrate + 6) + 64, np.uint8)
    n = ol.oracle().or_msc_depuncture(ol._ptr(dep), ol._ptr(np.zeros(64 * size, np.uint8)), C.byref(ol.SubCh(id=1, slform=1, protlev=protlev, size=size, bitrate=bitrate)))
    assert n == 4 * (24 * bitrate + 6)
    return dep[:n] != 128


@pytest.mark.parametrize("kind", ["full", "ties", "zero"])
def test_msc_code_words_equal_the_oracle(kind):
    from test_gpu_soft import _fic_values, _keep_mask
    cfg = dab.synth_preset(1, seed=811, cif_count0=400)
    cfg.nsub = len(SUBCHANNELS)
    for k, (protlev, size, bitrate, start) in enumerate(SUBCHANNELS):
        cfg.sub[k].id = 5 + 7 * k
        cfg.sub[k].start_cu = start
        cfg.sub[k].slform = 1
        cfg.sub[k].uep_index = 0
        cfg.sub[k].eep_protlev = protlev
        cfg.sub[k].size_cu = size
    rng = np.random.default_rng({"full": 71, "ties": 72, "zero": 73}[kind])
    cif = _values(rng, kind, 55296)                        # every CIF carries the same values: time de-interleaving returns them unchanged
    keep_fic = _keep_mask()
    od = ol.SoftDab(ol.SOFT_Q4)
    for t in range(16):
        od.process(_fic_values(cfg, t, keep_fic), np.tile(cif, 4))
    assert len(od.frames) > 0
    frame = od.frames[-1]
    od.close()
    nst = int(frame[5]) & 0x7f
    assert nst == len(SUBCHANNELS)
    pos = 8 + 4 * nst + 4 + 96                             # SYNC, FC, NST x STC, EOH, FIC of one CIF
    seen = 0
    for s in range(nst):
        stc = frame[8 + 4 * s:12 + 4 * s]
        sad, stl = ((int(stc[0]) & 3) << 8) | int(stc[1]), ((int(stc[2]) & 3) << 8) | int(stc[3])
        protlev, size, bitrate, start = next(x for x in SUBCHANNELS if x[3] == sad)
        assert stl * 8 == 3 * bitrate
        want = frame[pos:pos + 3 * bitrate]
        pos += 8 * stl
        keep = _msc_keep(protlev, size, bitrate)
        values = _depunctured(keep, cif[64 * start:64 * start + int(keep.sum())])
        nsteps = 24 * bitrate + 6
        for NL in (2, 1) if nsteps < 1000 or kind == "full" else (2,):
            got = _descrambled(model.decode(values, nsteps, NL))
            assert np.array_equal(got, want), (kind, NL, sad)
        seen += 1
    assert seen == len(SUBCHANNELS)


@pytest.mark.parametrize("NL", [1, 2])
def test_equals_the_one_lane_model_on_values_with_minus_eight(NL):
    """-8 among the values (the table counts it as -7; no sign is ever flipped, so it needs no special case), every count of received values per
    step, lengths with every admitted remainder, registers against the plain metrics after every step"""
    for nsteps, seed in ((774, 5), (70, 6), (64, 7), (68, 8), (69, 9), (39, 10)):
        assert model.run(NL, nsteps, seed, -8, 7)
    assert model.run(NL, 198, 11, -8, -6)                  # mostly -8 and -7: the same metric
