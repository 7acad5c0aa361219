"""Transmitter identification without a GPU (include/dabhip.h, "TII"; csrc/tii_detect.hpp): the pattern table and the carrier lists against the
model (tests/tii_model.py), the model's fixed-point transform against numpy's fp64 transform and against closed forms, the header's range claim on
full-scale inputs in Python integers, the library's detect rule against the model's, the modulator's TII null symbols, and aligned captures through
the model's fold and rule.  The host rule under sanitizers: a stand-alone program, tests/host_sanitize/tii_units.cpp."""
import functools
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import tii_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = tm.S
TF = tm.TF_SAMPLES


def test_pattern_table():
    assert len(tm.PATTERNS) == 70 and tm.PATTERNS[0] == 0x0f and tm.PATTERNS[69] == 0xf0
    assert tm.PATTERNS == sorted(tm.PATTERNS) and all(bin(w).count("1") == 4 for w in tm.PATTERNS)


def test_carriers_against_the_model_and_the_tiling():
    for p in range(70):
        for c in range(24):
            k = dab.tii_carriers(p, c)
            assert k.tolist() == tm.carriers(p, c), (p, c)
    # over c, b, the quarters and the two carriers: the 1536 carriers exactly once (patterns 0x0f and 0xf0 together hold every b)
    seen = sorted(k for c in range(24) for p in (0, 69) for k in tm.carriers(p, c))
    assert seen == [k for k in range(-768, 769) if k]
    slot = tm.slot_of_bin()
    assert (slot >= 0).sum() == 1536 and all((slot == v).sum() == 8 for v in range(192))
    for p, c, text in ((-1, 0, "main_id"), (70, 0, "main_id"), (0, -1, "sub_id"), (0, 24, "sub_id")):
        with pytest.raises(dab.DabhipError, match=text):
            dab.tii_carriers(p, c)
    k = np.zeros(32, np.int16)
    assert dab.lib().dabhip_tii_carriers(0, 0, k.ctypes.data_as(dab.C.POINTER(dab.C.c_int16)), 31) < 0
    assert dab.lib().dabhip_tii_carriers(0, 0, None, 32) < 0


def test_transform_against_numpys():
    """X against numpy.fft.fft(y) / 2048 in fp64 on 32 windows of random bytes ((b - 127) 128 per rail) and 32 of random int8 values, per rail and
    bin, in LSB of X.  Measured: the largest deviation is 3.82 LSB, the rms 0.73, the mean +0.50 ((a + t + 1) >> 1 rounds halves up: bin 0, where
    that bias of all eleven stages adds up, averages +2.7); the figures are those of the roundings alone and do not move with the input's level.
    Asserted, with the margin test_scan_model.py gives the 4096-point transform: every deviation below 5 LSB -- the measurement plus 1.2 LSB, two
    standard deviations (0.54) of the rounding noise about its mean -- and the rms below 1 LSB."""
    rng = np.random.default_rng(14)
    for x in ((rng.integers(0, 256, (32, S, 2)) - 127) * 128, rng.integers(-128, 128, (32, S, 2))):
        X = tm.transform(x)
        ref = np.fft.fft(x[..., 0] + 1j * x[..., 1], axis=1) / S
        dev = np.stack([X[..., 0] - ref.real, X[..., 1] - ref.imag])
        print("largest deviation %.3f LSB, rms %.3f, mean %+.3f, bin 0 mean %+.3f" % (np.abs(dev).max(), np.sqrt((dev ** 2).mean()), dev.mean(), dev[:, :, 0].mean()))
        assert np.abs(dev).max() < 5.0 and np.sqrt((dev ** 2).mean()) < 1.0


def test_transform_closed_forms():
    """Where rounding leaves the result exact: impulses at the quarter positions, DC, and tones at the quarter points."""
    k = np.arange(S)
    quarter = {0: (1, 0), 1: (0, -1), 2: (-1, 0), 3: (0, 1)}                      # (-j)^m as (re, im)
    for m, n0 in enumerate((0, 512, 1024, 1536)):
        x = np.zeros((1, S, 2), np.int64)
        x[0, n0] = (2048 * 5, -2048 * 3)
        X = tm.transform(x)[0]
        rot = np.array([quarter[(m * kk) % 4] for kk in k])                        # e^(-2 pi j k n0 / 2048) = (-j)^(m k)
        want = np.stack([5 * rot[:, 0] + 3 * rot[:, 1], 5 * rot[:, 1] - 3 * rot[:, 0]], axis=1)
        assert np.array_equal(X, want), n0
    for value in ((16384, 16384), (-16256, 12345), (1, -1), (0, 0)):
        X = tm.transform(np.tile(np.array(value, np.int64), (1, S, 1)))[0]
        assert tuple(X[0]) == value and not X[1:].any()
    for m, k0 in enumerate((0, 512, 1024, 1536)):                                  # x[n] = A j^(m n): all of it in bin k0
        rot = np.array([quarter[(-m * n) % 4] for n in k])
        A = (-16256, 777)
        x = np.stack([A[0] * rot[:, 0] - A[1] * rot[:, 1], A[0] * rot[:, 1] + A[1] * rot[:, 0]], axis=1)[None]
        X = tm.transform(x)[0]
        assert tuple(X[k0]) == A and not np.delete(X, k0, axis=0).any(), k0


def test_derotation_against_the_closed_form():
    """y = x e^(-j theta): a tone at an exact quarter step comes to rest; step 0 leaves the samples as they are."""
    rng = np.random.default_rng(3)
    w = rng.integers(0, 256, (2, S, 2))
    x = (w - 127) * 128
    assert np.array_equal(tm.derotate(w, [0, 0]), x)
    y = tm.derotate(w, [1 << 30, 1 << 31])                                         # a quarter and a half turn per sample
    n = np.arange(S)
    assert np.array_equal(y[1], x[1] * ((-1) ** n)[:, None])
    assert np.array_equal(y[0][n % 4 == 1], np.stack([x[0][n % 4 == 1][:, 1], -x[0][n % 4 == 1][:, 0]], axis=1))      # x (-j)
    assert tm.step_of(0, 0.0) == 0 and tm.step_of(1, 0.0) == round(1000 * 2 ** 32 / 2048000) and tm.step_of(-1, -200.0, 0) == (1 << 32) - round(1200 * 2 ** 32 / 2048000)
    assert tm.counted(1, 304, 0.0) and tm.counted(1, -304, -499.9) and not tm.counted(1, 305, 0.0) and not tm.counted(0, 0, 0.0)
    assert not tm.counted(1, 0, float("nan")) and not tm.counted(1, 0, float("inf"))


def test_range_claim_on_full_scale_inputs():
    """The header's step 5 in Python integers: no rail beyond 23,210 after the de-rotation or any stage, no product sum with its 8192 at or beyond
    2^29 -- on windows of all-0 and all-255 bytes and of bytes that alternate and rotate at full scale, de-rotated by steps that
    gather the energy in one bin."""
    n = np.arange(S)
    wins, steps = [], []
    for a in (0, 255):
        for b in (0, 255):
            for step in (0, 1, 0x12345678, 1 << 31, (1 << 32) - 1, 1 << 29):
                wins.append(np.tile(np.array([a, b]), (S, 1)))
                steps.append(step)
            wins.append(np.stack([np.where(n % 2, a, 255 - a), np.where(n % 2, b, 255 - b)], axis=1))
            steps.append(0)
    for k0 in (1, 511, 512, 769, 1537):                                                             # square waves in quadrature: full scale on both rails, turning
        ph = 2 * np.pi * (k0 * n / S + 1 / 8)
        wins.append(np.stack([np.where(np.cos(ph) >= 0, 255, 0), np.where(np.sin(ph) >= 0, 255, 0)], axis=1))
        steps.append(0)
    y = tm.derotate(np.array(wins), steps, wide=True)
    assert int(np.abs(y).max()) <= 23175
    watch = []
    X = tm.transform(y, watch, wide=True)
    assert all(type(v) is int for v in X.reshape(-1)[:8])
    print("largest rail per stage:", [w[0] for w in watch], "largest product sum:", max(w[1] for w in watch))
    assert max(w[0] for w in watch) <= 23210
    assert max(w[1] for w in watch) < 1 << 29
    assert np.array_equal(X.astype(np.int64), tm.transform(tm.derotate(np.array(wins), steps)))     # and int64 is as good as Python integers
    assert tuple(X[0, 0]) == (-16256, -16256)                                                       # the full-scale constant arrives whole
    T = tm.fold(X.astype(np.int64))
    assert int(T.max()) < 1 << 33


def same(a, b):
    assert a == b, (a, b)
    return a


def both(T):
    return same(dab.tii_detect(T), tm.detect(T))


def test_detect_zeros_ties_and_equal_values():
    assert both(np.zeros(192, np.uint64)) == []
    assert both(np.full(192, 2 ** 64 - 1, np.uint64)) == []
    T = np.zeros((24, 8), np.uint64)
    T[4, :4], T[4, 4:] = 10, 5                       # s == 2 n and v3 == 2 v4
    assert both(T) == []
    T[4, 3] = 11                                     # s > 2 n, v3 (now one of the 10s) == 2 v4
    assert both(T) == []
    T[4, :4] = 11
    assert [(r["main"], r["sub"]) for r in both(T)] == [(69, 4)]
    T[4] = (30, 30, 30, 9, 4, 4, 4, 4)               # an uneven comb: 99 > 32, 9 > 8
    assert len(both(T)) == 1
    T[4] = (9, 9, 9, 9, 4, 4, 4, 4)                  # 36 > 32, 9 > 8
    assert len(both(T)) == 1
    T[4] = (9, 9, 9, 9, 4, 4, 4, 6)                  # s == 2 n = 36, v3 = 9 <= 12
    assert both(T) == []
    E = np.zeros((24, 8), np.uint64)
    E[9, [0, 3, 4, 6, 7]] = 50                       # five equal values: the lower four are the strongest, and v3 == v4
    assert both(E) == []
    E[9, 7] = 0
    assert [(r["main"], r["sub"]) for r in both(E)] == [(tm.PATTERNS.index(0x9a), 9)]
    E[9, 7], E[9, 0] = 24, 49                        # order among 50, 50, 50, 49 | 24: the 49 is v3
    assert both(E)[0]["strong"] == 199 and both(E)[0]["weak"] == 24


def test_detect_on_random_sums_and_large_values():
    rng = np.random.default_rng(22)
    found = 0
    for k in range(300):
        top = 1 << int(rng.integers(1, 63))
        T = rng.integers(0, top, 192, dtype=np.uint64) >> rng.integers(0, 8, 192).astype(np.uint64)
        if k % 3 == 0:                               # combs on top of it, up to 2^62 per value
            for c in rng.integers(0, 24, 3):
                p = tm.PATTERNS[int(rng.integers(0, 70))]
                for b in range(8):
                    if p >> (7 - b) & 1:
                        T[8 * c + b] = rng.integers(1 << 61, 1 << 62, dtype=np.uint64)
        found += len(both(T))
    assert found > 100
    big = np.zeros(192, np.uint64)
    big[8:12], big[12:16] = 2 ** 64 - 1, 2 ** 63 - 1
    r = both(big)
    assert len(r) == 1 and r[0]["strong"] == 2 ** 64 - 1 == r[0]["weak"]      # saturated records, exact comparisons
    big[12:16] = 2 ** 63                                                      # 2 v4 = 2^64 > v3: a 64-bit product would wrap
    assert both(big) == []


def test_shadow_flag():
    T = np.zeros((24, 8), np.uint64)
    T[3, :4], T[10, :4], T[11, 4:] = 6400, 100, 1
    assert [(r["sub"], r["shadow"]) for r in both(T)] == [(3, False), (10, False), (11, False)]          # exactly 64 x: not flagged
    T[3, 0] = 6401
    assert [(r["sub"], r["shadow"]) for r in both(T)] == [(3, False), (10, True), (11, False)]           # just above; another main identifier never
    T[12, :4] = 99
    assert [(r["sub"], r["shadow"]) for r in both(T)] == [(3, False), (10, True), (11, False), (12, True)]


def test_refusals_of_detect():
    L, T = dab.lib(), np.zeros(192, np.uint64)
    recs = (dab.TiiRecord * 24)()
    p = T.ctypes.data_as(dab.C.POINTER(dab.C.c_uint64))
    assert L.dabhip_tii_detect(None, dab.C.cast(recs, dab.C.c_void_p), 24) < 0
    assert L.dabhip_tii_detect(p, dab.C.cast(recs, dab.C.c_void_p), -1) < 0
    assert L.dabhip_tii_detect(p, None, 1) < 0
    assert L.dabhip_tii_detect(p, None, 0) == 0
    with pytest.raises(dab.DabhipError, match="192 sums"):
        dab.tii_detect(T[:-1])
    T[8 * 5:8 * 5 + 4] = 9
    assert L.dabhip_tii_detect(p, None, 0) == 1                               # the count without room for a record


# ---- the modulator ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def capture(combs, ntf, snr=1000.0, seed=1, phase=0, preset=1):
    cfg = dab.synth_preset(preset, seed=seed, snr_db=snr)
    cfg.set_tii(combs, phase)
    iq = dab.synth_generate(cfg, ntf)
    iq.setflags(write=False)
    return iq


@pytest.mark.parametrize("snr, phase", [(1000.0, 0), (9.0, 0), (9.0, 1)])
def test_modulator_touches_only_the_null_symbols_of_the_tii_frames(snr, phase):
    ntf = 4
    plain = capture((), ntf, snr, 7).reshape(ntf, TF, 2)
    tii = capture(((17, 5, 0.0), (40, 9, -10.0)), ntf, snr, 7, phase).reshape(ntf, TF, 2)
    for tf in range(ntf):
        assert np.array_equal(plain[tf, tm.NULL_SAMPLES:], tii[tf, tm.NULL_SAMPLES:]), tf          # the noise draws have not moved
        if (tf + phase) % 2:
            assert np.array_equal(plain[tf], tii[tf]), tf                                              # the other frames' null symbols stay as they were
        else:
            assert not np.array_equal(plain[tf, :tm.NULL_SAMPLES], tii[tf, :tm.NULL_SAMPLES]), tf
    if snr >= 100:
        assert (plain[:, :tm.NULL_SAMPLES] == 127).all()


def test_an_all_zero_extension_is_off():
    cfg = dab.synth_preset(1, seed=3)
    a = dab.synth_generate(cfg, 2)
    cfg.set_tii([], 1)                               # a phase alone switches nothing on
    assert np.array_equal(a, dab.synth_generate(cfg, 2))
    cfg.set_tii([(70, 0, 0.0)])
    with pytest.raises(dab.DabhipError, match="TII comb"):
        dab.synth_generate(cfg, 1)
    cfg.set_tii([(0, 24, 0.0)])
    with pytest.raises(dab.DabhipError, match="TII comb"):
        dab.synth_generate(cfg, 1)


def test_modulator_pair_phases_against_the_phase_reference():
    """The null symbol is sum_k z_k e^(2 pi j k (n - 608) / 2048): the fp64 transform of its samples 608 .. 2655 holds, at the comb's carriers, the
    amplitude 2048 x amplitude x level with the phase-reference phase (dabhip_host_table(3), quarter turns) of the pair's LOWER carrier, and
    next to nothing elsewhere; the first 608 samples repeat the period's last."""
    prs = dab.host_table(3)
    cfg = dab.synth_preset(1, seed=1, amplitude=4.0)
    cfg.set_tii([(23, 11, 0.0), (5, 2, -6.0)])
    iq = dab.synth_generate(cfg, 1).reshape(-1, 2).astype(np.float64) - 127.0
    null = iq[:tm.NULL_SAMPLES, 0] + 1j * iq[:tm.NULL_SAMPLES, 1]
    assert np.array_equal(null[:608], null[2048:2656])
    X = np.fft.fft(null[608:]) / S
    expected = np.zeros(S, complex)
    for (p, c, db) in ((23, 11, 0.0), (5, 2, -6.0)):
        ks = tm.carriers(p, c)
        for i, k in enumerate(ks):
            lower = ks[i & ~1]
            expected[k % S] += 4.0 * 10 ** (db / 20) * 1j ** int(prs[lower + 768 if lower < 0 else lower + 767])
    assert np.abs(X - expected).max() < 0.05         # the cu8 rounding: at most 1 / sqrt 2 LSB per sample, 0.29 / sqrt(2048) rms per bin


# ---- aligned captures through the model's fold and rule -----------------------------------------------------------------------------------------
def ids(recs, flagged=False):
    return [(r["main"], r["sub"]) for r in recs if r["shadow"] == flagged]


def test_one_transmitter_at_5_db():
    T = tm.aligned_capture_sums(capture(((17, 5, 0.0),), 8, 5.0, 11), 8)
    assert ids(both(T)) == [(17, 5)] and ids(both(T), True) == []


def test_three_transmitters_10_db_apart():
    T = tm.aligned_capture_sums(capture(((3, 1, 0.0), (40, 9, -10.0), (69, 23, -20.0)), 16), 16)
    assert ids(both(T)) == [(3, 1), (40, 9), (69, 23)] and ids(both(T), True) == []


@pytest.mark.parametrize("ntf", [2, 8])
def test_nothing_in_noise(ntf):
    for seed in range(20):
        T = tm.aligned_capture_sums(capture((), ntf, 5.0, 100 + seed), ntf)
        assert both(T) == [], seed


def test_window_position_and_phase():
    """Any window inside the null symbol holds one period: the identifiers do not depend on it; with tii_phase = 1 the odd frames carry the comb."""
    iq = capture(((9, 20, 0.0),), 4, 1000.0, 2, 1)
    for fine in (-304, 0, 304):
        assert ids(both(tm.aligned_capture_sums(iq, 4, fine))) == [(9, 20)]
    frames = iq.reshape(4, TF, 2)
    even = tm.frame_sums(frames[0::2], [304, 304], [0, 0]).sum(axis=0, dtype=np.uint64)
    assert both(even) == []


def test_host_rule_under_sanitizers():
    here = os.path.join(ROOT, "tests", "host_sanitize")
    os.makedirs(os.path.join(here, "build"), exist_ok=True)
    exe = os.path.join(here, "build", "tii_units_asan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(here, "tii_units.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "Sanitizer" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.split() == ["ok", "tii-units"]
