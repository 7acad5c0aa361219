"""The block scan without a GPU (include/dabhip.h, "block scan"; csrc/scan_blocks.hpp): the model's fixed-point transform (tests/scan_model.py)
against numpy's fp64 transform and against closed forms, the header's range claim on full-scale inputs in Python integers, the library's detect
rule against the model's on the captures of tests/scan_cases.py, on random spectra up to 2^63 per bin, on zeros and on a 17-block spectrum made by
hand, the raster, the refusals and the bookkeeping of the window.  The host rule under sanitizers: a stand-alone program,
tests/host_sanitize/scan_units.cpp."""
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import ingest_cases as cases
import scan_cases as sc
import scan_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = sm.S


def test_transform_against_numpys():
    """X against numpy.fft.fft(x) / 4096 in fp64 on 16 random full-range cs16 segments, per rail and bin, in LSB of X.  Measured: the largest
    deviation is 3.80 LSB, the rms 0.74, the mean +0.50 ((a + t + 1) >> 1 rounds halves up: bin 0, where that bias of all twelve stages adds up,
    averages +3.03); the figures are those of the roundings alone and do not move with the input's level.  Asserted: every deviation below 5 LSB --
    the measurement plus 1.2 LSB, two standard deviations (0.54) of the rounding noise about its mean -- and the rms below 1 LSB."""
    rng = np.random.default_rng(14)
    x = rng.integers(-32768, 32768, (16, S, 2))
    X = sm.transform(x)
    ref = np.fft.fft(x[..., 0] + 1j * x[..., 1], axis=1) / S
    dev = np.stack([X[..., 0] - ref.real, X[..., 1] - ref.imag])
    print("largest deviation %.3f LSB, rms %.3f, mean %+.3f, bin 0 mean %+.3f" % (np.abs(dev).max(), np.sqrt((dev ** 2).mean()), dev.mean(), dev[:, :, 0].mean()))
    assert np.abs(dev).max() < 5.0 and np.sqrt((dev ** 2).mean()) < 1.0


def test_transform_closed_forms():
    """Where rounding leaves the result exact: impulses at the quarter positions (every stage halves an even number), DC, and tones at the table's
    quarter points."""
    k = np.arange(S)
    quarter = {0: (1, 0), 1: (0, -1), 2: (-1, 0), 3: (0, 1)}                      # (-j)^m as (re, im)
    for m, n0 in enumerate((0, 1024, 2048, 3072)):
        x = np.zeros((1, S, 2), np.int64)
        x[0, n0] = (4096 * 5, -4096 * 3)
        X = sm.transform(x)[0]
        rot = np.array([quarter[(m * kk) % 4] for kk in k])                        # e^(-2 pi j k n0 / 4096) = (-j)^(m k)
        want = np.stack([5 * rot[:, 0] + 3 * rot[:, 1], 5 * rot[:, 1] - 3 * rot[:, 0]], axis=1)      # (5 - 3j) (re + j im)
        assert np.array_equal(X, want), n0
    for value in ((32768, 32768), (-32768, 12345), (1, -1), (0, 0)):
        X = sm.transform(np.tile(np.array(value, np.int64), (1, S, 1)))[0]
        assert tuple(X[0]) == value and not X[1:].any()
    for m, k0 in enumerate((0, 1024, 2048, 3072)):                                 # x[n] = A j^(m n): all of it in bin k0
        rot = np.array([quarter[(-m * n) % 4] for n in k])                         # j^(m n) = (-j)^(-m n)
        A = (-32768, 777)
        x = np.stack([A[0] * rot[:, 0] - A[1] * rot[:, 1], A[0] * rot[:, 1] + A[1] * rot[:, 0]], axis=1)[None]
        X = sm.transform(x)[0]
        assert tuple(X[k0]) == A and not np.delete(X, k0, axis=0).any(), k0


def test_range_claim_on_full_scale_inputs():
    """The header's step 4 in Python integers: no rail beyond 46,400 after any stage, no product sum with its 8192 at or beyond 2^31 -- on constant,
    alternating and rotating inputs with both rails at full scale (cu8's 255 gives +32768, cs16 gives -32768), whose energy gathers in one bin."""
    n = np.arange(S)
    segs = []
    for a in (32768, -32768):
        for b in (32768, -32768):
            segs.append(np.tile(np.array([a, b]), (S, 1)))                                          # constant: all of it at DC
            segs.append(np.stack([a * (-1) ** n, b * (-1) ** n], axis=1))                           # alternating: bin 2048
    for k0 in (1, 511, 512, 1024, 1537, 3000):                                                      # 45 degrees at n = 0, turning
        ph = 2 * np.pi * (k0 * n / S + 1 / 8)
        segs.append(np.rint(32768 * np.sqrt(2) * np.stack([np.cos(ph), np.sin(ph)], axis=1)).astype(np.int64))
    square = [np.where(np.cos(2 * np.pi * k0 * n / S + 0.1) >= 0, 32768, -32768) for k0 in (1, 2, 300, 1024)]
    segs += [np.stack([q, q], axis=1) for q in square] + [np.stack([square[2], -square[2]], axis=1)]
    watch = []
    X = sm.transform(np.array(segs), watch, wide=True)
    assert all(type(v) is int for v in X.reshape(-1)[:8])
    print("largest rail per stage:", [w[0] for w in watch], "largest product sum:", max(w[1] for w in watch))
    assert watch[0][0] <= 46341 and max(w[0] for w in watch) <= 46400
    assert max(w[1] for w in watch) < 1 << 31
    assert np.array_equal(X.astype(np.int64), sm.transform(np.array(segs)))                         # and int64 is as good as Python integers
    assert tuple(X[0, 0]) == (32768, 32768)                                                        # the full-scale constant arrives whole


def offsets(recs):
    return [r["offset_hz"] for r in recs]


@pytest.mark.parametrize("nsegments", [16, 64])
@pytest.mark.parametrize("name", list(sc.CASES))
def test_detect_on_the_captures(name, nsegments):
    """The library's rule equals the model's on the model's spectra, and finds what the case holds: every block that is at most 20 dB below its
    neighbour, only the strong one from 26 dB on, one block at 5 dB of in-band SNR, nothing at 0 dB or in noise.  Offsets at 64 segments: within
    1,000 Hz (one bin of a 4.096 Msps capture) of the true one, within the 2,000 Hz of the design for the block 20 dB below its neighbour."""
    P, done = sc.model_spectrum(name, nsegments)
    assert done == nsegments
    got = dab.scan_detect(P, sc.RATE)
    assert got == sm.detect(P, sc.RATE)
    want = sc.CASES[name][1]
    print(name, nsegments, [(r["offset_hz"], r["raw_center_hz"], r["width_hz"]) for r in got])
    assert len(got) == len(want)
    for r, f in zip(got, want):
        weak = "plus20" in name and f < 0
        assert abs(r["offset_hz"] - f) <= (2000 if weak or nsegments < 64 else 1000), (r, f)
        assert sm.MIN_WIDTH <= r["width_hz"] <= sm.MAX_WIDTH and r["name"] == "" and r["in"] * r["ng"] > 4 * max(r["lo"], r["hi"]) * r["nin"]


@pytest.mark.parametrize("i", range(len(cases.CAPTURES)))
def test_detect_a_block_that_fills_the_capture(i):
    """One block at the centre of a 2.048 Msps capture: the guards reach the capture's very edge.  4 and 64 segments place it within 250 Hz (half a
    bin); 1 segment is off by up to 3 kHz, which is why the default is 64."""
    for nsegments, reach in ((1, 3000), (4, 250), (64, 250)):
        P, _ = sc.direct_spectrum(i, nsegments)
        got = dab.scan_detect(P, 2048000)
        assert got == sm.detect(P, 2048000)
        assert len(got) == 1 and abs(got[0]["offset_hz"]) <= reach, (nsegments, got)


def shaped_spectrum(rng, rate, top):
    """Blocks of random level on a random floor, bins up to `top`."""
    P = rng.integers(top // 4096, top // 512, S, dtype=np.uint64)
    f = -rate // 2 + 850000 + int(rng.integers(0, 400000))
    while f + 800000 <= rate // 2:
        lo, hi = ((f - 768000) * S // rate + S // 2, (f + 768000) * S // rate + S // 2)
        level = int(rng.integers(top // 300, top, dtype=np.uint64))
        P[max(lo, 0):hi] = rng.integers(level // 2, level, hi - max(lo, 0), dtype=np.uint64)
        f += int(rng.integers(1600000, 2600000))
    return np.roll(P, S // 2)                                      # built in shifted order


def test_detect_on_random_spectra():
    rng = np.random.default_rng(63)
    found = 0
    for k in range(60):
        rate = int(rng.integers(2048000, 10240001)) if k % 4 else (2048000, 10240000, 4096000)[k // 4 % 3]
        top = (1 << 63) + (1 << 62) if k % 2 else 1 << int(rng.integers(12, 60))
        P = shaped_spectrum(rng, rate, top) if k % 3 else rng.integers(0, top, S, dtype=np.uint64)
        center = int(rng.integers(174000000, 240000000)) if k % 5 == 0 else 0
        got = dab.scan_detect(P, rate, center)
        assert got == sm.detect(P, rate, center), (k, rate)
        assert offsets(got) == sorted(offsets(got))
        found += len(got)
    assert found > 40                                             # the shaped ones hold blocks, also with bins at 2^63 (sums beyond 2^64: saturated records)
    big = dab.scan_detect(shaped_spectrum(rng, 8000000, (1 << 63) + (1 << 62)), 8000000)
    assert big and all(r["in"] == 2 ** 64 - 1 for r in big)


def test_detect_nothing_in_zeros_or_a_flat_spectrum():
    for rate in (2048000, 4096000, 10240000):
        assert dab.scan_detect(np.zeros(S, np.uint64), rate) == [] == sm.detect(np.zeros(S, np.uint64), rate)
        assert dab.scan_detect(np.full(S, 2 ** 64 - 1, np.uint64), rate) == []


def test_seventeen_blocks_are_refused():
    """One block whose lower guard is a comb: at 2.048 Msps ng = 201 is odd, a guard window holds 100 or 101 teeth, and an in-band level of twice a
    tooth puts the candidate threshold between the two -- every other centre bin is a run of its own, all with the block's edges."""
    sh = np.zeros(S, np.uint64)
    sh[512:3585] = 2000
    sh[150:450:2] = 1000
    P = np.roll(sh, S // 2)
    with pytest.raises(sm.TooManyBlocks) as model:
        sm.detect(P, 2048000)
    count = model.value.args[0]
    assert count > 16
    with pytest.raises(dab.DabhipError, match="scan_detect: %d blocks found: more than 16" % count):
        dab.scan_detect(P, 2048000)
    sh[150:450:2] = 0                                             # without the comb: the one block
    assert offsets(dab.scan_detect(np.roll(sh, S // 2), 2048000)) == [0]


def test_raster():
    P, _ = sc.model_spectrum("cs16_plus20")
    got = dab.scan_detect(P, sc.RATE, sc.CENTER)
    assert got == sm.detect(P, sc.RATE, sc.CENTER)
    assert [(r["offset_hz"], r["name"]) for r in got] == [(-856000, "5A"), (856000, "5B")]
    measured = dab.scan_detect(P, sc.RATE)
    for shift in (40000, -40000):                                 # the centre 40 kHz off: nothing within 32 kHz, the measured offsets stay
        off = dab.scan_detect(P, sc.RATE, sc.CENTER + shift)
        assert off == measured == sm.detect(P, sc.RATE, sc.CENTER + shift) and all(r["name"] == "" for r in off)
    assert [r["offset_hz"] for r in dab.scan_detect(P, sc.RATE, sc.CENTER + 30000)] == [-886000, 826000]
    # each of the 38 names once: a block at the centre of a 2.048 Msps capture tuned 10 kHz above the block's frequency
    assert len(sm.RASTER) == 38 and sm.RASTER["5A"] == 174928000 and sm.RASTER["12D"] == 229072000 and sm.RASTER["13F"] == 239200000
    one, _ = sc.direct_spectrum(0, 4)
    for name, hz in sm.RASTER.items():
        got = dab.scan_detect(one, 2048000, hz + 10000)
        assert [(r["offset_hz"], r["name"]) for r in got] == [(-10000, name)] and got == sm.detect(one, 2048000, hz + 10000)


@pytest.mark.parametrize("nstreams, fmt, rate, nsegments, text", [
    (0, "cs16", 4096000, 64, "nstreams must be 1 .. 65535"),
    (65536, "cs16", 4096000, 64, "nstreams must be 1 .. 65535"),
    (1, 7, 4096000, 64, "unknown format"),
    (1, "cs16", 2047999, 64, "outside"),
    (1, "cs16", 10240001, 64, "outside"),
    (1, "cs16", 4096000, 0, "nsegments must be 1 .. 65536"),
    (1, "cs16", 4096000, 65537, "nsegments must be 1 .. 65536"),
])
def test_refusals_of_create(nstreams, fmt, rate, nsegments, text):
    with pytest.raises(dab.DabhipError, match=text):       # the refusal comes before the device is looked for
        dab.Scan(0, nstreams, fmt, rate, nsegments)


def test_refusals_of_the_host_calls():
    zeros = np.zeros(S, np.uint64)
    for rate in (2047999, 10240001):
        with pytest.raises(dab.DabhipError, match="outside"):
            dab.scan_detect(zeros, rate)
    with pytest.raises(dab.DabhipError, match="center_hz"):
        dab.scan_detect(zeros, 4096000, -1)
    with pytest.raises(dab.DabhipError, match="center_hz"):
        dab.scan_detect(zeros, 4096000, 10 ** 12 + 1)
    with pytest.raises(dab.DabhipError, match="4096 bins"):
        dab.scan_detect(zeros[:-1], 4096000)
    with pytest.raises(dab.DabhipError, match="nsegments"):
        dab.scan_plan(0, [1])
    with pytest.raises(dab.DabhipError, match="negative push"):
        dab.scan_plan(4, [1, -1])
    with pytest.raises(dab.DabhipError, match="unknown format"):
        dab.Scan(0, 1, "cs24", 4096000)


@pytest.mark.parametrize("nsegments", [1, 3, 64])
def test_model_against_the_librarys_bookkeeping(nsegments):
    rng = np.random.default_rng(nsegments)
    n = nsegments * S + 5000
    raw = cases.random_raw(rng, "cs16", n)
    want, done = sm.spectrum("cs16", raw, nsegments)
    assert done == nsegments and np.array_equal(want, sm.power(sm.im.to_16bit("cs16", raw)[:nsegments * S].reshape(nsegments, S, 2)))
    cuts = sorted([0, 0, 1, S - 1, S, S + 1, 2 * S + 1, n, n] + [int(v) for v in rng.integers(0, n + 1, 12)])
    sizes = [b - a for a, b in zip(cuts, cuts[1:])]
    m = sm.ScanModel("cs16", nsegments)
    segs = [m.push(raw[2 * a:2 * b]) for a, b in zip(cuts, cuts[1:])]
    nseg, carried = dab.scan_plan(nsegments, sizes)
    assert segs == nseg and sum(nseg) == nsegments and np.array_equal(m.P, want)
    for k, c in enumerate(carried):
        assert c == (0 if cuts[k + 1] >= nsegments * S else cuts[k + 1] % S)
    short = sm.ScanModel("cu8", nsegments)                        # fewer than S samples: no segment, an all-zero spectrum
    assert short.push(np.full(2 * (S - 1), 200, np.uint8)) == 0 and not short.P.any()


def run_unit(name):
    here = os.path.join(ROOT, "tests", "host_sanitize")
    os.makedirs(os.path.join(here, "build"), exist_ok=True)
    exe = os.path.join(here, "build", name + "_units_asan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(here, name + "_units.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "Sanitizer" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.split() == ["ok", name + "-units"]


def test_host_rule_under_sanitizers():
    run_unit("scan")


def test_push_front_under_sanitizers():
    """tests/host_sanitize/push_units.cpp: the front of the ingest's and the scan's push (csrc/sample_push.hpp), the scan's upload clamp and the
    packed mixer table."""
    run_unit("push")


def test_eti_push_front_under_sanitizers():
    """tests/host_sanitize/eti_push_units.cpp: the front of the five pushes of ETI frames (csrc/eti_push.hpp: counts, bounds, refusals, the packed
    per-stream block) and the STC walk of the three locate kernels (csrc/eti_locate.hpp) against a restatement, on hand-built headers."""
    run_unit("eti_push")
