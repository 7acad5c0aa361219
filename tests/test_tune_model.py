"""The ingest stage's tuned mode without a GPU (include/dabhip.h, "ingest stage, tuned mode"; csrc/ingest_plan.hpp): the tuned tap table and the
NCO table against their conditions, the step rule against Python integers, the refusals, the numpy model (tests/tune_model.py) against the
library's bookkeeping on random chunkings, the identity at offset 0, and the model end to end: two neighbouring blocks in one 4.096 Msps capture,
the second up to 20 dB stronger, each through the model and the CPU oracle.  The host rule under sanitizers: a stand-alone program,
tests/host_sanitize/tune_units.cpp."""
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import eti_check
import ingest_cases as cases
import ingest_model as im
import oracle_lib as ol
import tune_cases as tc
import tune_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (2400000, 2500000, 2560000, 2880000, 3000000, 3200000, 4096000, 6000000, 8000000, 8192000, 10000000)


@pytest.mark.parametrize("rate", RATES)
def test_tuned_tap_table_meets_its_conditions(rate):
    taps, L, M, T = dab.ingest_tune_taps("cs16", rate)
    assert L * rate == M * im.OUT_RATE and np.gcd(L, M) == 1 and taps.shape == (L, T)
    assert T == 2 * dab.ingest_taps("cs16", rate)[3] == 8 * -(-8 * M // L)
    t = taps.astype(np.int64)
    assert (t.sum(axis=1) == 16384).all()
    assert np.abs(t).sum(axis=1).max() <= 65535                   # |acc| < 2^31 on int16 input
    proto = t.T.reshape(-1).astype(np.float64)                    # interleaved: h[k L + p] = taps[p][k], at rate L Fin
    nfft = 1 << 21
    resp = np.abs(np.fft.rfft(proto, nfft))
    db = 20 * np.log10(np.maximum(resp / resp[0], 1e-12))
    f = np.arange(resp.size) * (L * rate / nfft)
    assert f[1] < 10e3                                            # the grid is fine enough for both edges
    assert np.abs(db[f <= 768e3]).max() <= 0.05
    assert db[f >= 944e3].max() <= -60.0


def test_identity_rate_has_no_tuned_filter():
    taps, L, M, T = dab.ingest_tune_taps("cu8", 2048000)
    assert (L, M, T) == (1, 1, 0) and taps.size == 0


def test_nco_table():
    cs = dab.ingest_tune_nco().astype(np.int64)
    assert cs.shape == (4096, 2)
    c, s = cs[:, 0], cs[:, 1]
    a = 2 * np.pi * np.arange(4096) / 4096
    assert np.abs(c - 16384 * np.cos(a)).max() <= 0.5 + 1e-6 and np.abs(s - 16384 * np.sin(a)).max() <= 0.5 + 1e-6
    assert [int(c[k]) for k in (0, 1024, 2048, 3072)] == [16384, 0, -16384, 0]
    assert [int(s[k]) for k in (0, 1024, 2048, 3072)] == [0, 16384, 0, -16384]
    i = np.arange(1, 4096)
    assert np.array_equal(c[i], c[4096 - i]) and np.array_equal(s[i], -s[4096 - i])
    i = np.arange(4096)
    assert np.array_equal(c[(i + 1024) % 4096], -s[i])


def test_step_rule():
    rng = np.random.default_rng(9)
    for rate in (2048000, 2400000, 4096000, 8192000, 10000000, 10240000):
        reach = rate // 2 - 768000
        for f in [0, 1, -1, reach, -reach, 856000 if reach >= 856000 else 0] + [int(v) for v in rng.integers(-reach, reach + 1, 200)]:
            want = ((2 * f * (1 << 32) + rate) // (2 * rate)) % (1 << 32)
            assert dab.ingest_tune_step(rate, f) == want == tm.step_rule(rate, f), (rate, f)
    assert dab.ingest_tune_step(4096000, 1024000) == 1 << 30 and dab.ingest_tune_step(4096000, -1024000) == 3 << 30


OFF1 = [0]


@pytest.mark.parametrize("nstreams, fmt, rate, offsets, text", [
    (1, "cs16", 10000000, [], "nchannels must be 1 .. 16"),
    (1, "cs16", 10000000, [0] * 17, "nchannels must be 1 .. 16"),
    (1, "cs16", 10000000, [4232001], "do not lie within"),
    (1, "cs16", 10000000, [0, -4232001], "do not lie within"),
    (1, "cs16", 2400000, [432001], "do not lie within"),
    (1, "cs16", 2048000, [256001], "do not lie within"),
    (4096, "cs16", 10000000, [0] * 16, "nstreams times nchannels"),
    (0, "cs16", 10000000, OFF1, "nstreams times nchannels"),
    (1, "cs16", 2047999, OFF1, "outside"),
    (1, "cs16", 10240001, OFF1, "outside"),
    (1, "cs16", 2400001, OFF1, "1024 filter phases"),
    (1, "cs16", 10229760, OFF1, "bytes of LDS"),                  # 200/999: the plain table fits its 65536 bytes, the tuned one and its tile do not fit 160 KiB
    (1, 7, 2400000, OFF1, "unknown format"),
])
def test_refusals(nstreams, fmt, rate, offsets, text):
    with pytest.raises(dab.DabhipError, match=text):              # the refusal comes before the device is looked for
        dab.Ingest(0, nstreams, fmt, rate, 256, offsets=offsets)


def test_refusals_of_the_host_calls():
    for rate, text in ((2047999, "outside"), (10240001, "outside"), (2400001, "1024 filter phases"), (10229760, "bytes of LDS")):
        with pytest.raises(dab.DabhipError, match=text):
            dab.ingest_tune_taps("cs16", rate)
        with pytest.raises(dab.DabhipError, match=text):
            dab.ingest_tune_plan(rate, [1, 2, 3])
        with pytest.raises(dab.DabhipError, match=text):
            dab.ingest_tune_step(rate, 0)
    dab.ingest_taps("cs16", 10229760)                             # the plain path takes that rate
    with pytest.raises(dab.DabhipError, match="unknown format"):
        dab.ingest_tune_taps("cs24", 2400000)
    with pytest.raises(dab.DabhipError, match="do not lie within"):
        dab.ingest_tune_step(10000000, 4232001)
    assert dab.ingest_tune_step(10000000, 4232000) == tm.step_rule(10000000, 4232000)


def test_accepted_limits():
    for rate in (2048000, 10000000, 10240000):
        dab.ingest_tune_taps("cu8", rate)
    assert dab.ingest_tune_taps("cs16", 10000000)[1:] == (128, 625, 320)


@pytest.mark.parametrize("fmt", ["cu8", "cs8", "cs16", "cf32"])
@pytest.mark.parametrize("rate", [2048000, 2400000, 2500000, 4096000, 10000000])
def test_model_against_the_librarys_bookkeeping_on_random_chunkings(fmt, rate):
    rng = np.random.default_rng(rate // 1000 + len(fmt))
    _, L, M, T = dab.ingest_tune_taps(fmt, rate)
    closes_at = cases.samples_for_outputs(L, M, T, im.W)          # the push that brings this many samples closes the window
    offset = int(rng.integers(-(rate // 2 - 768000), rate // 2 - 768000 + 1))
    for gain in (256, 777, 0):
        n = closes_at + 3000 if gain == 0 else 4000
        raw = cases.random_raw(rng, fmt, n)
        (want, g), = tm.one_shot(fmt, rate, gain, raw, [offset])
        # empty and one-sample pushes, the first output's edge, and with automatic gain the window's end inside a push and at a push's end
        cuts = [0, 0, 1, 2, max(T // 2 - 1, 2), max(T // 2, 2), T // 2 + 1 + 2] + sorted(int(v) for v in rng.integers(T, n + 1, 10)) + [n, n]
        if gain == 0:                                             # W inputs do not close it; then its end inside a push, or exactly at a push's end
            cuts = cuts + [im.W] + ([closes_at - 1, closes_at + 1] if rate in (2400000, 4096000) else [closes_at])
        cuts = sorted(cuts)
        sizes = [b - a for a, b in zip(cuts, cuts[1:])]
        m = tm.TuneModel(fmt, rate, offset, gain)
        outs = [m.push(raw[2 * a:2 * b]) for a, b in zip(cuts, cuts[1:])]
        nout, carried = dab.ingest_tune_plan(rate, sizes, auto_gain=gain == 0)
        assert [o.size // 2 for o in outs] == nout
        assert np.array_equal(np.concatenate(outs), want)
        assert m.g == g and (gain == 0 or g == gain)
        pushed = np.cumsum(sizes)
        for k, c in enumerate(carried):
            held = gain == 0 and pushed[k] < closes_at                    # the window closes on outputs: output W - 1 is not complete yet
            assert c == (pushed[k] if held else min(pushed[k], max(T - 1, 0)))
            assert not held or nout[k] == 0
        if gain == 0 and T:
            assert any(pushed[k] == im.W and nout[k] == 0 and carried[k] == im.W for k in range(len(sizes)))
        assert sum(nout) == want.size // 2 == m.complete()


@pytest.mark.parametrize("rate", [2048000, 2400000, 10000000])
def test_offset_zero_is_the_plain_model_with_the_tuned_table(rate):
    """cs16 at f = 0: c = 16384, s = 0, (x 16384 + 8192) >> 14 = x."""
    rng = np.random.default_rng(rate // 1000)
    raw = cases.random_raw(rng, "cs16", 5000)
    (out, g), = tm.one_shot("cs16", rate, 300, raw, [0])
    plain = im.IngestModel("cs16", rate, 300)
    taps, plain.L, plain.M, plain.T = dab.ingest_tune_taps("cs16", rate)
    plain.taps = taps.astype(np.int64)
    assert g == 300 and np.array_equal(out, plain.push(raw))


def test_mixer_clamp_and_index_rounding():
    m = tm.TuneModel("cs16", 4096000, 512000, 256)                # step = 2^29: the eighth points
    y = m.mix(np.array([[32767, 32767], [-32768, -32768], [-32768, 32767]], np.int64), 1)
    assert y.tolist()[0] == [32767, 0] and y.tolist()[1][0] == -32768          # +-46339 and a half, clamped
    # theta just below a full turn rounds to index 4096, which is index 0
    m.step = (1 << 32) - (1 << 19)
    assert np.array_equal(m.mix(np.array([[1234, -77]], np.int64), 1), [[1234, -77]])
    m.step = (1 << 32) - (1 << 19) - 1
    assert not np.array_equal(m.mix(np.array([[12340, -770]], np.int64), 1), [[12340, -770]])


@pytest.mark.parametrize("variant", list(tc.VARIANTS))
@pytest.mark.parametrize("channel", range(len(tc.OFFSETS)))
def test_two_blocks_decode_through_the_model(channel, variant):
    """Two blocks 1.712 MHz apart in one 4.096 Msps capture, the second up to 20 dB stronger -> model -> CPU oracle: every channel gives well-formed
    frames that carry its modulator's payload, as many as the direct decode gives, less at most one TF of lock-in."""
    cfg = cases.config(channel)
    direct, _ = ol.or_replay(cases.direct(channel))
    out, g = tc.model_output(variant, channel)
    v = out.reshape(-1, 2).astype(np.float64) - 127.0
    assert 24.0 < np.sqrt(np.mean(v * v)) < 40.0                  # the channel's own level set the gain: 32 LSB rms per rail
    eti, _ = ol.or_replay(out)
    assert len(direct) > 0 and len(eti) >= len(direct) - 4
    cif_of = {dab.synth_fibs(cfg, c).tobytes(): c for c in range(4 * cases.NTF)}
    assert eti_check.check_sequence(eti) == len(eti)
    for f in eti:
        p = eti_check.parse(f)
        cif = cif_of[p["fic"].tobytes()]
        assert len(p["subch"]) == cfg.nsub
        for k, data in enumerate(p["subch"]):
            assert np.array_equal(data, dab.synth_payload(cfg, cif, k)), (cif, k)


def test_host_rule_under_sanitizers():
    here = os.path.join(ROOT, "tests", "host_sanitize")
    os.makedirs(os.path.join(here, "build"), exist_ok=True)
    exe = os.path.join(here, "build", "tune_units_asan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(here, "tune_units.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "Sanitizer" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.split() == ["ok", "tune-units"]
