"""The ingest stage without a GPU (include/dabhip.h, "ingest stage"; csrc/ingest_plan.hpp): the tap table against its conditions, the refusals, the
numpy model (tests/ingest_model.py) against the library's bookkeeping on random chunkings, the identity, and the model end to end: captures
resampled to 2.4 Msps by test-only FFT interpolation, through the model and the CPU oracle -- which shows that the filter's phase order and
timing are right.  The host rule under sanitizers: a stand-alone program, tests/host_sanitize/ingest_units.cpp."""
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import eti_check
import ingest_cases as cases
import ingest_model as im
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (2400000, 2500000, 2560000, 2880000, 3000000, 3200000, 4096000, 6000000, 8000000, 8192000, 10000000)


@pytest.mark.parametrize("rate", RATES)
def test_tap_table_meets_its_conditions(rate):
    taps, L, M, T = dab.ingest_taps("cs16", rate)
    assert L * rate == M * im.OUT_RATE and np.gcd(L, M) == 1 and T % 2 == 0 and taps.shape == (L, T)
    t = taps.astype(np.int64)
    assert (t.sum(axis=1) == 16384).all()
    assert np.abs(t).sum(axis=1).max() <= 65535                   # |acc| < 2^31 on 16-bit-domain input
    proto = t.T.reshape(-1).astype(np.float64)                    # interleaved: h[k L + p] = taps[p][k], at rate L Fin
    nfft = 1 << 21
    resp = np.abs(np.fft.rfft(proto, nfft))
    db = 20 * np.log10(np.maximum(resp / resp[0], 1e-12))
    f = np.arange(resp.size) * (L * rate / nfft)
    assert f[1] < 10e3                                            # the grid is fine enough for both edges
    assert np.abs(db[f <= 768e3]).max() <= 0.05
    assert db[f >= 1.28e6].max() <= -60.0


def test_identity_rate_has_no_filter():
    taps, L, M, T = dab.ingest_taps("cu8", 2048000)
    assert (L, M, T) == (1, 1, 0) and taps.size == 0


@pytest.mark.parametrize("fmt, rate, text", [("cs16", 2047999, "outside"), ("cs16", 10240001, "outside"), ("cs16", 2400001, "1024 filter phases"),
                                             (7, 2400000, "unknown format"), (-1, 2400000, "unknown format")])
def test_refusals(fmt, rate, text):
    with pytest.raises(dab.DabhipError, match=text):
        dab.ingest_taps(fmt, rate)
    if isinstance(fmt, str):
        with pytest.raises(dab.DabhipError, match=text):
            dab.ingest_plan(rate, [1, 2, 3])
    with pytest.raises(dab.DabhipError, match=text):              # the refusal comes before the device is looked for
        dab.Ingest(0, 1, fmt, rate, 256)


def test_unknown_format_name_is_refused():
    with pytest.raises(dab.DabhipError, match="unknown format"):
        dab.ingest_taps("cs24", 2400000)


def test_accepted_rate_limits():
    for rate in (2048000, 10240000):
        dab.ingest_taps("cu8", rate)


def test_automatic_gain_rule():
    assert dab.ingest_auto_gain(0) == 256 == im.auto_gain(0)
    assert dab.ingest_auto_gain(1) == (1 << 24) - 1 == im.auto_gain(1)
    assert dab.ingest_auto_gain(2 * im.W * 8192 ** 2) == 256              # 8192 rms per rail = 32 LSB at g = 256
    rng = np.random.default_rng(5)
    for e in [int(v) for v in rng.integers(1, 1 << 47, 200)] + [2 * im.W * 32768 ** 2]:
        assert dab.ingest_auto_gain(e) == im.auto_gain(e), e


@pytest.mark.parametrize("fmt", ["cu8", "cs8", "cs16", "cf32"])
@pytest.mark.parametrize("rate", [2048000, 2400000, 2500000, 4096000, 10000000])
def test_model_against_the_librarys_bookkeeping_on_random_chunkings(fmt, rate):
    rng = np.random.default_rng(rate // 1000 + len(fmt))
    T = dab.ingest_taps(fmt, rate)[3]
    for gain in (256, 777, 0):
        n = im.W + 3000 if gain == 0 else 4000
        raw = cases.random_raw(rng, fmt, n)
        want, g = im.one_shot(fmt, rate, gain, raw)
        # empty and one-sample pushes, the first output's edge, and with automatic gain the window's end inside a push and at a push's end
        cuts = [0, 0, 1, 2, max(T // 2 - 1, 2), max(T // 2, 2), T // 2 + 1 + 2] + sorted(int(v) for v in rng.integers(T, n + 1, 10)) + [n, n]
        if gain == 0:
            cuts = sorted(cuts + [im.W] if rate % 3 else cuts + [im.W - 1, im.W + 1])
        cuts = sorted(cuts)
        sizes = [b - a for a, b in zip(cuts, cuts[1:])]
        m = im.IngestModel(fmt, rate, gain)
        outs = [m.push(raw[2 * a:2 * b]) for a, b in zip(cuts, cuts[1:])]
        nout, carried = dab.ingest_plan(rate, sizes, auto_gain=gain == 0)
        assert [o.size // 2 for o in outs] == nout
        assert np.array_equal(np.concatenate(outs), want)
        assert m.g == g and (gain == 0 or g == gain)
        pushed = np.cumsum(sizes)
        for k, c in enumerate(carried):
            held = gain == 0 and pushed[k] < im.W
            assert c == (pushed[k] if held else min(pushed[k], max(T - 1, 0)))
        assert sum(nout) == want.size // 2 == m.complete()


def test_identity():
    rng = np.random.default_rng(3)
    raw = cases.random_raw(rng, "cu8", 5000)
    out, g = im.one_shot("cu8", 2048000, 256, raw)
    assert g == 256 and np.array_equal(out, raw)


@pytest.mark.parametrize("variant", list(cases.VARIANTS))
@pytest.mark.parametrize("capture", range(len(cases.CAPTURES)))
def test_resampled_capture_decodes_through_the_model(capture, variant):
    """2.4 Msps captures in four formats -> model -> CPU oracle: well-formed frames that carry the modulator's payload, as many as the direct
    decode gives, less at most one TF of lock-in."""
    cfg = cases.config(capture)
    direct, _ = ol.or_replay(cases.direct(capture))
    out, g = cases.model_output(capture, variant)
    assert 0 <= cases.direct(capture).size // 2 - out.size // 2 <= 64 + 20                # whole 64-sample groups, less the filter's last T/2 inputs
    if variant == "cs16_low_auto":
        assert 30 * 256 * 0.8 < g < 30 * 256 * 1.25 * 1.2                # 28 LSB rms / 30 brought to 32 LSB
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
    exe = os.path.join(here, "build", "ingest_units_asan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(here, "ingest_units.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "Sanitizer" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.split() == ["ok", "ingest-units"]
