"""The Reed-Solomon decoder the DAB+, packet-mode and MPEG-2 TS kernels share (csrc/rs_code.hpp: the tables, the Horner step of the syndromes,
rs_solve) on the CPU, at both of its sizes: tests/host_sanitize/rs_units.cpp, a stand-alone program that includes that header, under ASan +
UBSan.  It decodes every crafted word of dabplus_cases.rs_cases() and packet_cases.rs_cases() to what those modules expect (by construction, or
by the independent decoders rs_reference / rs204_reference where only a decoder can say), and words it makes itself with 0 .. t + 3 errors."""
import os
import subprocess

import numpy as np
import pytest

import dabplus_cases as dcs
import packet_cases as pcs
import rs204_reference as ref204

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def exe():
    here = os.path.join(ROOT, "tests", "host_sanitize")
    os.makedirs(os.path.join(here, "build"), exist_ok=True)
    out = os.path.join(here, "build", "rs_units_asan")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", os.path.join(here, "rs_units.cpp"), "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    assert "warning" not in build.stdout, build.stdout[-3000:]
    return out


def run(exe, args, text=None):
    r = subprocess.run([exe] + args, input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout.split("\n")


def crafted_words():
    """[(code, class, label, received, expected word, expected count)] for every case of both stages' modules."""
    out = []
    rng = np.random.default_rng(120)
    cases = dcs.rs_cases()
    assert sorted(cases) == list("abcdefg")
    for cls in sorted(cases):
        for c in cases[cls]:
            rx, want, n = c.apply(dcs.codeword(rng))
            out.append((120, cls, c.label, rx, want, n))
    cases = pcs.rs_cases()
    assert sorted(cases) == sorted(("clean", "e1", "e8", "e9", "parity", "miscorrect", "shortened", "beyond"))
    for cls in sorted(cases):
        for label, rx, want, n, _ in cases[cls]:
            if n is None:
                want, n = ref204.decode(rx)
            out.append((204, cls, label, rx, want, n))
    return out


def test_every_crafted_word_of_both_stages(exe):
    words = crafted_words()
    assert sum(w[0] == 120 for w in words) > 450 and sum(w[0] == 204 for w in words) > 350
    lines = run(exe, ["words"], "".join("%d %s\n" % (code, bytes(bytearray(rx)).hex()) for code, _, _, rx, _, _ in words))
    assert len(lines) == len(words) + 1 and lines[-1] == ""
    counts = {}
    for (code, cls, label, rx, want, n), line in zip(words, lines):
        got_n, got = line.split()
        assert int(got_n) == n, (code, cls, label, got_n, n)
        assert got == bytes(bytearray(want)).hex(), (code, cls, label)
        if n < 0:
            assert got == bytes(bytearray(rx)).hex(), (code, cls, label)
        counts.setdefault(code, set()).add(n)
    # the answers the classes fix by construction are all there: failure, a clean word (packet_cases only), one error, the full t, counts between
    assert counts[120] >= {-1, 1, 2, 3, 4, 5} and counts[204] >= {-1, 0, 1, 4, 8}, counts


def test_words_by_construction(exe):
    out = run(exe, [])
    assert out[0].split() == ["ok", "rs-units"]
    for part, t in zip(out[1].split(";"), (5, 8)):
        f = part.replace(",", "").split()
        nwords, corrected, failed, mis = int(f[1]), int(f[3]), int(f[6]), int(f[8])
        assert nwords == 4000, out[1]
        # 0 .. t + 3 errors in turn: t + 1 of every t + 4 words lie within the bound and are corrected exactly, the other 3 lie beyond it
        rounds, rest = divmod(nwords, t + 4)
        assert corrected == rounds * t * (t + 1) // 2 + sum(range(min(rest, t + 1))), out[1]
        assert failed + mis == 3 * rounds + max(0, rest - (t + 1)), out[1]
