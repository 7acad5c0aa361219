"""eti2mpa (csrc/eti2mpa.cpp) on crafted ETI streams, as a program of its own under ASan + UBSan (tests/host_sanitize/Makefile, target eti2mpa):
a sub-channel that does not lie whole inside the 6144 bytes of its frame is absent from that frame (the kernels' rule: off + 8 STL <= 6144), and
no STC, however wrong, makes the program read or write past the frame.  Expected bytes, exit status and the summary's counts are asserted."""
import os
import subprocess

import numpy as np
import pytest

from dabplus_cases import raw_frame

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sanitize")
ETI = 6144
WANT = 7


def _payload(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _cases():
    """{label: (stdin bytes, expected stdout, exit status, frames, absent)}"""
    out = {}
    # valid frames: the wanted id first, in the middle and last, with and without FIC bytes, STLs of other sizes in every frame
    frames, want = [], b""
    for f in range(6):
        pay = _payload(8 * (3 + 5 * f), f)
        entries = [(2, 30 + f, None), (40, 9, None)]
        entries.insert(f % 3, (WANT, len(pay) // 8, pay))
        frames.append(raw_frame(248 + f, entries, ficf=f & 1))      # the frame count wraps at 250: both sync words
        want += pay
    valid = b"".join(bytes(f) for f in frames)
    out["valid"] = (valid, want, 0, 6, 0)
    # header 12 + 4 x 3 + 96 = 120: 700 + 50 + 3 STL units end exactly at byte 6144; one unit more ends 8 bytes later
    pay = _payload(32, 10)
    exact = raw_frame(0, [(1, 700, None), (2, 50, None), (WANT, 3, pay)])
    assert 120 + 8 * 753 == ETI and bytes(exact[-24:]) == pay[:24]
    later = raw_frame(1, [(1, 700, None), (2, 50, None), (WANT, 4, pay)])
    out["ends at byte 6144"] = (bytes(exact), pay[:24], 0, 1, 0)
    out["ends 8 bytes later"] = (bytes(exact) + bytes(later), pay[:24], 0, 2, 1)
    # header 12 + 4 + 96 = 112: STL 754 fills the frame, 755 and 1023 run past it
    pay = _payload(8 * 754, 11)
    out["one entry filling the frame"] = (bytes(raw_frame(0, [(WANT, 754, pay)])), pay, 0, 1, 0)
    out["one entry, STL 755"] = (bytes(raw_frame(0, [(WANT, 755, pay)])), b"", 4, 1, 1)
    out["one entry, STL 1023"] = (bytes(raw_frame(0, [(WANT, 1023, pay)])), b"", 4, 1, 1)
    out["127 entries of STL 1023, wanted last"] = (bytes(raw_frame(0, [(8 + i % 50, 1023, None) for i in range(126)] + [(WANT, 1023, None)])), b"", 4, 1, 1)
    out["127 entries of STL 1023, wanted last, short"] = (bytes(raw_frame(0, [(8 + i % 50, 1023, None) for i in range(126)] + [(WANT, 3, None)])), b"", 4, 1, 1)
    out["behind an entry past the frame"] = (bytes(raw_frame(0, [(3, 765, None), (WANT, 6, None)])), b"", 4, 1, 1)
    # the entry before ends inside the frame (byte 116 + 6024 = 6140), the wanted one does not
    out["begins inside, ends outside"] = (bytes(raw_frame(0, [(3, 753, None), (WANT, 6, None)])), b"", 4, 1, 1)
    out["good frames around a bad one"] = (valid[:2 * ETI] + bytes(raw_frame(0, [(WANT, 1023, None)])) + valid[2 * ETI:], want, 0, 7, 1)
    out["final frame cut short"] = (valid + bytes(raw_frame(0, [(WANT, 1023, None)]))[:3000], want, 0, 6, 0)
    out["absent from every frame"] = (b"".join(bytes(raw_frame(f, [(9, 12, None)])) for f in range(3)), b"", 4, 3, 3)
    out["no input"] = (b"", b"", 0, 0, 0)
    bad = bytearray(valid)
    bad[2 * ETI + 2] ^= 0x01
    out["bad sync"] = (bytes(bad), want[:8 * 3 + 8 * 8], 2, None, None)      # the third frame: the first two frames' bytes are out
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def exe():
    build = subprocess.run(["make", "-C", HERE, "eti2mpa"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    return os.path.join(HERE, "build", "eti2mpa_asan")


def check(exe, label):
    stdin, want, status, frames, absent = CASES[label]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, str(WANT)], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=60)
    assert b"Sanitizer" not in run.stderr and b"runtime error" not in run.stderr, (label, run.stderr[-3000:])
    assert run.returncode == status, (label, run.returncode, run.stderr[-1000:])
    assert run.stdout == want, (label, len(run.stdout), len(want))
    if status == 2:
        assert b"frame 3: bad sync" in run.stderr, run.stderr
    else:
        assert b"eti2mpa: %d frames, sub-channel %d absent in %d\n" % (frames, WANT, absent) in run.stderr, (label, run.stderr)


@pytest.mark.parametrize("label", sorted(CASES))
def test_eti2mpa_stays_inside_the_frame(exe, label):
    check(exe, label)
