"""The lock-in rule (control_plane.hpp: lockin_deferred, dabhip.h: dabhip_host_lockin_deferred) against the back end it restates.

The engine does not demodulate the MSC symbols of the transmission frames the rule names.  That is only right if the back end never reads them:
here the REAL reference back end (oracle/_ref/libdabref.so through the refh_* harness) -- and the oracle's restatement of it, which is always
built -- replays the golden demapped TFs of tests/golden/backend_e2e.npz (9 dB, FIC destroyed in TF 18: lock lost and regained) in pieces, each
piece standing for one decode / one segment of a session.  (locked, okcount) in front of a piece are tracked by the test from the back end's own
lock flag and its per-TF "12 of 12 FIBs good" flags; the MSC bytes of every TF the rule defers are overwritten with random bytes; the ETI output
must be the untouched run's, byte for byte.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import dabtools_amd as dab
import oracle_lib as ol
from oracle_lib import _ptr

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOSS_TF = 18                                         # make_golden.py destroys the FIC of this TF


def _sequence():
    """The golden run (lock at TF 9, frames out of TFs 13..17, loss at 18, lock again at 28) and its TFs 19..31 once more behind it, so that frames come
    out after the second lock-in as well (the back end does not look at the continuity of the CIF counter: dab.c:35-98)."""
    rows = np.load(os.path.join(G, "backend_e2e.npz"))["tf_bits"]
    bits = [np.unpackbits(r) for r in rows] + [np.unpackbits(r) for r in rows[LOSS_TF + 1:]]
    return [(np.ascontiguousarray(b[:9216]), np.ascontiguousarray(b[9216:])) for b in bits]


class _Ref:
    """libdabref.so: dab_process_frame itself"""

    def __init__(self):
        self.L = ol.ref()
        self.h = self.L.refh_new()

    def process(self, fic, msc):
        L, h = self.L, self.h
        idx = L.refh_tfidx(h)                        # the TF buffer this frame is decoded in (a lock loss resets the index afterwards)
        C.memmove(L.refh_tf_fic(h), _ptr(fic), fic.size)
        C.memmove(L.refh_tf_msc(h), _ptr(msc), msc.size)
        L.refh_process(h)
        ok = np.ctypeslib.as_array(L.refh_fib_ok(h, idx), (12,))
        return bool(L.refh_locked(h)), bool((ok != 0).all())

    def eti(self):
        n = self.L.refh_neti(self.h)
        return np.ctypeslib.as_array(self.L.refh_eti(self.h), (n, 6144)).copy() if n else np.zeros((0, 6144), np.uint8)


class _Oracle:
    """liboracle.so: the restatement of the same function"""

    def __init__(self):
        self.L = ol.oracle()
        self.frames = []
        self._cb = C.CFUNCTYPE(None, C.POINTER(C.c_uint8), C.c_void_p)(lambda p, u: self.frames.append(np.ctypeslib.as_array(p, (6144,)).copy()))
        self.L.or_dab_locked.restype = C.c_int
        self.h = self.L.or_dab_new(C.cast(self._cb, C.c_void_p), None)

    def process(self, fic, msc):
        L, h = self.L, self.h
        C.memmove(L.or_dab_tf_fic(h), _ptr(fic), fic.size)
        C.memmove(L.or_dab_tf_msc(h), _ptr(msc), msc.size)
        L.or_dab_process_frame(h)
        fibs, ok = np.zeros((12, 32), np.uint8), np.zeros(12, np.uint8)
        L.or_fic_decode(_ptr(fic), _ptr(fibs), _ptr(ok))              # the oracle's FIC decode of the same bits (what process_frame ran on them)
        return bool(L.or_dab_locked(h)), bool((ok != 0).all())

    def eti(self):
        return np.array(self.frames) if self.frames else np.zeros((0, 6144), np.uint8)


def _replay(make, seq, pieces, rng):
    """-> (ETI frames, indices of the TFs the rule deferred).  pieces: lengths that add up to len(seq); rng None: nothing is overwritten."""
    be = make()
    locked, okcount, at, deferred = False, 0, 0, []
    for n in pieces:
        ndefer = dab.host_lockin_deferred(locked, okcount, n)
        assert ndefer == (0 if locked else min(n, max(0, 9 - okcount)))
        for i in range(n):
            fic, msc = seq[at]
            if i < ndefer:
                deferred.append(at)
                if rng is not None:
                    msc = rng.integers(0, 256, msc.size, dtype=np.uint8)
            locked, good = be.process(fic, msc)
            okcount = okcount + 1 if good else 0
            at += 1
    assert at == len(seq)
    return be.eti(), deferred


def _partitions(n):
    for cut in range(1, n):                           # two decodes, cut at every position
        yield [cut, n - cut]
    for step in (1, 2, 3, 5, 7):                      # sessions of even segments
        yield [step] * (n // step) + ([n % step] if n % step else [])
    yield [sum(p) for p in ([3], [1], [7], [2], [4], [1], [1], [6], [5])] + [n - 30]     # and an uneven one: lock-in straddles several boundaries


@pytest.mark.parametrize("backend", ["reference", "oracle"])
def test_deferred_tfs_are_never_read_by_the_back_end(backend):
    if backend == "reference" and ol.ref() is None:
        pytest.skip("oracle/_ref not built")
    make = _Ref if backend == "reference" else _Oracle
    seq = _sequence()
    n = len(seq)
    want, none = _replay(make, seq, [n], None)
    golden = np.load(os.path.join(G, "backend_e2e.npz"))["eti"]
    assert len(want) > len(golden) and np.array_equal(want[:len(golden)], golden)      # frames before the loss: the golden ones; more after the second lock-in
    assert none == list(range(9))
    rng = np.random.default_rng(20250707)
    total, after_loss = 0, 0
    for pieces in _partitions(n):
        got, deferred = _replay(make, seq, pieces, rng)
        assert got.shape == want.shape and np.array_equal(got, want), pieces
        assert len(deferred) >= 9 and deferred[:9] == list(range(9)), pieces       # the first nine TFs of a fresh back end, however they are cut
        total += len(deferred)
        after_loss += sum(1 for t in deferred if t > LOSS_TF)
        if pieces[0] == LOSS_TF + 1 and len(pieces) == 2:                           # a boundary right behind the loss: okcount = 0, nine more
            assert deferred[9:] == list(range(LOSS_TF + 1, LOSS_TF + 10))
        if set(pieces) == {1}:                                                     # one TF per segment: 9 - okcount shrinks to nothing, TF by TF
            assert deferred == list(range(9)) + list(range(LOSS_TF + 1, LOSS_TF + 10))
    assert total >= 9 and after_loss >= 1


def test_rule_values():
    f = dab.host_lockin_deferred
    assert [f(False, 0, n) for n in (0, 1, 8, 9, 10, 62)] == [0, 1, 8, 9, 9, 9]
    assert [f(False, k, 62) for k in range(12)] == [9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 0, 0]
    assert [f(True, k, 62) for k in (0, 5, 10, 1000)] == [0, 0, 0, 0]
    assert f(False, 4, 3) == 3 and f(False, 0, -1) == 0
