"""tests/eti_filter_model.py (what the sub-channel filter must produce, a rewrite of reference frames) held on the CPU: it is the identity on reference
frames when every id is listed, its frames pass the validator, and its header is the GOLD-pinned header builder's (dabhip_host_eti_header, held to the
reference's init_eti by test_host.py) for the kept sub-channels alone.  tests/test_gpu_subch_filter.py then holds the kernels against it."""
import os

import numpy as np
import pytest

import dabtools_amd as dab
import eti_check
import eti_filter_model as fm
import oracle_lib as ol
import subch_filter_cases as cases
import test_oracle_golden as tg

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def reference_frames():
    """{name: frames}: the committed reference ETI (back-end and whole-path fixtures), the oracle's replay of a preset-0 and a preset-1 capture and of
    the 20-sub-channel multiplex."""
    out = {"backend_e2e": np.load(os.path.join(G, "backend_e2e.npz"))["eti"]}
    for ci, _, _, want in tg._e2e_small_cases():
        out["e2e_small case %d" % ci] = want
    out["preset 0"] = ol.or_replay(dab.synth_generate(dab.synth_preset(0, seed=71, cif_count0=123), 18))[0]
    out["preset 1"] = ol.or_replay(dab.synth_generate(dab.synth_preset(1, seed=72, cif_count0=4990, skip_samples=50000), 19))[0]
    out["dense"] = ol.or_replay(dab.synth_generate(cases.dense_cfg(8102), 18))[0]
    assert all(len(f) >= 8 for f in out.values()), {k: len(f) for k, f in out.items()}
    return out


def _ids(frames):
    return sorted({s[0] for f in frames for s in eti_check.parse(f)["stc"]})


def _gold_header(frame):
    """The header of dabhip_host_eti_header for the sub-channels the frame's STC lists and its CIF counter."""
    p = eti_check.parse(frame)
    rows = np.full((64, 8), -1, np.int32)
    for scid, sad, tpl, stl in p["stc"]:
        slform = tpl >> 5
        protlev = (tpl & 0x1F) if slform else (tpl & 0x0F) + 1
        assert stl % 3 == 0
        rows[scid] = [scid, slform, 0, sad, 0, stl // 3 * 8, protlev, -1]      # id, slform, uep_index, start_cu, size_cu, bitrate, protlev, ascty
    lo = p["fct"]
    hi = next(h for h in range(4) if (h * 250 + lo) % 8 == p["fp"])           # any CIF count with this FCT and FP: the header holds no more of it
    return dab.host_eti_header([0, hi, lo], rows)


def _assert_model(frames, ids, what):
    got = fm.filter_frames(frames, ids)
    keep = fm.keep_set(ids)
    assert got.shape == np.asarray(frames).shape
    for lo, hi in _locked_runs(frames):
        assert eti_check.check_sequence(got[lo:hi]) == hi - lo, what
    for f, g in zip(frames, got):
        a, b = eti_check.parse(f), eti_check.parse(g)                             # well formed: FSYNC, FL, HCRC, EOF CRC, padding
        kept = [k for k, s in enumerate(a["stc"]) if keep is None or s[0] in keep]
        assert b["stc"] == [a["stc"][k] for k in kept], what
        assert all(np.array_equal(b["subch"][j], a["subch"][k]) for j, k in enumerate(kept)), what
        assert b["fct"] == a["fct"] and b["fp"] == a["fp"] and np.array_equal(a["fic"], b["fic"]), what
        hdr = _gold_header(g)
        assert hdr.size == 12 + 4 * b["nst"] and np.array_equal(g[:hdr.size], hdr), what + ": header differs from the GOLD-pinned builder's"
    return got


def _locked_runs(frames):
    """[(lo, hi)]: the runs of consecutive frames.  The back-end fixture holds a lock loss: the FCT of the reference's frames jumps there."""
    fct = [int(f[4]) for f in frames]
    cuts = [0] + [k + 1 for k, (a, b) in enumerate(zip(fct, fct[1:])) if (b - a) % 250 != 1] + [len(fct)]
    return list(zip(cuts, cuts[1:]))


def test_the_fast_crc_is_the_validators():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 97, 1000):
        d = rng.integers(0, 256, n, dtype=np.uint8)
        assert fm.crc16(d) == eti_check.crc16_ccitt(d) and fm.crc16(d, 0) == eti_check.crc16_ccitt(d, 0)


def test_identity_on_reference_frames_with_every_id_listed(reference_frames):
    for name, frames in reference_frames.items():
        for ids in (_ids(frames), list(range(64)), None, []):
            assert np.array_equal(fm.filter_frames(frames, ids), frames), (name, ids)
        _assert_model(frames, _ids(frames), name)


def test_keeping_nothing_gives_nst_0_and_fl_25(reference_frames):
    for name, frames in reference_frames.items():
        absent = [i for i in range(64) if i not in _ids(frames)][:3]
        for ids in (absent, [-1, 64, 1000], [64]):
            got = _assert_model(frames, ids, (name, ids))
            for f, g in zip(frames, got):
                p = eti_check.parse(g)
                assert p["nst"] == 0 and p["fl"] == 25 and p["stc"] == [] and np.array_equal(p["fic"], eti_check.parse(f)["fic"])
                assert (g[12 + 96 + 8:] == 0x55).all()


def test_first_last_middle_and_duplicate_ids(reference_frames):
    for name, frames in reference_frames.items():
        ids = _ids(frames)
        for pick in ([ids[0]], [ids[-1]], [ids[len(ids) // 2]], [ids[-1], ids[0]], [ids[-1], ids[-1], ids[0], ids[0], 64, -1]):
            got = _assert_model(frames, pick, (name, pick))
            want_ids = sorted(set(pick) & set(ids))
            assert all([s[0] for s in eti_check.parse(g)["stc"]] == [i for i in want_ids if i in [t[0] for t in eti_check.parse(f)["stc"]]]
                       for f, g in zip(frames, got)), (name, pick)
        assert np.array_equal(fm.filter_frames(frames, [ids[-1], ids[-1], ids[0]]), fm.filter_frames(frames, [ids[0], ids[-1]])), name


def test_dense_multiplex_filters(reference_frames):
    frames = reference_frames["dense"]
    assert _ids(frames) == cases.DENSE_IDS
    stl = {s[0]: s[3] for s in eti_check.parse(frames[0])["stc"]}
    assert stl[cases.DENSE_SMALLEST] == min(stl.values()) == 3 and stl[cases.DENSE_LARGEST] == max(stl.values()) == 48
    for name, ids in cases.DENSE_FILTERS.items():
        got = _assert_model(frames, ids, name)
        p = eti_check.parse(got[0])
        assert [s[0] for s in p["stc"]] == sorted(ids) and p["fl"] == len(ids) + 25 + sum(2 * stl[i] for i in ids), name


def test_the_model_moves_the_bytes_it_says():
    """A hand-made frame, so that the test does not lean on the parser alone: two sub-channels of 24 and 48 bytes, the second kept."""
    f = np.full(6144, 0x55, np.uint8)
    f[0:8] = [0xFF, 0xF8, 0xC5, 0x49, 7, 0x82, (7 << 5) | 8, 2 + 1 + 24 + 6 + 12]
    f[8:16] = [(5 << 2) | 0, 10, (0x21 << 2), 3, (63 << 2) | 1, 44, (0x13 << 2), 6]
    f[16:18] = 0xFF
    c = eti_check.crc16_ccitt(f[4:18]) ^ 0xFFFF
    f[18:20] = [c >> 8, c & 0xFF]
    f[20:116] = np.arange(96)
    f[116:140] = 0xA1
    f[140:188] = np.arange(48) + 100
    c = eti_check.crc16_ccitt(f[20:188]) ^ 0xFFFF
    f[188:190] = [c >> 8, c & 0xFF]
    f[190:196] = 0xFF
    eti_check.parse(f)
    g = fm.filter_frames(f, [63])[0]
    assert list(g[4:8]) == [7, 0x81, (7 << 5) | 8, 1 + 1 + 24 + 12] and list(g[8:12]) == list(f[12:16]) and list(g[12:14]) == [0xFF, 0xFF]
    assert np.array_equal(g[16:112], f[20:116]) and np.array_equal(g[112:160], f[140:188])
    c = eti_check.crc16_ccitt(g[16:160]) ^ 0xFFFF
    assert list(g[160:162]) == [c >> 8, c & 0xFF] and (g[162:168] == 0xFF).all() and (g[168:] == 0x55).all()
    assert np.array_equal(fm.with_fic(g, g[16:112]), g)
    h = fm.with_fic(g, np.zeros(96, np.uint8))
    assert eti_check.parse(h)["fic"].sum() == 0 and np.array_equal(h[112:160], g[112:160])
