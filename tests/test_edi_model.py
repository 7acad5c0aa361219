"""The EDI model (tests/edi_model.py) and the stage's host-only parts on the CPU: known answers that need no second implementation (the CRC
check value, the generator's roots, parity of the zero and the unit chunk, parity against plain long division), the size rule as a property
over the whole grid, dabhip_edi_plan against the model on that grid with every refusal, unpack(pack(frames)) == frames on the crafted frames
in all three modes, the FCTH and SEQ rule under every cutting into pushes, and tests/host_sanitize/edi_units.cpp, a stand-alone program, under
ASan + UBSan: edi_plan.hpp's sizes, its CRC combine rule, and one stream through the stage's steps on the host against the model's bytes."""
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import edi_cases as cs
import edi_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(0, 0, 1400), (1, 0, 64), (1, 0, 1400), (2, 0, 1472), (2, 2, 1400), (2, 5, 64)]


# ---- known answers ---------------------------------------------------------------------------------------------------------------------------------
def test_crc_check_value_and_the_two_crcs_agree():
    assert m.crc16(b"123456789") == 0xD64E
    rng = np.random.default_rng(1)
    msgs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (1, 2, 9, 255, 1000)]
    for msg in msgs:
        m._check_crcs([msg + m.crc16(msg).to_bytes(2, "big")], "model")        # the bit-by-bit one of unpack against the table one of pack
    assert m._crc16_many(msgs) == [m.crc16(x) for x in msgs]
    with pytest.raises(AssertionError):
        m._check_crcs([msgs[2] + (m.crc16(msgs[2]) ^ 1).to_bytes(2, "big")], "model")


def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x11D
        b >>= 1
    return r


def _long_division(msg207):
    """remainder of msg(x) x^48 by g(x), coefficient by coefficient"""
    g = [int(v) for v in m.GEN[::-1]]                  # highest power first, g[0] = 1
    rem = [int(v) for v in msg207] + [0] * m.RS_P
    for i in range(m.RS_K):
        q = rem[i]
        if q:
            for j in range(1, m.RS_P + 1):
                rem[i + j] ^= _gmul(q, g[j])
    return rem[m.RS_K:]


def test_generator_is_monic_of_degree_48_with_exactly_the_roots_alpha_0_to_47():
    assert len(m.GEN) == 49 and m.GEN[48] == 1
    x = 1
    for e in range(255):
        v = 0
        for coeff in m.GEN[::-1]:
            v = _gmul(v, x) ^ int(coeff)
        assert (v == 0) == (e < 48), e
        x = _gmul(x, 2)


def test_parity_known_answers_and_long_division():
    assert not m.rs_parity(np.zeros((1, 207), np.uint8)).any()
    unit = np.zeros((1, 207), np.uint8)
    unit[0, 206] = 1
    assert m.rs_parity(unit)[0].tolist() == m.GEN[47::-1].tolist()
    rng = np.random.default_rng(48)
    for k in (1, 104, 206, 207):
        chunks = rng.integers(0, 256, (20, k), dtype=np.uint8)
        par = m.rs_parity(chunks)
        words = np.zeros((20, 255), np.uint8)
        words[:, :k] = chunks
        words[:, 207:] = par
        for c, p in zip(chunks, par):
            assert p.tolist() == _long_division(list(c) + [0] * (207 - k)), k
        assert not m.syndromes(words).any()
        words[3, 17 % k] ^= 1
        assert m.syndromes(words)[3].all() and not m.syndromes(words)[[0, 1, 2, 4]].any()      # a single error shows in every syndrome


# ---- the size rule ---------------------------------------------------------------------------------------------------------------------------------
def _worst_cover(c, k, B, f, s, recover):
    """the most bytes of one code word that `recover` fragments carry, counted from the index map"""
    b = np.arange(f * s).reshape(s, f)                 # [j, i] = j f + i
    frag = np.broadcast_to(np.arange(f)[None, :], b.shape)[b < B]
    word = b[b < B] // (k + 48)
    counts = np.bincount(word * f + frag, minlength=c * f).reshape(c, f)
    return int(np.sort(counts, axis=1)[:, ::-1][:, :recover].sum(axis=1).max()) if recover else 0


def test_size_rule_over_the_whole_grid():
    seen, max_f = set(), 0
    for l in cs.GRID_L:
        for recover in cs.GRID_RECOVER:
            for F in cs.GRID_FRAG:
                c, k, z, B, f, s = m.plan(l, 2, recover, F)
                assert z < c and k <= 207, (l, recover, F)
                assert f * s >= B and f * s - B < f, (l, recover, F)
                assert f * s // (k + 48) == c, (l, recover, F)
                assert s <= F, (l, recover, F)
                if l <= m.MAX_L:
                    max_f = max(max_f, f)
                key = (c, k, f, s, recover)
                if key not in seen:
                    seen.add(key)
                    assert _worst_cover(c, k, B, f, s, recover) <= 48, (l, recover, F)
    assert max_f <= 132                                 # the kernels' header array


def _c_plan(l, mode, recover, max_frag):
    out = np.zeros(1, dtype=dab.EDI_SIZES)
    r = dab.lib().dabhip_edi_plan(int(l), mode, recover, max_frag, out.ctypes.data)
    return r, tuple(int(out[0][n]) for n in dab.EDI_SIZES.names)


def test_library_plan_against_the_model_on_the_grid_and_every_refusal():
    for l in cs.GRID_L:
        for F in cs.GRID_FRAG:
            for recover in cs.GRID_RECOVER:
                assert _c_plan(l, 2, recover, F) == (0, m.plan(l, 2, recover, F)), (l, recover, F)
            assert _c_plan(l, 1, 0, F) == (0, m.plan(l, 1, 0, F)), (l, F)
        assert _c_plan(l, 0, 0, 0) == (0, m.plan(l, 0)), l
    assert dab.edi_plan(6620, dab.EDI_PFT_FEC, 2, 1400) == dict(zip("ckzBfs", m.plan(6620, 2, 2, 1400)))
    for args in [(12, 0, 0, 0), (0, 2, 0, 64), (-5, 0, 0, 0), ((1 << 20) + 1, 0, 0, 0), (13, 3, 0, 64), (13, -1, 0, 64), (13, 2, 6, 64), (13, 2, -1, 64),
                 (13, 1, 0, 63), (13, 1, 0, 1473), (13, 2, 0, 63), (13, 2, 5, 1473), (13, 1, 9, 64), (13, 0, 9, 5), (1 << 20, 2, 5, 1472)]:
        want = m.plan_refused(*args)
        assert _c_plan(*args)[0] == -want, args
        if want:
            with pytest.raises(dab.DabhipError):
                dab.edi_plan(*args)
    assert dab.lib().dabhip_edi_plan(100, 0, 0, 0, None) < 0


def test_binding_exports_the_stage():
    names = {"dabhip_edi_" + n for n in ("plan", "create", "destroy", "push", "records", "data", "reset", "stats", "stage_ms")}
    assert names <= set(dab.exported_symbols())
    assert dab.EDI_STAGES == ("plan", "scan", "assemble", "rs", "fragment") and dab.EDI_STATS == m.STATS and dab.EDI_REC.itemsize == 32
    assert (dab.EDI_AF, dab.EDI_PFT, dab.EDI_PFT_FEC) == (0, 1, 2) and callable(dab.Edi.reset)
    if dab.lib().dabhip_device_count() == 0:
        with pytest.raises(dab.DabhipError, match="no HIP device"):
            dab.Edi(1)


# ---- pack and unpack -------------------------------------------------------------------------------------------------------------------------------
def _round_trip(frames, mode, recover, max_frag, seq0=0):
    data, recs = m.pack(frames, mode, recover, max_frag, seq0)
    fields, infos = m.unpack(data, mode)
    kept = [f for f in frames if m.accepted(f) is not None]
    assert len(fields) == len(kept)
    for i, (got, f) in enumerate(zip(fields, kept)):
        assert m.same_fields(got, f), i
        assert got["seq"] == (seq0 + i) & 0xFFFF
    assert [(r[0], r[1], r[3], r[4], r[5]) for r in recs] == infos
    return data, recs, fields


@pytest.mark.parametrize("mode,recover,max_frag", MODES)
def test_unpack_of_pack_gives_the_frames_back(mode, recover, max_frag):
    frames = cs.border_frames()
    data, recs, fields = _round_trip(frames, mode, recover, max_frag, seq0=65534)
    numbers = [i for i, f in enumerate(frames) if m.accepted(f) is not None]
    assert sorted(set(r[2] for r in recs)) == numbers and len(numbers) == len(frames) - 4
    assert sorted({len(m.af_body(f, 0, 0)) + 2 for f in frames if m.accepted(f) is not None} & set(cs.BORDER_L)) == sorted(cs.BORDER_L)
    if mode == 2:
        borders = cs.size_borders(recover, max_frag)
        rng = np.random.default_rng(5)
        _round_trip([cs.frame_of_l(rng, l, i) for i, l in enumerate(borders.values())], mode, recover, max_frag)


def test_unpack_sees_a_broken_byte():
    frames = cs.border_frames()[:12]
    for mode, recover, max_frag in ((0, 0, 1400), (1, 0, 255), (2, 1, 255)):
        data = m.pack(frames, mode, recover, max_frag)[0].copy()
        data[len(data) // 2] ^= 0x10
        with pytest.raises(AssertionError):
            m.unpack(data, mode)


# ---- FCTH and SEQ ----------------------------------------------------------------------------------------------------------------------------------
def test_fcth_by_hand():
    frames = cs.fct_frames(cs.FCT_SEQUENCES["skipped at a wrap"])
    fields, _ = m.unpack(m.pack(frames)[0], 0)
    assert [x["fcth"] for x in fields] == [0, 0, 1, 1, 2] and [x["fct"] for x in fields] == [248, 249, 1, 2, 0]
    fields, _ = m.unpack(m.pack(cs.fct_frames([5, 4] * 21))[0], 0)
    assert [x["fcth"] for x in fields][-5:] == [19, 19, 0, 0, 1]                        # 19 -> 0
    fields, _ = m.unpack(m.pack(cs.fct_frames([1, 2, 3, 4]), seq0=65534)[0], 0)
    assert [x["seq"] for x in fields] == [65534, 65535, 0, 1]


@pytest.mark.parametrize("name", sorted(cs.FCT_SEQUENCES))
def test_fcth_and_seq_under_every_cutting_into_pushes(name):
    frames = cs.fct_frames(cs.FCT_SEQUENCES[name])
    for mode, recover, max_frag in ((0, 0, 1400), (2, 1, 64)):
        whole = m.Stream(mode, recover, max_frag, 65534)
        want, want_recs = whole.push(frames)
        for sizes in cs.cuttings(len(frames)):
            st = m.Stream(mode, recover, max_frag, 65534)
            parts, recs, at, base = [], [], 0, 0
            for n in [0] + sizes + [0]:                # pushes of no frame at both ends
                d, r = st.push(frames[at:at + n])
                at += n
                parts.append(d)
                recs += [(base + x[0],) + x[1:] for x in r]
                base += d.size
            assert (np.concatenate(parts) == want).all() and recs == want_recs and st.stat_list() == whole.stat_list(), (name, sizes)


def test_reset_returns_fcth_and_seq_and_keeps_the_numbers():
    frames = cs.fct_frames([9, 3, 4, 1])
    st = m.Stream(0, seq0=7)
    st.push(frames)
    st.reset()
    data, recs = st.push(frames)
    fields, _ = m.unpack(data, 0)
    assert [x["fcth"] for x in fields] == [0, 1, 1, 2] and [x["seq"] for x in fields] == [7, 8, 9, 10] and [r[2] for r in recs] == [4, 5, 6, 7]
    assert st.stats["frames"] == 8


# ---- the shared header under sanitizers ------------------------------------------------------------------------------------------------------------
def _units_exe():
    here = os.path.join(ROOT, "tests", "host_sanitize")
    os.makedirs(os.path.join(here, "build"), exist_ok=True)
    exe = os.path.join(here, "build", "edi_units_asan")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(here, "edi_units.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    return exe


def _run_units(args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "Sanitizer" not in run.stderr, run.stderr[-4000:]
    out = run.stdout.split("\n")
    assert out[0].split() == ["ok", "edi-units"]
    return out[1]


def test_rule_header_under_sanitizers(tmp_path):
    exe = _units_exe()
    words = _run_units([exe]).replace(";", "").replace(",", "").split()
    assert words[:3] == ["sizes:", str(len(cs.GRID_L) * 6 * 5), "combinations"], words
    assert int(words[words.index("frame") + 1]) <= 132 and int(words[words.index("cover") + 1]) <= 48, words
    assert int(words[words.index("crc:") + 1]) >= sum(n + 1 for n in range(1, 301)) + 200, words
    frames = cs.border_frames() + cs.fct_frames(cs.FCT_SEQUENCES["skipped at a wrap"])
    src = tmp_path / "in.eti"
    np.concatenate(frames).tofile(src)
    for mode, recover, max_frag in MODES:
        dst = tmp_path / ("out%d%d%d.edi" % (mode, recover, max_frag))
        want, recs = m.pack(frames, mode, recover, max_frag, 65534)
        line = _run_units([exe, str(src), str(mode), str(recover), str(max_frag), "65534", str(dst)])
        assert line == "stage: %d packets" % len(recs)
        assert dst.read_bytes() == want.tobytes(), (mode, recover, max_frag)
