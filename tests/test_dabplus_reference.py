"""The DAB+ CPU model (dabplus_model.py) against checkers that share nothing with it: the Peterson-Gorenstein-Zierler decoder and long-division
encoder of rs_reference.py, and the crafted classes of dabplus_cases.py, whose expected results are known from how they were built.  No GPU.
test_gpu_dabplus_edges.py sends the same classes through the kernels."""
import numpy as np
import pytest

import dabplus_cases as cs
import dabplus_model as m
import rs_reference as ref
from conftest import fresh_seed

RS = cs.rs_cases()


def test_independent_encoder_equals_the_model_encoder():
    rng = np.random.default_rng(3)
    assert ref.GEN == m.GEN
    data = rng.integers(0, 256, (40, 110)).astype(np.uint8)
    data[0] = 0
    data[1] = 255
    data[2, :109] = 0
    many = cs.encode_many(data)
    for d, p in zip(data, many):
        want = ref.encode(d)
        assert (want == m.rs_encode(d)).all() and (want == p).all()
        assert not any(ref.syndromes(np.concatenate([d, want])))
    words = rng.integers(0, 256, (20, 120)).astype(np.uint8)
    assert [list(r) for r in cs.syndromes_many(words)] == [ref.syndromes(w) for w in words] == [m.syndromes(w) for w in words]


def test_field_product_table_equals_the_bitwise_and_the_model_product():
    for a in (0, 1, 2, 3, 0x1D, 0x80, 0xFF):
        for b in range(256):
            assert cs.MUL[a, b] == ref.mul(a, b) == m.gmul(a, b)
    assert all(ref.mul(a, ref.inv(a)) == 1 for a in range(1, 256))


@pytest.mark.parametrize("cls", sorted(RS))
def test_rs_class_reference_model_and_construction_agree(cls):
    cases = RS[cls]
    assert len(cases) > 0, cls
    rng = np.random.default_rng(100 + ord(cls))
    outcomes = []
    for case in cases:
        sent = cs.codeword(rng)
        rx, want, n = case.apply(sent)
        ctx = (cls, len(cases), case.label)
        r_word, r_n = ref.decode(rx)
        m_word, m_n = m.rs_decode(rx)
        assert r_n == n and (r_word == want).all(), ("reference", ctx, r_n, n)
        assert m_n == n and (m_word == want).all(), ("model", ctx, m_n, n)
        if n >= 0:
            assert int((want != rx).sum()) == n and not any(ref.syndromes(want)), ctx
        outcomes.append((n, bool((want == sent).all())))
    ns = [n for n, _ in outcomes]
    if cls in "abc":
        assert ns == [{"a": 1, "b": 2, "c": 5}[cls]] * len(cases) and all(same for _, same in outcomes), (cls, len(cases))
    if cls == "d":                                                      # decodes, but not to what was sent
        assert ns == [5] * len(cases) and not any(same for _, same in outcomes), (cls, len(cases))
    if cls == "e":
        assert ns == [-1] * len(cases), (cls, len(cases))
    if cls in "fg":                                                     # both outcomes occur
        assert -1 in ns and any(n >= 0 for n in ns), (cls, len(cases), ns)


def test_class_a_covers_every_position_and_value():
    pos = [int(np.flatnonzero(c.pattern)[0]) for c in RS["a"]]
    assert sorted(set(pos)) == list(range(120)) and min(pos.count(k) for k in range(120)) >= 3
    assert {int(c.pattern.max()) for c in RS["a"]} == set(range(1, 256))


def test_reference_equals_model_on_fresh_random_words():
    seed = fresh_seed("test_reference_equals_model_on_fresh_random_words")
    rng = np.random.default_rng(seed)
    fails = 0
    for trial in range(300):
        sent = cs.codeword(rng)
        ne = trial % 10 if trial < 250 else 120
        rx = sent.copy()
        if ne == 120:
            rx = rng.integers(0, 256, 120).astype(np.uint8)
        else:
            pos = rng.choice(120, ne, replace=False)
            rx[pos] ^= rng.integers(1, 256, ne).astype(np.uint8)
        a, n = ref.decode(rx)
        b, k = m.rs_decode(rx)
        assert n == k and (a == b).all(), (seed, trial, ne, n, k)
        if ne <= 5:
            assert n == ne and (a == sent).all(), (seed, trial)
        fails += n < 0
    assert fails > 50


def test_fire_code_generator_is_the_standards_product():
    assert cs.polymul2((1 << 11) | 1, 0b101111) == cs.FIRE_GEN == 0x10000 | 0x782F           # (x^11 + 1)(x^5 + x^3 + x^2 + x + 1)
    rng = np.random.default_rng(8)
    for _ in range(50):
        b = rng.integers(0, 256, 9).astype(np.uint8).tobytes()
        assert m.fire_code(b) == cs.fire_code(b) == cs.polymod2(int.from_bytes(b, "big") << 16, cs.FIRE_GEN)
        a = rng.integers(0, 256, int(rng.integers(1, 300))).astype(np.uint8).tobytes()
        assert m.au_crc(a) == cs.au_crc(a)


PARSED = ("fire_ok", "layout_ok", "rfa", "dac_rate", "sbr_flag", "aac_channel_mode", "ps_flag", "mpeg_surround_config", "num_aus", "au_start", "au_len",
          "crc_ok")


@pytest.mark.parametrize("s", cs.RATES)
def test_superframe_classes_parse_to_what_they_were_built_as(s):
    rng = np.random.default_rng(900 + s)
    counts = {}
    for dac, sbr in cs.LAYOUTS:
        classes = cs.superframe_cases(rng, s, dac, sbr)
        assert set(classes) == {"au3", "slice", "flip", "layout", "fire"}
        for cls, cases in classes.items():
            assert len(cases) > 0, (s, dac, sbr, cls)
            counts[cls] = counts.get(cls, 0) + len(cases)
            for label, data, exp in cases:
                got = m.parse(data)
                for f in PARSED:
                    assert got[f] == exp[f], (s, dac, sbr, cls, len(cases), label, f, got[f], exp[f])
                if cls == "flip":
                    n = exp["num_aus"]
                    assert bin(exp["crc_ok"]).count("1") == n - 1, (s, cls, label)
        n = cs.AU_LAYOUT[(dac, sbr)][0]
        assert len(classes["flip"]) == 2 * n
        assert any(3 in exp["au_len"][:n] for _, _, exp in classes["au3"])
        sl = cs.slice_len(s)
        assert any(all(v % sl == 0 for v in exp["au_start"][1:n]) for _, _, exp in classes["slice"])
        assert any(all(v % sl == 1 for v in exp["au_start"][1:n]) for _, _, exp in classes["slice"]) or sl == 1
        assert any(all(v % sl == sl - 1 for v in exp["au_start"][1:n]) for _, _, exp in classes["slice"])
    assert all(v > 0 for v in counts.values()), counts


def _lane(frames, scid):
    sm = m.SyncModel(scid)
    return m.stage(sm, frames), sm.losses


def test_frame_classes_locate_and_sync_as_built():
    cases = cs.frame_cases()
    assert len(cases) >= 18
    for case in cases:
        label, frames, counts, losses = case[:4]
        for scid in cs.FRAME_IDS:
            recs, lost = _lane(frames, scid)
            assert len(recs) == counts[scid] and lost == losses[scid], (label, scid, len(recs), counts[scid], lost)
            assert all(r["fire_ok"] and r["layout_ok"] and r["rs_failed"] == 0 and r["rs_corrected"] == 0 and r["crc_ok"] == (1 << r["num_aus"]) - 1
                       for r in recs), (label, scid)
        if len(case) > 4:                                               # an id listed twice: the first entry's superframes
            recs, _ = _lane(frames, 5)
            assert [r["data"].tobytes() for r in recs] == [sf[:110 * (len(sf) // 120)].tobytes() for sf in case[4]], label


def test_locate_refusals_one_by_one():
    rng = np.random.default_rng(4)
    pay = rng.integers(0, 256, 8 * 1023).astype(np.uint8).tobytes()
    for stl, present in ((0, False), (1, False), (2, False), (3, True), (4, False), (216, True), (219, False), (1023, False)):
        got = m.locate(cs.raw_frame(9, [(5, stl, pay[:8 * stl])]), 5)
        assert got[0] == present and got[1] == 9 and got[2] == stl, (stl, got[:3])
        if present:
            assert got[3].tobytes() == pay[:8 * stl]
    f = cs.raw_frame(1, [(20, 300, None), (21, 237, None), (5, 216, pay[:1728])])
    assert m.locate(f, 5)[0] and m.locate(f, 5)[3].tobytes() == pay[:1728] == f[6144 - 1728:].tobytes()
    assert not m.locate(cs.raw_frame(1, [(20, 300, None), (21, 238, None), (5, 216, pay[:1728])]), 5)[0]
    assert not m.locate(cs.raw_frame(1, [(20, 1023, None), (5, 3, pay[:24])]), 5)[0]            # behind a sub-channel that overruns the frame
    f = cs.raw_frame(1, [(5, 3, pay[:24])], ficf=0)
    assert m.locate(f, 5)[3].tobytes() == pay[:24] == f[16:40].tobytes()
    assert (cs.raw_frame(7, [(5, 3, pay[:24]), (9, 6, pay[24:72])], ficf=0) == m.eti_frame(7, [(5, pay[:24]), (9, pay[24:72])], ficf=0)).all()
    assert (cs.raw_frame(8, [(5, 3, pay[:24])]) == m.eti_frame(8, [(5, pay[:24])])).all()
    assert m.locate(cs.raw_frame(1, []), 5)[:3] == (False, 1, 0)
    f = cs.raw_frame(1, [(5, 6, pay[:48]), (5, 3, pay[48:72])])                                 # listed twice: the first entry
    assert m.locate(f, 5)[2] == 6 and m.locate(f, 5)[3].tobytes() == pay[:48]


def test_rs_lane_and_fast_decoder_equal_the_model_stage():
    """The carriers the GPU tests use: rs_lane's expectation and decode_superframes give what the model's own stage gives."""
    lane = cs.rs_lane({k: v[:7] for k, v in RS.items()}, s=24)
    assert len(lane) == 7
    frames = cs.frames_of(3, [(5, [sf for _, _, sf, _, _, _ in lane])])
    recs, lost = _lane(frames, 5)
    assert len(recs) == len(lane) and lost == 0
    fast = cs.decode_superframes([sf for _, _, sf, _, _, _ in lane])
    for r, (cls, ncase, sf, want, fixed, failed), (data, ffixed, ffailed) in zip(recs, lane, fast):
        assert (r["data"] == want).all() and (data == want).all(), cls
        assert (r["rs_corrected"], r["rs_failed"]) == (fixed, failed) == (ffixed, ffailed), cls
        if cls == "d":
            assert fixed == 5 * ncase and failed == 0
        if cls == "e":
            assert failed == ncase and fixed == 0 and (want == sf[:want.size]).all()
