"""The sub-channel filter (dabhip_*_set_subchannels, dab2eti-hip --subch) against tests/eti_filter_model.py: every filtered frame, whole, must be the
model's rewrite of the reference's unfiltered frame (the oracle's replay of the same capture).  The filter changes work in every stage behind the
FIC -- the layouts and fault check of the control plane, the cached header, the code words and groups of the MSC batch, every sub-channel's offset in
the frame, the EOF CRC's length -- so it is run in every decoder form, with soft decisions, across reconfigurations, lock loss, sessions, several
slices, a split decode, poisoned multiplexes, into the stages behind the decoder and through the CLI.

The only comparisons of GPU with GPU: a split decode with the unsplit one, and filtered with unfiltered frames through DabPlus / Ts / eti2aac.  All
comparisons are exact.  Captures are 18 to 28 TF (lock takes 10, the ring 4 more: 18 TF give 12 frames) of 1 to 6 streams."""
import functools
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import eti_check
import eti_filter_model as fm
import oracle_lib as ol
import subch_filter_cases as cases
import test_gpu_channel as channel
from test_gpu_decoder_forms import FORM_PAIRS, _assert_report
from test_gpu_fault import POISONS

pytestmark = pytest.mark.gpu


# ---- captures and their reference frames, made once and left alone ---------------------------------------------------------------------------------
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _capture(name):
    """(IQ bytes, the oracle's ETI frames) of a named capture."""
    make = {
        "dense": lambda: (cases.dense_cfg(8102), 18),
        "dense-b": lambda: (cases.dense_cfg(8105), 18),
        "dense-9dB": lambda: (cases.dense_cfg(8103, snr=9.0, skip=61003), 20),          # starts inside a TF: the cut TF and the next go to the front end
        "edge": lambda: (cases.edge_cfg(), 18),
        "large": lambda: (cases.large_cfg(), 18),
        "preset0": lambda: (dab.synth_preset(0, seed=7311, cif_count0=123), 18),
        "preset1": lambda: (dab.synth_preset(1, seed=7312, cif_count0=4990, skip_samples=50000), 20),
    }[name]
    cfg, ntf = make()
    iq = dab.synth_generate(cfg, ntf)
    want = ol.or_replay(iq)[0]
    assert want.shape[0] >= 12, (name, want.shape)
    return _frozen(iq), _frozen(want)


@functools.lru_cache(maxsize=None)
def _expected(name, ids):
    """The model's frames for a named capture under the filter `ids` (a tuple; None = no filter)."""
    return _frozen(fm.filter_frames(_capture(name)[1], None if ids is None else list(ids)))


@functools.lru_cache(maxsize=None)
def _soft_replay(name):
    return _frozen(ol.or_replay_soft(_capture(name)[0], ol.SOFT_Q4)[0])


def _assert_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        k = int(np.flatnonzero((got != want).any(axis=1))[0])
        at = np.flatnonzero(got[k] != want[k])
        raise AssertionError("%s: frame %d of %d differs from the model at bytes %s ..." % (what, k, len(got), at[:8].tolist()))


def _assert_named(obj, names, ids, what):
    for b, name in enumerate(names):
        _assert_equal(obj.eti(b), _expected(name, tuple(ids)), "%s, stream %d (%s), filter %s" % (what, b, name, list(ids)))


def _feed_odd(session, caps, sizes=(1000003, 777777, 2222221, 393217)):
    """Feed the captures in segments of odd sizes (they cut inside a TF, inside a sample pair) -> the frames of every stream, all segments."""
    got = [[] for _ in caps]
    pos, k = 0, 0
    while pos < max(c.size for c in caps):
        n = sizes[k % len(sizes)]
        session.feed([c[pos:pos + n] for c in caps])
        for b in range(len(caps)):
            got[b].append(session.eti(b))
        pos, k = pos + n, k + 1
    assert k >= 3
    return [np.concatenate(g) for g in got]


# ---- every decoder form ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msc,fic", FORM_PAIRS)
def test_every_decoder_form_under_every_filter(msc, fic):
    """The 20-sub-channel multiplex, clean and at 9 dB from a mid-frame start (the parity guard keeps the hard decisions the oracle's), under the
    five filters; the two-kernel OFDM stage on one of them, the fused one on the others."""
    names = ["dense", "dense-9dB"]
    caps = [_capture(n)[0] for n in names]
    eng = dab.Engine(0)
    eng.set_decoder_forms(msc=msc, fic=fic)
    unfused = sorted(cases.DENSE_FILTERS)[[p[0] for p in FORM_PAIRS].index(msc) % len(cases.DENSE_FILTERS)]
    for fname, ids in cases.DENSE_FILTERS.items():
        eng.set_subchannels(ids)
        eng.set_fused(fname != unfused)
        assert eng.decode(caps) == sum(len(_capture(n)[1]) for n in names)
        _assert_report(eng, msc, fic)
        _assert_named(eng, names, ids, "%s/%s %s" % (msc, fic, fname))
    eng.close()


# ---- soft decisions --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msc,fic,soft_lanes", [("lane", "lane", False), ("four", "four", True), ("two-plain", "lane", True)])
def test_soft_decisions_under_a_filter(msc, fic, soft_lanes):
    """A clean capture against the model of the oracle's soft replay (what test_gpu_soft.py takes as expected).  No value tolerance enters: the
    comparison is exact, and on a clean capture the oracle's soft frames are its hard ones -- a value one step off cannot move a byte there."""
    iq, hard = _capture("dense")
    want = _soft_replay("dense")
    assert np.array_equal(want, hard)
    eng = dab.Engine(0)
    eng.set_soft(True)
    eng.set_soft_lanes(soft_lanes)
    eng.set_decoder_forms(msc=msc, fic=fic)
    for fname in ("every-second", "largest", "first-and-last"):
        ids = cases.DENSE_FILTERS[fname]
        eng.set_subchannels(ids)
        assert eng.decode([iq]) == len(want)
        _assert_report(eng, msc, fic)
        _assert_equal(eng.eti(0), fm.filter_frames(want, ids), "soft %s %s" % (msc, fname))
    eng.close()


# ---- only the kept code words are decoded ------------------------------------------------------------------------------------------------------
def test_only_the_kept_code_words_are_decoded():
    """Engine.msc_plan() under a filter lists the trellis-step counts of the kept sub-channels only: a filter that decoded everything and dropped
    bytes afterwards fails here.  A filter that keeps nothing present: no group, no MSC launch, the full number of frames with NST 0."""
    iq, want = _capture("dense")
    eng = dab.Engine(0)
    eng.set_decoder_forms(msc="lane", fic="lane")
    eng.set_subchannels([])
    assert eng.decode([iq]) == len(want)
    all_steps = set(eng.msc_plan()[0].tolist())
    filters = [cases.DENSE_FILTERS[k] for k in ("first-and-last", "every-second", "smallest", "largest")]
    alone = {}
    for i in sorted({i for ids in filters for i in ids}):
        eng.set_subchannels([i])
        assert eng.decode([iq]) == len(want)
        steps = eng.msc_plan()[0]
        assert len(steps) == 1, (i, steps)                                   # 12 code words of one shape: one group
        alone[i] = set(steps.tolist())
        _assert_named(eng, ["dense"], [i], "alone")
    assert len(set.union(*alone.values())) >= 6 and set.union(*alone.values()) <= all_steps
    for ids in filters:
        eng.set_subchannels(ids)
        assert eng.decode([iq]) == len(want)
        steps = eng.msc_plan()[0]
        assert set(steps.tolist()) == set.union(*(alone[i] for i in ids)), ids
        assert len(steps) == len(ids), ids                                   # one group per kept sub-channel, not one per sub-channel of the ensemble
    # nothing present is kept: alone ...
    for ids in ([2, 3], [64], [-1, 1000]):
        eng.set_subchannels(ids)
        assert eng.decode([iq]) == len(want)
        steps, _ = eng.msc_plan()
        m, f = eng.decoder_forms(masks=True)
        assert len(steps) == 0 and m == 0 and f == 1 << dab.FORMS["lane"], (ids, steps, m, f)
        assert eng.launch_report()["decoder"] == 0 and eng.stream_status(0) == 0
        got = eng.eti(0)
        assert len(got) == len(want) and all(eti_check.parse(g)["nst"] == 0 for g in got)
        _assert_named(eng, ["dense"], ids, "nothing kept")
    # ... and beside two streams that carry sub-channels: ids 1 and 58 exist in the dense multiplex, not in the one of ids 0, 31, 32, 63
    names = ["dense", "edge", "dense-b"]
    eng.set_subchannels([1, 58])
    assert eng.decode([_capture(n)[0] for n in names]) == sum(len(_capture(n)[1]) for n in names)
    assert set(eng.msc_plan()[0].tolist()) == alone[1] | alone[58]
    _assert_report(eng, "lane", "lane")
    _assert_named(eng, names, [1, 58], "one stream of three keeps nothing")
    assert all(eti_check.parse(g)["nst"] == 0 for g in eng.eti(1)) and all(eti_check.parse(g)["nst"] == 2 for g in eng.eti(0))
    eng.close()


# ---- ids at the mask's ends ------------------------------------------------------------------------------------------------------------------
def test_ids_at_the_ends_of_the_mask():
    iq, want = _capture("edge")
    assert [s[0] for s in eti_check.parse(want[0])["stc"]] == cases.EDGE_IDS
    eng = dab.Engine(0)
    for ids in cases.EDGE_FILTERS:
        eng.set_subchannels(ids)
        assert eng.decode([iq]) == len(want)
        _assert_named(eng, ["edge"], ids, "mask ends")
        kept = [s[0] for s in eti_check.parse(eng.eti(0)[0])["stc"]]
        assert kept == (cases.EDGE_IDS if ids == [] else sorted(set(ids) & set(cases.EDGE_IDS))), (ids, kept)
    assert np.array_equal(eng.eti(0), want)                                 # [] came last: the reference's frames again
    eng.close()
    st = dab.Stream(1, subchannels=[63, 63, 0])
    _assert_equal(_feed_odd(st, [iq])[0], _expected("edge", (63, 63, 0)), "session, ids 63 and 0")
    st.close()


# ---- streams with different ensembles in one batch ---------------------------------------------------------------------------------------------
def test_different_ensembles_in_one_batch_under_one_filter():
    names = ["preset0", "preset1", "dense"]
    caps = [_capture(n)[0] for n in names]
    present = [{s[0] for s in eti_check.parse(_capture(n)[1][0])["stc"]} for n in names]
    eng = dab.Engine(0)
    for ids in ([2, 5, 7, 9, 40, 58], [12], [3, 4]):
        assert any(set(ids) & p for p in present) and any(set(ids) - p for p in present)      # the ids exist in some streams and not in others
        eng.set_subchannels(ids)
        assert eng.decode(caps) == sum(len(_capture(n)[1]) for n in names)
        _assert_named(eng, names, ids, "mixed batch")
    eng.close()


# ---- a large code word at offsets that move ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msc,fic", [("lane", "lane"), ("four", "four")])
def test_a_large_code_word_at_offsets_that_move(msc, fic):
    """EEP 3-A n = 72, the longest code word the reference decodes, from CU 47 on between small sub-channels: alone it moves to the front of the
    MST, without it the small ones close up, with the last small one two code words of very different length share the frame."""
    iq, want = _capture("large")
    stc = eti_check.parse(want[0])["stc"]
    assert [s[0] for s in stc] == sorted(cases.LARGE_SMALL_IDS + [cases.LARGE_ID]) and dict((s[0], s[3]) for s in stc)[cases.LARGE_ID] == 216
    eng = dab.Engine(0)
    eng.set_decoder_forms(msc=msc, fic=fic)
    for fname, ids in cases.LARGE_FILTERS.items():
        eng.set_subchannels(ids)
        assert eng.decode([iq]) == len(want)
        _assert_report(eng, msc, fic)
        _assert_named(eng, ["large"], ids, "%s %s" % (msc, fname))
    eng.close()


# ---- reconfiguration -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reconf():
    """The captures of test_gpu_channel.reconf_configs(), cut a few TFs behind their last change, and the oracle's frames."""
    out = []
    for name, cfg, _ in channel.reconf_configs():
        last = max(cfg.reconf[k].at_cif for k in range(2))
        iq = dab.synth_generate(cfg, last // 4 + 8)
        want = ol.or_replay(iq)[0]
        layouts = {(int(f[5]) & 0x7f, ((int(f[6]) & 7) << 8) | int(f[7])) for f in want}
        assert len(want) >= 24 and len(layouts) >= 2, (name, len(want), layouts)       # frames of both multiplexes
        out.append((name, _frozen(iq), _frozen(want)))
    return out


RECONF_FILTERS = {
    "ids that appear only after the change": [20, 33],
    "ids that are moved, re-protected or resized": [2, 5],
    "ids that swap places and kinds": [1, 2],
    "an id the FIC drops": [12],
    "kept ids stay while an unlisted one appears": [1, 9],
}


@pytest.mark.parametrize("which", sorted(RECONF_FILTERS))
def test_reconfiguration_under_a_filter(which):
    ids = RECONF_FILTERS[which]
    runs = _reconf()
    caps = [iq for _, iq, _ in runs]
    wants = [fm.filter_frames(want, ids) for _, _, want in runs]
    if which == "kept ids stay while an unlisted one appears":
        # capture 0: SubChId 20 appears beside 1, 2, 5, 9.  The unfiltered frames change, the layout list grows; the filtered header must not
        nst = {int(f[5]) & 0x7f for f in runs[0][2]}
        assert nst == {4, 5} and len({(int(f[5]), int(f[6]) & 7, int(f[7])) for f in wants[0]}) == 1 and wants[0][0][5] == 0x82      # NST and FL stay
    if which == "an id the FIC drops":
        assert all([s[0] for s in eti_check.parse(f)["stc"]] == [12] for f in wants[2])          # merge_info never removes: it stays to the end
    eng = dab.Engine(0)
    eng.set_subchannels(ids)
    assert eng.decode(caps) == sum(len(w) for w in wants)
    for b, (name, _, _) in enumerate(runs):
        _assert_equal(eng.eti(b), wants[b], "%s: engine, %s" % (which, name))
        assert eng.stream_status(b) == 0
    eng.close()
    st = dab.Stream(len(caps), subchannels=ids)
    for b, got in enumerate(_feed_odd(st, caps)):
        _assert_equal(got, wants[b], "%s: session, %s" % (which, runs[b][0]))
    st.close()


# ---- lock loss and re-lock -----------------------------------------------------------------------------------------------------------------------
def test_lock_loss_and_relock_under_a_filter():
    """A drop-out and return: the signal is gone for the three FIC symbols of TF 18 (the null and phase reference symbols stay, so the front end keeps
    its timing; test_gpu_frontend_ref.py's degenerate set drops whole TFs, an odd number of bytes, and never locks again).  The back end loses lock
    on that TF, drops its ring, and locks and fills it again.  The operator log does not depend on the filter: it dumps the whole ensemble."""
    cfg = dab.synth_preset(1, seed=781, cif_count0=4990)
    cap = dab.synth_generate(cfg, 36).copy()
    gone = 18 * dab.TF_BYTES + 2 * (2656 + 2552)                          # behind the null symbol and the phase reference symbol
    cap[gone:gone + 2 * 3 * 2552] = 128
    want = ol.or_replay(cap)[0]
    cif = [next(c for c in range(4 * 36) if np.array_equal(dab.synth_fibs(cfg, c), eti_check.parse(f)["fic"])) for f in want]
    jumps = [b - a for a, b in zip(cif, cif[1:]) if b - a != 1]
    assert len(want) >= 24 and len(jumps) == 1 and jumps[0] > 16, (len(want), jumps)          # frames on both sides of the loss, a ring apart and more
    ids = [2, 9]
    exp = fm.filter_frames(want, ids)
    eng = dab.Engine(0)
    eng.decode([cap])
    assert np.array_equal(eng.eti(0), want)
    log = eng.log(0)
    assert log.count("Locked\n") == 2 and "Lock lost, resetting ringbuffer\n" in log and "SubChId=5," in log
    eng.set_subchannels(ids)
    assert eng.decode([cap]) == len(want)
    _assert_equal(eng.eti(0), exp, "engine")
    assert eng.log(0) == log
    eng.close()
    st = dab.Stream(1, subchannels=ids)
    _assert_equal(_feed_odd(st, [cap])[0], exp, "session")
    assert st.log(0) == log
    st.close()


# ---- sessions and several slices -------------------------------------------------------------------------------------------------------------
def test_sessions_and_slices_under_a_filter():
    names = ["preset0", "preset1", "dense"]
    caps = [_capture(n)[0] for n in names]
    ids = [5, 9, 40]
    # a session: the filter is the creation's; a later one is refused and changes nothing
    st = dab.Stream(3, subchannels=ids)
    st.feed([c[:1000003] for c in caps])
    other = (dab.C.c_int32 * 1)(1)
    assert dab.lib().dabhip_stream_set_subchannels(st._h, other, 1) == -1
    assert dab.last_error() == "stream_set_subchannels: only before the first segment"
    got = [[st.eti(b)] for b in range(3)]
    rest = _feed_odd(st, [c[1000003:] for c in caps])
    for b, name in enumerate(names):
        _assert_equal(np.concatenate(got[b] + [rest[b]]), _expected(name, tuple(ids)), "session, %s" % name)
    st.close()
    # three streams over two slices of one device
    mu = dab.Multi([0, 0])
    mu.set_subchannels(ids)
    assert mu.decode(caps) == sum(len(_capture(n)[1]) for n in names)
    assert {mu.slice_of(b)[0] for b in range(3)} == {0, 1}
    _assert_named(mu, names, ids, "Multi, two slices")
    mu.close()
    ms = dab.MultiStream(3, [0, 0], subchannels=ids)
    assert {ms.slice_of(b)[0] for b in range(3)} == {0, 1}
    for b, g in enumerate(_feed_odd(ms, caps)):
        _assert_equal(g, _expected(names[b], tuple(ids)), "MultiStream, %s" % names[b])
    ms.close()


# ---- a split decode ------------------------------------------------------------------------------------------------------------------------------
def test_a_split_decode_under_a_filter():
    names = ["dense", "dense-b"]
    caps = [_capture(n)[0] for n in names]
    ids = cases.DENSE_FILTERS["every-second"]
    eng = dab.Engine(0)
    eng.set_decoder_forms(msc="lane", fic="lane")
    eng.set_subchannels(ids)
    assert eng.decode(caps) == 24
    assert eng.launch_report()["decoder"] == 1
    unsplit = [eng.eti(b) for b in range(2)]
    steps = eng.msc_plan()[0]
    assert len(steps) == len(ids)
    eng.set_launch_limits(decision_rows=(int(steps[0]) + 7) // 8 * 8)        # one group of the longest class per slice
    assert eng.decode(caps) == 24
    r = eng.launch_report()
    assert 3 <= r["decoder"] <= len(ids) and r["decoder"] == r["decoder_planned"], r
    for b in range(2):
        assert np.array_equal(eng.eti(b), unsplit[b]), b
    _assert_named(eng, names, ids, "split decode")
    eng.close()


# ---- fault flags of the carried multiplex ------------------------------------------------------------------------------------------------------
POISONED_IDS = {"outside_cif": [40], "mux_overflow": list(range(50, 59)), "eep_option": [41]}
FAULT_TF, FAULT_NTF = 17, 24


@functools.lru_cache(maxsize=None)
def _fault_twins():
    """Three clean preset-1 captures (ids 1, 2, 5, 9) and the oracle's frames; the poisons go into copies of the middle one."""
    cfgs = [dab.synth_preset(1, seed=8300 + i, cif_count0=111 * i + 7, skip_samples=(0, 60001, 0)[i]) for i in range(3)]
    caps = [_frozen(dab.synth_generate(c, FAULT_NTF)) for c in cfgs]
    wants = [_frozen(ol.or_replay(iq)[0]) for iq in caps]
    return caps, wants


@pytest.mark.parametrize("kind", sorted(POISONS))
def test_fault_flags_describe_the_carried_multiplex(kind):
    patch, flag = POISONS[kind]
    caps, wants = _fault_twins()
    clean_cfg = dab.synth_preset(1, seed=8301, cif_count0=118, skip_samples=60001)
    bad_cfg = dab.synth_preset(1, seed=8301, cif_count0=118, skip_samples=60001)
    bad_cfg.set_fib_patch(patch, from_cif=4 * FAULT_TF)              # un-assemblable from TF 17 on, after the first frames have left
    assert np.array_equal(dab.synth_generate(clean_cfg, FAULT_NTF), caps[1])
    batch = [caps[0], dab.synth_generate(bad_cfg, FAULT_NTF), caps[2]]
    eng = dab.Engine(0)
    eng.decode(batch)
    silent_after = eng.eti_count(1)
    assert eng.stream_status(1) == flag and 0 < silent_after < len(wants[1])
    assert np.array_equal(eng.eti(1), wants[1][:silent_after])
    # the poisoned id is listed: flags and silence of the unfiltered decode
    ids = [1] + POISONED_IDS[kind]
    eng.set_subchannels(ids)
    eng.decode(batch)
    assert [eng.stream_status(b) for b in range(3)] == [0, flag, 0]
    _assert_equal(eng.eti(1), fm.filter_frames(wants[1], ids)[:silent_after], "poisoned id listed")
    for b in (0, 2):
        _assert_equal(eng.eti(b), fm.filter_frames(wants[b], ids), "neighbour %d, poisoned id listed" % b)
    # only healthy ids are listed: layout_fault sees the carried list alone -- no flag, frames to the end, the poisoned FIC passed on
    ids = [1, 9]
    eng.set_subchannels(ids)
    assert eng.decode(batch) == sum(len(w) for w in wants)
    assert [eng.stream_status(b) for b in range(3)] == [0, 0, 0]
    twin = fm.filter_frames(wants[1], ids)
    fic0 = eti_check.parse(wants[1][0])["fic"]
    cif0 = next(c for c in range(4 * FAULT_NTF) if np.array_equal(dab.synth_fibs(clean_cfg, c), fic0))      # the logical CIF of the first frame
    exp = np.array([fm.with_fic(f, dab.synth_fibs(bad_cfg, cif0 + k)) for k, f in enumerate(twin)])
    changed = sum(1 for f, g in zip(twin, exp) if not np.array_equal(f, g))
    assert 4 <= changed == len(twin) - (4 * FAULT_TF - cif0), (changed, cif0)                            # the frames of TF 17 on carry the patched FIB
    _assert_equal(eng.eti(1), exp, "healthy ids listed")
    for b in (0, 2):
        _assert_equal(eng.eti(b), fm.filter_frames(wants[b], ids), "neighbour %d, healthy ids listed" % b)
    # the same through a session
    st = dab.Stream(3, subchannels=ids)
    got = _feed_odd(st, batch)
    assert [st.status(b) for b in range(3)] == [0, 0, 0]
    _assert_equal(got[1], exp, "session, healthy ids listed")
    st.close()
    eng.close()


# ---- behind the decoder --------------------------------------------------------------------------------------------------------------------------
def test_stages_behind_the_decoder_take_filtered_device_frames():
    """DAB+ slots and a TS slot in preset 0: the filtered device frames (the sub-channels sit at other offsets) give DabPlus and Ts what the
    unfiltered ones give."""
    cfg = dab.synth_preset(0, seed=7320, cif_count0=4980)
    cfg.dabplus_slots = (1 << 1) | (1 << 6)                 # SubChIds 2 and 7
    cfg.dabplus_phase = 3
    cfg.ts_slots = 1 << 5                                   # SubChId 6
    cfg.ts_phase = 777
    plus_ids, ts_ids = [cfg.sub[1].id, cfg.sub[6].id], [cfg.sub[5].id]
    assert plus_ids == [2, 7] and ts_ids == [6]
    iq = dab.synth_generate(cfg, 26)
    want = ol.or_replay(iq)[0]
    import dabplus_model
    assert all(len(dabplus_model.stage(dabplus_model.SyncModel(i), list(want))) >= 6 for i in plus_ids)         # there are superframes to find
    buf = dab.DeviceBuffer(iq.size)
    try:
        buf.upload(iq)
        eng = dab.Engine(0)
        seen = []
        for ids in ([], plus_ids + ts_ids):
            eng.set_subchannels(ids)
            assert eng.decode_device([buf.ptr], [iq.size]) == len(want)
            _assert_equal(eng.eti(0), fm.filter_frames(want, ids), "device decode, filter %s" % ids)
            ptr, total = eng.eti_device_ptr()
            assert total == len(want)
            dp, ts = dab.DabPlus(1, plus_ids), dab.Ts(1, ts_ids)
            assert dp.push((ptr, [total])) >= 2 * 6 and ts.push((ptr, [total])) > 0         # superframes and TS packets were found at all
            seen.append(([(dp.superframes(0, q).tobytes(), dp.data(0, q).tobytes(), dp.stats(0, q).tolist()) for q in range(2)],
                         (ts.records(0, 0).tobytes(), ts.data(0, 0).tobytes(), ts.stats(0, 0).tolist())))
            dp.close()
            ts.close()
        assert seen[1] == seen[0]
        eng.close()
    finally:
        buf.free()


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------------------
def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def test_cli_subch(tmp_path):
    here = os.path.dirname(dab.LIB_PATH)
    exe = os.path.join(here, "dab2eti-hip")
    iq, _ = _capture("preset0")
    cap = tmp_path / "cap.cu8"
    iq.tofile(cap)
    want = _expected("preset0", (5, 9)).tobytes()
    for args in (["--subch", "5,9"], ["--stream", "--subch", "5,9"]):
        r = _run([exe] + args + [str(cap)])
        assert r.returncode == 0, r.stderr
        assert r.stdout == want, args
    r = _run([exe, "--subch", "5,x", str(cap)])
    assert r.returncode == 1 and r.stdout == b"" and b"dab2eti-hip: bad --subch list\n" in r.stderr


def test_cli_subch_pipe_into_eti2aac(tmp_path):
    here = os.path.dirname(dab.LIB_PATH)
    cfg = dab.synth_preset(0, seed=7321, cif_count0=4990)
    cfg.dabplus_slots = (1 << cfg.nsub) - 1
    cfg.dabplus_phase = 2
    cap = tmp_path / "cap.cu8"
    dab.synth_generate(cfg, 26).tofile(cap)
    scid = cfg.sub[5].id
    cmd = "set -o pipefail; '%s' %s '%s' | '%s' %d" % (os.path.join(here, "dab2eti-hip"), "%s", cap, os.path.join(here, "eti2aac"), scid)
    plain = _run(["bash", "-c", cmd % ""])
    only = _run(["bash", "-c", cmd % ("--subch %d" % scid)])
    assert plain.returncode == 0 and only.returncode == 0, (plain.stderr, only.stderr)
    assert len(plain.stdout) > 1000 and only.stdout == plain.stdout
