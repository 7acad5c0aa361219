"""The DAB+ kernels (k_dabplus.hip through DabPlus.push) on the crafted classes of dabplus_cases.py -- Reed-Solomon words at the decoder's
edges, superframes at the AU kernel's slice borders and layout refusals, ETI frames at the locate kernel's refusals -- whose expected results
come from their construction or from the independent decoder of rs_reference.py; on more than 1024 lanes with different content in every
lane; and on every way frames arrive (host, device, device at an odd address).  Everything is bit-exact."""
import time

import numpy as np
import pytest

import dabplus_cases as cs
import dabplus_model as m
import dabtools_amd as dab
from conftest import fresh_seed
from test_gpu_dabplus import _assert_lane_equal, _gpu_lane, _model_stats, _run

pytestmark = pytest.mark.gpu

RS = cs.rs_cases()


def _want(fct, s, data, fixed, failed):
    r = m.parse(data)
    r.update(fct=fct % 250, s=s, rs_corrected=fixed, rs_failed=failed, data=np.asarray(data, np.uint8))
    return r


@pytest.mark.parametrize("cls", sorted(RS))
def test_rs_class_through_the_stage(cls):
    """Codewords 11..71 of superframes of rate 72 carry the class's words; codewords 0..10 (the raw fire code) stay clean, so every superframe
    built must come out."""
    cases = RS[cls]
    assert len(cases) > 0
    lane = cs.rs_lane({cls: cases})
    assert sum(n for _, n, _, _, _, _ in lane) == len(cases)
    frames = cs.frames_of(17, [(5, [sf for _, _, sf, _, _, _ in lane])])
    want = [_want(17 + 5 * i, 72, data, fixed, failed) for i, (_, _, _, data, fixed, failed) in enumerate(lane)]
    dp = dab.DabPlus(1, [5])
    ctx = (cls, len(cases))
    assert dp.push([np.array(frames)]) == len(lane), ctx
    recs, data, aus = _gpu_lane(dp, 0, 0)
    assert len(recs) == len(lane), ctx
    at = 0
    for rec, (_, ncase, sf, wdata, fixed, failed) in zip(recs, lane):     # word by word first: a wrong word is named
        got = data[at:at + 7920].reshape(110, 72)
        for i in range(ncase):
            assert (got[:, 11 + i] == wdata.reshape(110, 72)[:, 11 + i]).all(), (ctx, cases[at // 7920 * 61 + i].label)
        if cls == "d":
            assert rec["rs_corrected"] == 5 * ncase and rec["rs_failed"] == 0, ctx
        if cls == "e":
            assert rec["rs_failed"] == ncase and rec["rs_corrected"] == 0 and (data[at:at + 7920] == sf[:7920]).all(), ctx
        at += 7920
    _assert_lane_equal(recs, data, aus, want, ctx)
    assert list(dp.stats(0, 0)) == _model_stats(want, 0), ctx
    dp.close()


def _superframe_streams(s, seed, classes=None):
    """One stream per (dac_rate, sbr_flag) with every superframe case of rate s -> (streams, per-stream cases)."""
    rng = np.random.default_rng(seed)
    streams, built = [], []
    for dac, sbr in cs.LAYOUTS:
        by_class = cs.superframe_cases(rng, s, dac, sbr)
        cases = [(cls,) + c for cls in ("au3", "slice", "flip", "layout", "fire") if classes is None or cls in classes for c in by_class[cls]]
        assert cases and cases[0][0] != "fire"                           # the bad raw fire code never comes first, and only once: sync holds
        sfs = cs.protect_many([data for _, _, data, _ in cases])
        streams.append(cs.frames_of(31 * s + dac, [(5, sfs)]))
        built.append(cases)
    return streams, built


def _check_superframe_streams(dp, streams, built, first, ctx):
    for b, cases in enumerate(built):
        recs, data, aus = _gpu_lane(dp, first + b, 0)
        assert len(recs) == len(cases), (ctx, b, len(recs), len(cases))
        s = len(cases[0][2]) // 110
        for rec, (cls, label, _, exp) in zip(recs, cases):               # against the construction: a wrong record is named
            for f in exp:
                got = list(rec[f]) if f in ("au_start", "au_len") else int(rec[f])
                assert got == exp[f], (ctx, b, cls, label, f, got, exp[f])
        want = [_want(int(streams[b][0][4]) + 5 * i, s, c[2], 0, 0) for i, c in enumerate(cases)]
        _assert_lane_equal(recs, data, aus, want, (ctx, b))
        assert list(dp.stats(first + b, 0)) == _model_stats(want, 0), (ctx, b)


@pytest.mark.parametrize("s", cs.RATES)
def test_superframe_classes_through_the_stage(s):
    streams, built = _superframe_streams(s, 900 + s)
    counts = {}
    for cases in built:
        for c in cases:
            counts[c[0]] = counts.get(c[0], 0) + 1
    assert set(counts) == {"au3", "slice", "flip", "layout", "fire"}, counts
    dp = dab.DabPlus(len(streams), [5])
    assert dp.push([np.array(f) for f in streams]) == sum(len(c) for c in built), (s, counts)
    _check_superframe_streams(dp, streams, built, 0, (s, counts))
    dp.close()


def test_full_lds_buffer_of_the_au_kernel():
    """Rate 72 behind 9 codewords of rate 1: every superframe's bytes start 14 past a 16-byte boundary, which fills the AU kernel's LDS copy to
    its last vector (the start is 110 times a codeword number, so 14 is the largest offset there is)."""
    rng = np.random.default_rng(12)
    head = cs.plain_superframes(rng, 1, 9)
    streams, built = _superframe_streams(72, 1972, classes=("au3", "slice", "flip"))
    assert (110 * len(head)) % 16 == 14 and (110 * 72) % 16 == 0
    first = cs.frames_of(3, [(5, cs.protect_many(head))])
    dp = dab.DabPlus(1 + len(streams), [5])
    assert dp.push([np.array(first)] + [np.array(f) for f in streams]) == len(head) + sum(len(c) for c in built)
    recs, data, aus = _gpu_lane(dp, 0, 0)
    _assert_lane_equal(recs, data, aus, [_want(3 + 5 * i, 1, d, 0, 0) for i, d in enumerate(head)], "rate 1")
    _check_superframe_streams(dp, streams, built, 1, "lead 14")
    dp.close()


def test_frame_classes_through_the_stage():
    cases = cs.frame_cases()
    assert len(cases) >= 18
    streams = [list(c[1]) for c in cases]
    want, losses = {}, {}
    for b, case in enumerate(cases):
        for q, scid in enumerate(cs.FRAME_IDS):
            sm = m.SyncModel(scid)
            want[b, q] = m.stage(sm, case[1])
            losses[b, q] = sm.losses
            assert len(want[b, q]) == case[2][scid] and sm.losses == case[3][scid], (case[0], scid)
    for chunk in (None, 4):
        dp = dab.DabPlus(len(streams), list(cs.FRAME_IDS))
        got = _run(dp, streams, cs.FRAME_IDS, chunk)
        for (b, q), w in want.items():
            ctx = (len(cases), chunk, cases[b][0], cs.FRAME_IDS[q])
            assert len(got[b, q][0]) == cases[b][2][cs.FRAME_IDS[q]], ctx
            _assert_lane_equal(*got[b, q], w, ctx)
            assert list(dp.stats(b, q)) == _model_stats(w, losses[b, q]), ctx
        dp.close()


# ---- many lanes -----------------------------------------------------------------------------------------------------------------------------
def _scale_case(rng, nstreams, ids, max_frames):
    """Streams with different frame counts (none, fewer than 5, many) and start phases, different content and a few dirty codewords in every
    lane -> (streams, {(stream, sub): records the stage must give}, {(stream, sub): sync losses})."""
    nq = len(ids)
    plan, datas = [], []
    for b in range(nstreams):
        count = (0, int(rng.integers(1, 5)))[b % 8] if b % 8 < 2 else int(rng.integers(10, max_frames + 1))
        phase = int(rng.integers(5))
        nsf = -(-(phase + count) // 5) if count else 0
        rates = [1 + (b + q) % 3 for q in range(nq)]
        plan.append((count, phase, nsf, rates, int(rng.integers(250))))
        for s in rates:
            datas += cs.plain_superframes(rng, s, nsf)
    prot = cs.protect_many(datas) if datas else []
    streams, at = [], 0
    for count, phase, nsf, rates, fct0 in plan:
        subs = []
        for q, s in enumerate(rates):
            sfs = prot[at:at + nsf]
            at += nsf
            for _ in range(2 if nsf else 0):                             # dirty codewords, off the raw fire code's bytes (rows 0..10)
                grid = sfs[int(rng.integers(nsf))].reshape(120, s)
                ne = int(rng.integers(1, 8))
                grid[11 + rng.choice(109, ne, replace=False), int(rng.integers(s))] ^= rng.integers(1, 256, ne).astype(np.uint8)
            subs.append((ids[q], sfs))
        streams.append(cs.frames_of(fct0, subs, phase, count) if count else [])
    raws, owners, losses = [], [], {}
    for b, frames in enumerate(streams):
        for q, scid in enumerate(ids):
            sm = m.SyncModel(scid)
            for fct, s, raw in sm.push(frames):
                raws.append(raw)
                owners.append((b, q, fct, s))
            losses[b, q] = sm.losses
    want = {(b, q): [] for b in range(nstreams) for q in range(nq)}
    for (b, q, fct, s), (data, fixed, failed) in zip(owners, cs.decode_superframes(raws)):
        want[b, q].append(_want(fct, s, data, fixed, failed))
    return streams, want, losses


@pytest.mark.parametrize("nstreams,nids,max_frames", [(256, 4, 40), (205, 5, 40), (256, 12, 40), (17, 64, 40)])
def test_every_lane_beyond_1024_lanes(nstreams, nids, max_frames):
    name = "test_every_lane_beyond_1024_lanes[%d-%d]" % (nstreams, nids)
    seed = fresh_seed(name)
    rng = np.random.default_rng(seed)
    ids = [int(i) for i in np.sort(rng.choice(64, nids, replace=False))]
    t0 = time.time()
    streams, want, losses = _scale_case(rng, nstreams, ids, max_frames)
    t1 = time.time()
    nlanes = nstreams * nids
    assert nlanes >= 1024 and len(want) == nlanes
    nsf = sum(len(w) for w in want.values())
    empty = sum(1 for w in want.values() if not w)
    fixed = sum(r["rs_corrected"] for w in want.values() for r in w)
    failed = sum(r["rs_failed"] for w in want.values() for r in w)
    assert nsf > nlanes and empty >= nlanes // 8 and fixed > 0 and failed > 0, (seed, nsf, empty, fixed, failed)
    for chunk in (None, 7):
        dp = dab.DabPlus(nstreams, ids)
        got = _run(dp, streams, ids, chunk)
        for key, w in want.items():                                      # every lane
            _assert_lane_equal(*got[key], w, (seed, nlanes, chunk, key))
            assert list(dp.stats(*key)) == _model_stats(w, losses[key]), (seed, nlanes, chunk, key)
        dp.close()
    print("%s: %d lanes, %d superframes; CPU side %.1f s to build and expect, %.1f s to push and compare" % (name, nlanes, nsf, t1 - t0, time.time() - t1))


# ---- the ways frames arrive ----------------------------------------------------------------------------------------------------------------
def _push_chunks(dp, streams, ids, chunk, how):
    """As test_gpu_dabplus._run, with the frames of each push in host memory ("host"), in device memory at an allocation's base ("device") or one
    byte above it ("device+1")."""
    got = {(b, q): ([], [], []) for b in range(len(streams)) for q in range(len(ids))}
    for a in range(0, max(len(f) for f in streams), chunk):
        parts = [f[a:a + chunk] for f in streams]
        counts = [len(p) for p in parts]
        flat = np.concatenate([np.asarray(f, np.uint8).reshape(-1) for p in parts for f in p]) if sum(counts) else np.zeros(0, np.uint8)
        buf = None
        if how == "host":
            dp.push(flat, counts)
        else:
            off = 1 if how == "device+1" else 0
            buf = dab.DeviceBuffer(flat.size + 16)
            assert buf.ptr % 16 == 0
            buf.upload(np.concatenate([np.zeros(off, np.uint8), flat]))
            dp.push((buf.ptr + off, counts))
        for key, (r, d, u) in got.items():
            rr, dd, uu = _gpu_lane(dp, *key)
            r.append(rr)
            d.append(dd)
            u += uu
        if buf is not None:
            buf.free()
    return {k: (np.concatenate(r), np.concatenate(d), u) for k, (r, d, u) in got.items()}


def test_host_device_and_unaligned_device_frames_give_the_same():
    seed = fresh_seed("test_host_device_and_unaligned_device_frames_give_the_same")
    rng = np.random.default_rng(seed)
    ids = [5, 9]
    streams = []
    for b, count in enumerate((23, 0, 12, 31, 4, 17, 1, 2, 3, 8)):
        phase = b % 5
        nsf = -(-(phase + count) // 5)
        subs = []
        for scid, s in zip(ids, (2 + b % 2, 3)):
            sfs = cs.protect_many(cs.plain_superframes(rng, s, nsf)) if nsf else []
            for sf in sfs:
                grid = sf.reshape(120, s)
                ne = int(rng.integers(0, 8))
                grid[rng.choice(120, ne, replace=False), int(rng.integers(s))] ^= rng.integers(1, 256, ne).astype(np.uint8)
            subs.append((scid, sfs))
        streams.append(cs.frames_of(40 * b, subs, phase, count) if count else [])
    assert {min(4, len(f)) for f in streams} == {0, 1, 2, 3, 4}          # every number of carried frames after the first push
    want, losses = {}, {}
    for b, frames in enumerate(streams):
        for q, scid in enumerate(ids):
            sm = m.SyncModel(scid)
            want[b, q] = m.stage(sm, frames)
            losses[b, q] = sm.losses
    assert sum(len(w) for w in want.values()) >= 20
    results = {}
    for chunk in (7, 9):
        for how in ("host", "device", "device+1"):
            dp = dab.DabPlus(len(streams), ids)
            got = _push_chunks(dp, streams, ids, chunk, how)
            for key, w in want.items():
                _assert_lane_equal(*got[key], w, (seed, chunk, how, key))
                assert list(dp.stats(*key)) == _model_stats(w, losses[key]), (seed, chunk, how, key)
            results[chunk, how] = {k: (r.tobytes(), d.tobytes(), u) for k, (r, d, u) in got.items()}
            dp.close()
    first = results[7, "host"]
    assert all(v == first for v in results.values())
