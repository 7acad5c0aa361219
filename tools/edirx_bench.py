"""Cost of the EDI receiving stage (dabhip_edirx_push) at full batch, beside the decode step of the same rounds: 256 streams x 256 ETI frames of
the preset-0 ensemble as EDI packets, made once by the sending stage (Edi) and resident in device memory.

  python tools/edirx_bench.py [--rounds 3] [--streams 256] [--tf 64] [--reps 5] [--recover 2] [--max-frag 1400] [--depth 4] [--parent-tree DIR] [--out FILE]

Every measurement is a process of its own, and the kinds alternate round by round: the stage on mode-0 packets, on mode-1 fragments, on mode-2
fragments with nothing lost, on mode-2 fragments with two fragments of every frame lost (every code word then has erasures), the decode step
of this build (bench.py, the stage unused) and, with --parent-tree, the decode step of another built checkout (the parent commit's) through
that checkout's own bench.py and binding.  Prints one JSON object with every round's figures, their medians and spreads, the per-stage GPU
times from dabhip_edirx_stage_ms and the ratio to the decode step.

One stream's packets are made by Edi from frames built on the host (as tools/edi_bench.py builds them) and repeated for every stream.  The
timed push is followed by a flush, whose time is reported beside it: with loss the last frame of a stream leaves at the flush only."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"mode0_af": (0, 0), "mode1_pft": (1, 0), "mode2_pft_rs": (2, 0), "mode2_two_lost": (2, 2)}


def child_stage(a, case):
    import dabplus_model as dm
    import dabtools_amd as dab
    import edi_model as em
    import edirx_model as rx
    mode, lost = CASES[case]
    nf = 4 * a.tf
    cfg = dab.synth_preset(0, seed=1)
    ids = [cfg.sub[k].id for k in range(cfg.nsub)]
    one = np.stack([dm.eti_frame(c % 250, [(ids[k], dab.synth_payload(cfg, c, k)) for k in range(cfg.nsub)]) for c in range(nf)])
    one[:, 6] = ((np.arange(nf) % 8) << 5) | (1 << 3)                     # FP, MID = 1
    edi = dab.Edi(1, mode, a.recover, a.max_frag)
    edi.push(one)
    data, recs = edi.data(0), edi.records(0)
    edi.close()
    keep = np.ones(recs.size, bool)
    if lost:
        keep = (recs["findex"] != 1) & (recs["findex"] != recs["fcount"] - 1)
    lengths = recs["length"][keep].astype(np.int32)
    stream = np.concatenate([data[int(r["offset"]):int(r["offset"]) + int(r["length"])] for r in recs[keep]])
    buf = dab.DeviceBuffer(stream.size * a.streams)
    buf.upload(np.tile(stream, a.streams))
    all_lengths = np.tile(lengths, a.streams)
    counts = [lengths.size] * a.streams
    walls, flushes, stages = [], [], []
    for r in range(a.reps + 1):
        erx = dab.EdiRx(a.streams, a.depth)
        erx.push((buf.ptr, all_lengths, counts))                           # the first push allocates; after the flush the same packets come again:
        erx.flush()                                                        # they begin 256 numbers below the window and look like a new stream by the
        for b in range(a.streams):                                         # rule of d >= 32768 only after a reset
            erx.reset(b)
        t = time.perf_counter()
        n = erx.push((buf.ptr, all_lengths, counts))
        w = (time.perf_counter() - t) * 1e3
        st = erx.stage_ms()
        if r == a.reps:                                                    # outside the timed parts: the first frame against the numpy model's rebuild
            same = bool(n > 0 and (erx.frames(a.streams - 1)[0] == rx.rebuild(em.carried(one[0]))).all())
        t = time.perf_counter()
        n += erx.flush()
        fl = (time.perf_counter() - t) * 1e3
        if r:
            walls.append(w)
            flushes.append(fl)
            stages.append(st)
        if r == a.reps:
            stats = np.sum([erx.stats(b) for b in range(0, a.streams, max(1, a.streams // 8))], axis=0)
        erx.close()
    st = {key: float(np.median([x[key] for x in stages])) for key in stages[0]}
    out = {"push_ms_median": float(np.median(walls)), "push_ms_min": float(np.min(walls)), "flush_ms_median": float(np.median(flushes)),
           "gpu_ms_median": float(sum(st.values())), "stage_ms_median": st, "frames_out": int(n), "frames_expected": a.streams * nf, "first_frame_equal": same,
           "packets_per_push": int(all_lengths.size), "bytes_per_push": int(stream.size) * a.streams,
           "counters_of_every_8th_stream": dict(zip(dab.EDIRX_STATS, [int(x) for x in stats]))}
    print(json.dumps(out))


def run_child(args, env=None):
    out = subprocess.run([sys.executable] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=900)
    if out.returncode != 0:
        raise SystemExit("child failed: %s\n%s" % (" ".join(args), out.stderr[-2000:]))
    return json.loads([line for line in out.stdout.splitlines() if line.startswith("{")][-1])


def spread(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values)), "rounds": [float(v) for v in values]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--tf", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--recover", type=int, default=2)
    ap.add_argument("--max-frag", type=int, default=1400)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child is not None:
        return child_stage(a, a.child)
    me = [os.path.abspath(__file__), "--streams", str(a.streams), "--tf", str(a.tf), "--reps", str(a.reps), "--recover", str(a.recover), "--max-frag", str(a.max_frag),
          "--depth", str(a.depth)]
    bench = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup), "--no-cpu-baseline", "--no-variants"]
    rounds = {n: [] for n in tuple(CASES) + ("decode", "decode_parent")}

    def measure(kind, args):
        rounds[kind].append(run_child(args))
        print("round %d: %s done" % (len(rounds[kind]), kind), file=sys.stderr, flush=True)

    for _ in range(a.rounds):
        measure("mode2_two_lost", me + ["--child", "mode2_two_lost"])
        measure("decode", bench)
        measure("mode0_af", me + ["--child", "mode0_af"])
        if a.parent_tree:
            measure("decode_parent", [os.path.join(os.path.abspath(a.parent_tree), "bench.py")] + bench[1:])
        measure("mode2_pft_rs", me + ["--child", "mode2_pft_rs"])
        measure("mode1_pft", me + ["--child", "mode1_pft"])
    result = {"streams": a.streams, "tf_per_stream": a.tf, "rounds": a.rounds, "recover": a.recover, "max_frag": a.max_frag, "depth": a.depth,
              "decode_step_ms": spread([r["ms_per_step"] for r in rounds["decode"]]),
              "decode_step_ms_is": "bench.py --gpus 1 ms_per_step of this build in the same rounds, the EDI receiving stage unused"}
    if a.parent_tree:
        result["decode_step_ms_parent_build"] = spread([r["ms_per_step"] for r in rounds["decode_parent"]])
    step = result["decode_step_ms"]["median"]
    for name in CASES:
        last = rounds[name][-1]
        result[name] = {"push_ms": spread([r["push_ms_median"] for r in rounds[name]]), "flush_ms": spread([r["flush_ms_median"] for r in rounds[name]]),
                        "gpu_ms": spread([r["gpu_ms_median"] for r in rounds[name]]),
                        "stage_ms_median_of_rounds": {k: float(np.median([r["stage_ms_median"][k] for r in rounds[name]])) for k in last["stage_ms_median"]},
                        "packets_per_push": last["packets_per_push"], "bytes_per_push": last["bytes_per_push"], "frames_out": last["frames_out"],
                        "frames_expected": last["frames_expected"], "first_frame_equal": last["first_frame_equal"],
                        "counters_of_every_8th_stream": last["counters_of_every_8th_stream"]}
        result[name]["push_over_decode_step"] = result[name]["push_ms"]["median"] / step
    print(json.dumps(result, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
