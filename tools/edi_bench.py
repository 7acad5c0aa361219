"""Cost of the EDI stage (dabhip_edi_push) at full batch, beside the decode step of the same run: 256 streams x 64 TF (256 ETI frames each) of the
preset-0 ensemble, resident in device memory as Engine.eti_device_ptr leaves them, in each of the three modes.

  python tools/edi_bench.py [--rounds 3] [--streams 256] [--tf 64] [--reps 10] [--recover 2] [--max-frag 1400] [--parent-tree DIR] [--out FILE]

Every measurement is a process of its own, and the kinds alternate round by round: the stage in mode 0, 1 and 2, the decode step of this build
(bench.py, the stage unused) and, with --parent-tree, the decode step of another built checkout (the parent commit's) through that checkout's own
bench.py and binding.  Prints one JSON object with every round's figures, their medians and spreads, the per-stage GPU times from
dabhip_edi_stage_ms, the ratio to the decode step, and beside the rs kernel's time what its LDS reads and its byte traffic would allow.

The frames are built on the host from the synthetic modulator's payloads (one ensemble, its 256 frames repeated for every stream), so the stage's
processes need no IQ and no decode."""
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

LDS_READ_TBPS = 150.0        # ds_read_b128 with every CU streaming
HBM_TBPS = 6.29              # measured copy rate


def child_stage(a, mode):
    import dabplus_model as dm
    import dabtools_amd as dab
    import edi_model as em
    nf = 4 * a.tf
    cfg = dab.synth_preset(0, seed=1)
    ids = [cfg.sub[k].id for k in range(cfg.nsub)]
    one = np.stack([dm.eti_frame(c % 250, [(ids[k], dab.synth_payload(cfg, c, k)) for k in range(cfg.nsub)]) for c in range(nf)])
    one[:, 6] = ((np.arange(nf) % 8) << 5) | (1 << 3)                     # FP, MID = 1
    assert all(em.accepted(f) is not None for f in one)
    l = len(em.af_body(one[0], 0, 0)) + 2
    c, k, z, B, f, s = em.plan(l, mode, a.recover, a.max_frag)
    frames = np.tile(one, (a.streams, 1))
    buf = dab.DeviceBuffer(frames.size)
    buf.upload(frames)
    counts = [nf] * a.streams
    walls, stages = [], []
    for r in range(a.reps + 1):
        edi = dab.Edi(a.streams, mode, a.recover, a.max_frag)
        edi.push((buf.ptr, counts))                                       # the first push allocates; the timed one goes on with the same frames again
        t = time.perf_counter()
        npk = edi.push((buf.ptr, counts))
        w = (time.perf_counter() - t) * 1e3
        if r:
            walls.append(w)
            stages.append(edi.stage_ms())
        if r == a.reps:
            stats = np.sum([edi.stats(b) for b in range(0, a.streams, max(1, a.streams // 8))], axis=0)
        edi.close()
    st = {key: float(np.median([x[key] for x in stages])) for key in stages[0]}
    nframes = a.streams * nf
    out = {"push_ms_median": float(np.median(walls)), "push_ms_min": float(np.min(walls)), "gpu_ms_median": float(sum(st.values())), "stage_ms_median": st,
           "packets_per_push": int(npk), "af_packet_bytes": l, "sizes": dict(zip("ckzBfs", (c, k, z, B, f, s))), "frames": nframes,
           "frame_bytes_in": nframes * 6144, "counters_of_every_8th_stream": dict(zip(dab.EDI_STATS, [int(x) for x in stats]))}
    if mode == 2:
        # per chunk the rs kernel reads 207 rows of 48 bytes and k message bytes from LDS; per frame it moves c k bytes in and 48 c out,
        # and every workgroup loads the 12 KB table once (2048 workgroups at most)
        lds = nframes * c * 207 * 48 + nframes * c * k
        mem = nframes * (c * k + 48 * c) + min(2048, (nframes + 3) // 4) * 12288
        out["rs"] = {"ms": st["rs"], "lds_read_bytes": lds, "lds_floor_ms": lds / (LDS_READ_TBPS * 1e9), "memory_bytes": mem, "memory_floor_ms": mem / (HBM_TBPS * 1e9),
                     "lds_rate_assumed_TBps": LDS_READ_TBPS, "memory_rate_assumed_TBps": HBM_TBPS, "gf256_multiply_adds": nframes * c * 207 * 48}
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--recover", type=int, default=2)
    ap.add_argument("--max-frag", type=int, default=1400)
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child is not None:
        return child_stage(a, int(a.child))
    me = [os.path.abspath(__file__), "--streams", str(a.streams), "--tf", str(a.tf), "--reps", str(a.reps), "--recover", str(a.recover), "--max-frag", str(a.max_frag)]
    bench = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup), "--no-cpu-baseline", "--no-variants"]
    names = ("mode0_af", "mode1_pft", "mode2_pft_rs")
    rounds = {n: [] for n in names + ("decode", "decode_parent")}

    def measure(kind, args):
        rounds[kind].append(run_child(args))
        print("round %d: %s done" % (len(rounds[kind]), kind), file=sys.stderr, flush=True)

    for _ in range(a.rounds):
        measure("mode2_pft_rs", me + ["--child", "2"])
        measure("decode", bench)
        measure("mode0_af", me + ["--child", "0"])
        if a.parent_tree:
            measure("decode_parent", [os.path.join(os.path.abspath(a.parent_tree), "bench.py")] + bench[1:])
        measure("mode1_pft", me + ["--child", "1"])
    result = {"streams": a.streams, "tf_per_stream": a.tf, "rounds": a.rounds, "recover": a.recover, "max_frag": a.max_frag,
              "decode_step_ms": spread([r["ms_per_step"] for r in rounds["decode"]]),
              "decode_step_ms_is": "bench.py --gpus 1 ms_per_step of this build in the same rounds, the EDI stage unused"}
    if a.parent_tree:
        result["decode_step_ms_parent_build"] = spread([r["ms_per_step"] for r in rounds["decode_parent"]])
    step = result["decode_step_ms"]["median"]
    for name in names:
        last = rounds[name][-1]
        result[name] = {"push_ms": spread([r["push_ms_median"] for r in rounds[name]]), "gpu_ms": spread([r["gpu_ms_median"] for r in rounds[name]]),
                        "stage_ms_median_of_rounds": {k: float(np.median([r["stage_ms_median"][k] for r in rounds[name]])) for k in last["stage_ms_median"]},
                        "packets_per_push": last["packets_per_push"], "af_packet_bytes": last["af_packet_bytes"], "sizes": last["sizes"], "frames": last["frames"],
                        "frame_bytes_in": last["frame_bytes_in"], "counters_of_every_8th_stream": last["counters_of_every_8th_stream"]}
        result[name]["push_over_decode_step"] = result[name]["push_ms"]["median"] / step
    rs = dict(rounds["mode2_pft_rs"][-1]["rs"])
    rs["ms"] = spread([r["rs"]["ms"] for r in rounds["mode2_pft_rs"]])
    result["rs_kernel"] = rs
    print(json.dumps(result, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
