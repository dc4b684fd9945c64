"""Times one push of raw camera frames in steady state (rings full, eval mode, fp32, one process): u8 frames at the
camera's size in pinned host memory, one frame per camera per push, --streams S cameras in a stream group, for
CausalAnomalyDetector (target --height x --width) and the memory autoencoder (64x64).  Four legs, run one after the
other within every repetition, each on a group of its own:

  push_u8      group.push_u8 on the pinned u8 frames (one table-form ingest launch, then push's body)
  host_route   what the package offered before push_u8: data.resize_u8 per frame on the host, the numpy normalise,
               .to(device) per camera, then group.push
  push_u8_hbm  group.push_u8 on the same u8 frames already in HBM
  push_hbm     group.push on fp32 frames already resized, normalised and in HBM (push_u8_hbm - push_hbm is the price
               of the ingest launch itself)

Wall-clock time of the host thread from the call to the end of a device synchronise (the host route's cost is host
work, which device events would not see).  Median (min-max) of --reps after --warmup.  Also the largest absolute
difference between push_u8's and the host route's scores, which must be 0.  Writes one JSON file.

    python tools/ingest_timing.py --out profiles/ingest_u8_240x360.json --git-hash $(git rev-parse --short HEAD)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src-height", type=int, default=360)
    ap.add_argument("--src-width", type=int, default=640)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=360)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 4, 16, 32])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--git-hash", default="unknown")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import numpy as np
    import torch
    from vad_amd import data
    from vad_amd.ae import VideoAutoEncoder
    from vad_amd.cad import CausalAnomalyDetector
    if not torch.cuda.is_available():
        raise SystemExit("ingest_timing: needs a HIP device (a CPU run gives no time)")
    torch.manual_seed(0)
    T, Hs, Ws = a.window, a.src_height, a.src_width
    f32 = np.float32
    models = {
        "cad": (CausalAnomalyDetector().cuda().eval(), (a.height, a.width), 0, dict(frame_size=(a.height, a.width)),
                lambda u: (u.astype(f32) - f32(0.5)) / f32(0.5)),
        "ae": (VideoAutoEncoder().cuda().eval(), (64, 64), 2, {},
               lambda u: np.clip(u.astype(f32) / f32(255), f32(0.001), f32(0.999))),
    }

    def stats(ms):
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=len(ms))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    res = dict(git=a.git_hash, device=torch.cuda.get_device_name(0), host_cpus=os.cpu_count(), source=[Hs, Ws],
               source_memory="pinned host, uint8", window=T, stride=1, dtype="fp32", frames_per_camera_per_push=1,
               clock="host wall clock, call to end of synchronize", models={})
    pushes = a.warmup + a.reps
    NF = 4  # distinct frames per camera, pushed in turn
    for name, (m, size, mode, kw, norm) in models.items():
        res["models"][name] = dict(target=list(size), mode=mode, streams={})
        for S in a.streams:
            rng = np.random.default_rng(S)
            u8 = torch.from_numpy(rng.integers(0, 256, (S, NF, Hs, Ws), dtype=np.uint8)).pin_memory()
            u8_np = u8.numpy()
            u8_dev = u8.cuda()
            f32_dev = torch.stack([data.ingest_u8(u8_dev[s], size, mode) for s in range(S)])

            def host_route(f):
                return [torch.from_numpy(norm(data.resize_u8(u8_np[s, f], *size))[None, None]).to("cuda")
                        for s in range(S)]

            legs = {
                "push_u8": lambda g, f: g.push_u8([u8[s, f:f + 1] for s in range(S)]),
                "host_route": lambda g, f: g.push(host_route(f)),
                "push_u8_hbm": lambda g, f: g.push_u8([u8_dev[s, f:f + 1] for s in range(S)]),
                "push_hbm": lambda g, f: g.push([f32_dev[s, f:f + 1] for s in range(S)]),
            }
            groups = {k: m.open_stream_group(S, window=T, stride=1, max_push=1, **kw) for k in legs}
            for i in range(T - 1):  # the rings, one frame short of the first window
                for k, fn in legs.items():
                    fn(groups[k], i % NF)
            ms, worst = {k: [] for k in legs}, 0.0
            for i in range(pushes):
                f = (T - 1 + i) % NF
                outs = {}
                for k, fn in legs.items():
                    t, outs[k] = timed(lambda: fn(groups[k], f))
                    if i >= a.warmup:
                        ms[k].append(t)
                assert all(o["anomaly_scores"].shape == (1,) for v in outs.values() for o in v), "steady state"
                sc = {k: torch.cat([o["anomaly_scores"] for o in v]) for k, v in outs.items()}
                worst = max(worst, float((sc["push_u8"] - sc["host_route"]).abs().max()))
            r = {k: stats(v) for k, v in ms.items()}
            r["cameras"] = S
            r["max_abs_score_diff_push_u8_vs_host_route"] = worst
            r["speedup_push_u8_over_host_route"] = r["host_route"]["median_ms"] / r["push_u8"]["median_ms"]
            r["push_u8_max_below_host_route_min"] = r["push_u8"]["max_ms"] < r["host_route"]["min_ms"]
            r["ingest_launch_ms"] = r["push_u8_hbm"]["median_ms"] - r["push_hbm"]["median_ms"]
            res["models"][name]["streams"][str(S)] = r
            print(json.dumps({name: {str(S): r}}), flush=True)
            del groups, u8, u8_dev, f32_dev
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
