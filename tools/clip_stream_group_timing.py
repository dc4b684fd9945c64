"""Times one push of a ClipStreamGroup in steady state (rings full, eval mode, fp32, one process) against the way to
get the same result without a group: one ClipStream per camera, pushed one after the other.  For the three 3-D clip
models -- a2.CausalAnomalyDetector, mc.SimpleVideoAnomalyDetector (grey) and bbox.CausalAnomalyDetector -- at 64 x 64
frames, T = 8, stride 1; for each --streams S every camera brings one frame per push and completes one window.  Two
forms of the push:

  push      fp32 frames on the device
  push_u8   packed BGR camera frames of --source-size in pinned host memory, read in place by the ingest kernel (the
            group: one table-form launch for all cameras; a lone stream: one launch per camera, into its ring slot)

The two paths alternate within every repetition.  Wall-clock time of the host thread from the call to the end of a
device synchronise.  Median (min-max) of --reps after --warmup, whether the two ranges overlap, and the largest absolute
difference between the two paths' scores over the timed pushes.  Writes one JSON file.

    python tools/clip_stream_group_timing.py --out profiles/clip_stream_group_64x64.json \\
        --git-hash $(git rev-parse --short HEAD)
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
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 4, 16, 32])
    ap.add_argument("--models", nargs="+", default=["a2", "mc", "bbox"])
    ap.add_argument("--source-size", type=int, nargs=2, default=[120, 160])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--git-hash", default="unknown")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    from vad_amd.a2 import CausalAnomalyDetector as A2Detector
    from vad_amd.bbox import CausalAnomalyDetector as BboxDetector
    from vad_amd.mc import SimpleVideoAnomalyDetector
    if not torch.cuda.is_available():
        raise SystemExit("clip_stream_group_timing: needs a HIP device (a CPU run gives no time)")
    torch.manual_seed(0)
    T, HW = a.window, 64
    Hs, Ws = a.source_size
    make = {"a2": lambda: (A2Detector().cuda().eval(), 3),
            "mc": lambda: (SimpleVideoAnomalyDetector(input_channels=1, temporal_frames=T).cuda().eval(), 1),
            "bbox": lambda: (BboxDetector(num_frames=T).cuda().eval(), 3)}

    def stats(ms):
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=len(ms))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    res = dict(git=a.git_hash, device=torch.cuda.get_device_name(0), host_cpus=os.cpu_count(), frame=[HW, HW],
               window=T, stride=1, dtype="fp32", frames_per_camera_per_push=1, source_u8=[Hs, Ws, "bgr", "pinned"],
               clock="host wall clock, call to end of synchronize", models={})
    pushes = a.warmup + a.reps
    N = T - 1 + pushes
    for name in a.models:
        m, C = make[name]()
        res["models"][name] = dict(channels=C, push={}, push_u8={})
        for form in ("push", "push_u8"):
            for S in a.streams:
                gen = torch.Generator().manual_seed(S)
                if form == "push":
                    frames = torch.rand(S, N, C, HW, HW, generator=gen).cuda()
                    kw = {}
                else:
                    frames = torch.randint(0, 256, (S, N, Hs, Ws, 3), dtype=torch.uint8, generator=gen).pin_memory()
                    kw = dict(color="bgr")
                group = m.open_stream_group(S, window=T, stride=1, max_push=1, frame_size=(HW, HW))
                singles = [m.open_stream(window=T, stride=1, max_push=1, frame_size=(HW, HW)) for _ in range(S)]
                g_push, s_push = getattr(group, form), [getattr(st, form) for st in singles]
                for f in range(T - 1):  # the rings, one frame short of the first window
                    g_push([frames[s, f:f + 1] for s in range(S)], **kw)
                    for s in range(S):
                        s_push[s](frames[s, f:f + 1], **kw)
                g_ms, s_ms, worst = [], [], 0.0
                for i in range(pushes):
                    f = T - 1 + i
                    chunk = [frames[s, f:f + 1] for s in range(S)]
                    tg, og = timed(lambda: g_push(chunk, **kw))
                    ts, os_ = timed(lambda: [s_push[s](chunk[s], **kw) for s in range(S)])
                    assert all(o["anomaly_scores"].shape == (1,) for o in og + os_), "steady state: a window per camera"
                    if i >= a.warmup:
                        g_ms.append(tg)
                        s_ms.append(ts)
                        gs = torch.cat([o["anomaly_scores"] for o in og])
                        ss = torch.cat([o["anomaly_scores"] for o in os_])
                        worst = max(worst, float((gs - ss).abs().max()))
                r = dict(cameras=S, ring_frames_per_camera=group.cap, group=stats(g_ms),
                         sequential_streams=stats(s_ms), max_abs_score_diff=worst)
                r["speedup"] = r["sequential_streams"]["median_ms"] / r["group"]["median_ms"]
                r["ranges_overlap"] = not (r["group"]["max_ms"] < r["sequential_streams"]["min_ms"]
                                           or r["sequential_streams"]["max_ms"] < r["group"]["min_ms"])
                r["group_ms_per_camera"] = r["group"]["median_ms"] / S
                res["models"][name][form][str(S)] = r
                print(json.dumps({name: {form: {str(S): r}}}), flush=True)
                torch.cuda.synchronize()
                del frames, group, singles, g_push, s_push
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
