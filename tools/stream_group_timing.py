"""Times one push of a CausalAnomalyDetector stream group in steady state (rings full, eval mode, fp32, one process)
against the way to get the same result without a group: one CadStream per camera, pushed one after the other.  For each
--streams S every camera brings one frame per push and completes one window (stride 1).  Device events around every
group push, and around each run of S CadStream pushes (one event pair for the S of them); both enclose their host
reads (nmax / counts).  Median (min-max) of --reps after --warmup, the method of tools/stream_timing.py.  Also the
largest absolute difference between the two paths' scores over the timed pushes.  Writes one JSON file.

    python tools/stream_group_timing.py --out profiles/stream_group_240x360.json --git-hash $(git rev-parse --short HEAD)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=360)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 4, 16, 32])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--git-hash", default="unknown")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    from vad_amd.cad import CausalAnomalyDetector
    if not torch.cuda.is_available():
        raise SystemExit("stream_group_timing: needs a HIP device (a CPU run gives no time)")
    torch.manual_seed(0)
    m = CausalAnomalyDetector().cuda().eval()
    T, H, W = a.window, a.height, a.width

    def stats(ms):
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=len(ms))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    res = dict(git=a.git_hash, device=torch.cuda.get_device_name(0), height=H, width=W, window=T, stride=1,
               dtype="fp32", frames_per_camera_per_push=1, streams={})
    pushes = a.warmup + a.reps
    N = T - 1 + pushes
    for S in a.streams:
        gen = torch.Generator(device="cuda").manual_seed(1)
        frames = torch.rand(S, N, 1, H, W, device="cuda", generator=gen) * 2 - 1
        group = m.open_stream_group(S, window=T, stride=1, max_push=1)
        singles = [m.open_stream(window=T, stride=1, max_push=1) for _ in range(S)]
        for f in range(T - 1):  # the rings, one frame short of the first window
            group.push([frames[s, f:f + 1] for s in range(S)])
            for s in range(S):
                singles[s].push(frames[s, f:f + 1])
        g_ms, s_ms, worst = [], [], 0.0
        for i in range(pushes):
            f = T - 1 + i
            chunk = [frames[s, f:f + 1] for s in range(S)]
            tg, og = timed(lambda: group.push(chunk))
            ts, os_ = timed(lambda: [singles[s].push(chunk[s]) for s in range(S)])
            assert all(o["anomaly_scores"].shape == (1,) for o in og + os_), "steady state: one window per camera"
            if i >= a.warmup:
                g_ms.append(tg)
                s_ms.append(ts)
                gs = torch.cat([o["anomaly_scores"] for o in og])
                ss = torch.cat([o["anomaly_scores"] for o in os_])
                worst = max(worst, float((gs - ss).abs().max()))
        r = dict(cameras=S, ring_frames_per_camera=group.cap, group=stats(g_ms), sequential_streams=stats(s_ms),
                 max_abs_score_diff=worst)
        r["speedup"] = r["sequential_streams"]["median_ms"] / r["group"]["median_ms"]
        r["group_median_below_sequential_min"] = r["group"]["median_ms"] < r["sequential_streams"]["min_ms"]
        r["group_ms_per_camera"] = r["group"]["median_ms"] / S
        res["streams"][str(S)] = r
        print(json.dumps({str(S): r}), flush=True)
        del frames, group, singles
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
