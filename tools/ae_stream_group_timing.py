"""Times one push of a VideoAutoEncoder stream group in steady state (rings full, eval mode, fp32, one process) against
the way to get the same result without a group: one AeStream per camera, pushed one after the other.  For each
--streams S every camera brings one frame per push and completes one window (stride 1).  Device events around every
group push, and around each run of S AeStream pushes (one event pair for the S of them); neither path reads a device
value on the host, so the timed span ends at the device synchronise that follows the second event.  The two paths
alternate push by push in one process.  Median (min-max) of --reps after --warmup, the method of
tools/ae_stream_timing.py.  Also the largest absolute difference between the two paths' scores over the timed pushes.
Writes one JSON file.

    python tools/ae_stream_group_timing.py --out profiles/ae_stream_group_64x64.json --git-hash HASH
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
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 4, 16, 32])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--git-hash", default="unknown")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    from vad_amd.ae import VideoAutoEncoder
    if not torch.cuda.is_available():
        raise SystemExit("ae_stream_group_timing: needs a HIP device (a CPU run gives no time)")
    torch.manual_seed(0)
    m = VideoAutoEncoder().cuda().eval()
    T = a.window
    gen = torch.Generator(device="cuda").manual_seed(1)
    with torch.no_grad():  # a filled memory ring, so that the memory score does its work
        m.update_memory(torch.randn(64, 64, device="cuda", generator=gen))

    def stats(ms):
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=len(ms))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    res = dict(git=a.git_hash, device=torch.cuda.get_device_name(0), height=64, width=64, window=T, stride=1,
               dtype="fp32", frames_per_camera_per_push=1, warmup=a.warmup, streams={})
    pushes = a.warmup + a.reps
    N = T - 1 + pushes
    for S in a.streams:
        frames = torch.rand(S, N, 1, 64, 64, device="cuda", generator=gen).clamp_(0.001, 0.999)
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
        r = dict(cameras=S, ring_frames_per_camera=group.cap, ring_bytes=group._ring.numel() * 4,
                 plan_frames=group.max_frames, group=stats(g_ms), sequential_streams=stats(s_ms),
                 max_abs_score_diff=worst)
        seq = r["sequential_streams"]
        r["speedup"] = seq["median_ms"] / r["group"]["median_ms"]
        r["sequential_spread_ms"] = seq["max_ms"] - seq["min_ms"]
        r["saving_ms"] = seq["median_ms"] - r["group"]["median_ms"]
        r["saving_exceeds_sequential_spread"] = r["saving_ms"] > r["sequential_spread_ms"]
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
