"""Times CausalAnomalyDetector.score_video against the clip forward over the same windows (eval mode, fp32, one
process): a video of N frames, windows of T at each of the given strides.  Device events around every repetition,
median of --reps after --warmup; the clip path runs model(X) on the stacked windows in batches of --clip-batch clips
(the stacking is not timed).  A second, profiled pass gives the per-window cost of the windowed sequence kernel
(label head_seq_win) beside the clip kernel's (head_seq).  Writes one JSON file.

    python tools/score_video_timing.py --out profiles/score_video_240x360.json --git-hash $(git rev-parse --short HEAD)
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
    ap.add_argument("--frames", type=int, default=180)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=360)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--strides", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--clip-batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--git-hash", default="unknown")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    from vad_amd.cad import CausalAnomalyDetector
    if not torch.cuda.is_available():
        raise SystemExit("score_video_timing: needs a HIP device (a CPU run gives no time)")
    torch.manual_seed(0)
    m = CausalAnomalyDetector().cuda().eval()
    N, T, H, W = a.frames, a.window, a.height, a.width
    g = torch.Generator(device="cuda").manual_seed(1)
    frames = torch.rand(N, 1, H, W, device="cuda", generator=g) * 2 - 1

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=a.reps)

    res = dict(git=a.git_hash, device=torch.cuda.get_device_name(0), frames=N, height=H, width=W, window=T,
               chunk=a.chunk, clip_batch=a.clip_batch, dtype="fp32", strides={})
    eng = m.engine()
    for s in a.strides:
        Wn = (N - T) // s + 1
        X = torch.stack([frames[w * s:w * s + T] for w in range(Wn)])
        batches = [X[i:i + a.clip_batch].contiguous() for i in range(0, Wn, a.clip_batch)]

        def clip_path():
            with torch.no_grad():
                return [m(xb, seed=0, clip0=i * a.clip_batch)["anomaly_scores"] for i, xb in enumerate(batches)]

        def video_path():
            return m.score_video(frames, window=T, stride=s, chunk=a.chunk)["anomaly_scores"]

        diff = float((torch.cat(clip_path()) - video_path()).abs().max())
        r = dict(windows=Wn, frames_through_backbone=dict(clip=Wn * T, score_video=N), max_abs_score_diff=diff,
                 clip=timed(clip_path), score_video=timed(video_path))
        r["speedup"] = r["clip"]["median_ms"] / r["score_video"]["median_ms"]
        # per-window cost of the two sequence kernels (profiled pass: hipEventRecord around each labelled launch)
        eng.profile(True)
        clip_path()
        video_path()
        prof = {}
        for shape, pl in eng.plans.items():
            for k, (tot, cnt) in eng.profile_read(shape).items():
                if k in ("head_seq", "head_seq_win", "window_mean", "frame_cache", "head_rows", "avgpool"):
                    t0, c0 = prof.get(k, (0.0, 0))
                    prof[k] = (t0 + tot, c0 + cnt)
        eng.profile(False)
        r["profiled"] = {k: dict(total_ms=v[0], launches=v[1]) for k, v in prof.items()}
        for k in ("head_seq", "head_seq_win"):
            if k in prof:
                r["profiled"][k]["us_per_window"] = 1e3 * prof[k][0] / Wn
        res["strides"][str(s)] = r
        print(json.dumps({str(s): r}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
