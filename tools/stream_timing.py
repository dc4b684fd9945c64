"""Times one push of a CausalAnomalyDetector stream in steady state (ring full, eval mode, fp32, one process) against
the two ways to get the same result without a stream: model(last T frames) once per new frame, and
score_video(last T frames, window=T) once per new frame.  For each --max-push k a push brings k frames and completes
k windows (stride 1), so the two other paths run k times per push.  Device events around every push, median of
--reps after --warmup; the events enclose the push's host reads (nmax / counts), as they do for the other two paths.
A second, profiled pass gives the device time of the labelled launches of one push.  Writes one JSON file.

    python tools/stream_timing.py --out profiles/stream_240x360.json --git-hash $(git rev-parse --short HEAD)
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
    ap.add_argument("--max-push", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--git-hash", default="unknown")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    from vad_amd.cad import CausalAnomalyDetector
    if not torch.cuda.is_available():
        raise SystemExit("stream_timing: needs a HIP device (a CPU run gives no time)")
    torch.manual_seed(0)
    m = CausalAnomalyDetector().cuda().eval()
    T, H, W = a.window, a.height, a.width
    eng = m.engine()

    def median_ms(ms):
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=len(ms))

    res = dict(git=a.git_hash, device=torch.cuda.get_device_name(0), height=H, width=W, window=T, stride=1,
               dtype="fp32", max_push={})
    for k in a.max_push:
        # the stream: T - 1 frames to fill the ring short of the first window, then warmup + reps pushes of k frames
        pushes = a.warmup + a.reps
        N = (T - 1 + k - 1) // k * k + pushes * k
        g = torch.Generator(device="cuda").manual_seed(1)
        frames = torch.rand(N, 1, H, W, device="cuda", generator=g) * 2 - 1
        s = m.open_stream(window=T, stride=1, max_push=k)
        f = 0
        while f + k <= N - pushes * k:
            s.push(frames[f:f + k])
            f += k
        ms, scores, starts = [], [], []
        for i in range(pushes):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            o = s.push(frames[f:f + k])
            e1.record()
            torch.cuda.synchronize()
            f += k
            assert o["anomaly_scores"].shape == (k,), "steady state: every push completes k windows"
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
                scores.append(o["anomaly_scores"])
                starts += o["window_starts"].tolist()
        stream_scores = torch.cat(scores)

        # the same windows without a stream, k calls per push
        def other_path(fn):
            ms, scores = [], []
            for i in range(pushes):
                ws = starts[:k] if i < a.warmup else starts[(i - a.warmup) * k:(i - a.warmup + 1) * k]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = [fn(w) for w in ws]
                e1.record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    ms.append(e0.elapsed_time(e1))
                    scores += out
            return ms, torch.cat(scores)

        def clip_call(w):
            with torch.no_grad():
                return m(frames[w:w + T][None], seed=0, clip0=w)["anomaly_scores"]

        def video_call(w):
            return m.score_video(frames[w:w + T], window=T, stride=1, seed=0, clip0=w)["anomaly_scores"]

        clip_ms, clip_scores = other_path(clip_call)
        video_ms, video_scores = other_path(video_call)
        r = dict(frames_per_push=k, windows_per_push=k, ring_frames=s.cap,
                 stream=median_ms(ms), clip=median_ms(clip_ms), score_video=median_ms(video_ms),
                 max_abs_score_diff=dict(
                     stream_vs_clip=float((stream_scores - clip_scores).abs().max()),
                     stream_vs_score_video=float((stream_scores - video_scores).abs().max()),
                     clip_vs_score_video=float((clip_scores - video_scores).abs().max())))
        r["speedup_vs_clip"] = r["clip"]["median_ms"] / r["stream"]["median_ms"]
        r["speedup_vs_score_video"] = r["score_video"]["median_ms"] / r["stream"]["median_ms"]
        # where a push's device time goes (profiled pass: an event pair around each labelled launch)
        s2 = m.open_stream(window=T, stride=1, max_push=k)
        for f in range(0, (T - 1 + k - 1) // k * k, k):
            s2.push(frames[f:f + k])
        eng.profile(True)
        np_ = 4
        for j in range(np_):
            s2.push(frames[f + (j + 1) * k:f + (j + 2) * k])
        prof = eng.profile_read((k, 1, H, W))
        eng.profile(False)
        r["profiled_per_push_ms"] = {lab: tot / np_ for lab, (tot, cnt) in sorted(prof.items(), key=lambda kv: -kv[1][0])}
        r["profiled_per_push_ms"]["all_labelled_launches"] = sum(tot for tot, _ in prof.values()) / np_
        r["profiled_launches_per_push"] = sum(cnt for _, cnt in prof.values()) / np_
        res["max_push"][str(k)] = r
        print(json.dumps({str(k): r}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
