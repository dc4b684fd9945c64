"""Times one push of a VideoAutoEncoder stream in steady state (ring full, eval mode, fp32, one process) against the
two ways to get the same result without a stream: score_video(last T frames, window=T) once per new frame, and
AeTrainer.eval_batch(last T frames) plus the blend 0.7 * error + 0.3 * memory score once per new frame.  For each
--max-push k a push brings k frames and completes k windows (stride 1), so the two other paths run k times per push,
k calls inside one event pair.  Device events around every push, median and min / max of --reps after --warmup.  Writes
one JSON file.

    python tools/ae_stream_timing.py --out profiles/ae_stream_64x64.json --git-hash $(git rev-parse --short HEAD)
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
    ap.add_argument("--max-push", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--git-hash", default="unknown")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    from vad_amd.ae import AeTrainer, VideoAutoEncoder
    if not torch.cuda.is_available():
        raise SystemExit("ae_stream_timing: needs a HIP device (a CPU run gives no time)")
    torch.manual_seed(0)
    m = VideoAutoEncoder().cuda().eval()
    T = a.window
    g = torch.Generator(device="cuda").manual_seed(1)
    with torch.no_grad():  # a filled ring, so that the memory score does its work
        m.update_memory(torch.randn(64, 64, device="cuda", generator=g))
    trainer = AeTrainer(m)

    def summary(ms):
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=len(ms))

    res = dict(git=a.git_hash, device=torch.cuda.get_device_name(0), height=64, width=64, window=T, stride=1,
               dtype="fp32", warmup=a.warmup, max_push={})
    for k in a.max_push:
        # the stream: T - 1 frames to fill the ring short of the first window, then warmup + reps pushes of k frames
        pushes = a.warmup + a.reps
        fill = (T - 1 + k - 1) // k * k
        N = fill + pushes * k
        frames = torch.rand(N, 1, 64, 64, device="cuda", generator=g).clamp_(0.001, 0.999)
        s = m.open_stream(window=T, stride=1, max_push=k)
        f = 0
        while f < fill:
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

        def video_call(w):
            return m.score_video(frames[w:w + T], window=T, stride=1)["anomaly_scores"]

        def clip_call(w):
            with torch.no_grad():
                o = trainer.eval_batch(frames[w:w + T][None])
                return 0.7 * o["recon_error"] + 0.3 * o["anomaly_score"]

        video_ms, video_scores = other_path(video_call)
        clip_ms, clip_scores = other_path(clip_call)
        r = dict(frames_per_push=k, windows_per_push=k, ring_frames=s.cap, ring_bytes=s._ring.numel() * 4,
                 stream=summary(ms), score_video=summary(video_ms), eval_batch=summary(clip_ms),
                 max_abs_score_diff=dict(
                     stream_vs_score_video=float((stream_scores - video_scores).abs().max()),
                     stream_vs_eval_batch=float((stream_scores - clip_scores).abs().max()),
                     score_video_vs_eval_batch=float((video_scores - clip_scores).abs().max())))
        r["speedup_vs_score_video"] = r["score_video"]["median_ms"] / r["stream"]["median_ms"]
        r["speedup_vs_eval_batch"] = r["eval_batch"]["median_ms"] / r["stream"]["median_ms"]
        res["max_push"][str(k)] = r
        print(json.dumps({str(k): r}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
