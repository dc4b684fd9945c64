"""Times VideoAutoEncoder.score_video against the clip path over the same windows (eval mode, fp32, one process): a
video of N 64x64 frames, windows of T at each of the given strides.  Device events around every repetition, median /
min / max of --reps after --warmup; the clip path runs AeTrainer.eval_batch on the stacked windows in batches of
--clip-batch clips (the stacking is not timed) and blends 0.7 * error + 0.3 * memory score as
calculate_anomaly_scores does.  Records the largest score difference between the two paths.  Writes one JSON file.

    python tools/ae_score_video_timing.py --out profiles/ae_score_video_64x64.json --git-hash $(git rev-parse --short HEAD)
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
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--strides", type=int, nargs="+", default=[4, 1])
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--clip-batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--git-hash", default="unknown")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    from vad_amd.ae import AeTrainer, VideoAutoEncoder
    if not torch.cuda.is_available():
        raise SystemExit("ae_score_video_timing: needs a HIP device (a CPU run gives no time)")
    torch.manual_seed(0)
    m = VideoAutoEncoder().cuda().eval()
    N, T = a.frames, a.window
    g = torch.Generator(device="cuda").manual_seed(1)
    frames = torch.rand(N, 1, 64, 64, device="cuda", generator=g).clamp_(0.001, 0.999)
    with torch.no_grad():  # a filled ring, so that the memory score does its work
        m.update_memory(torch.randn(64, 64, device="cuda", generator=g))
    trainer = AeTrainer(m)

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

    res = dict(git=a.git_hash, device=torch.cuda.get_device_name(0), frames=N, height=64, width=64, window=T,
               chunk=a.chunk, clip_batch=a.clip_batch, dtype="fp32", warmup=a.warmup, strides={})
    for s in a.strides:
        Wn = (N - T) // s + 1
        X = torch.stack([frames[w * s:w * s + T] for w in range(Wn)])
        batches = [X[i:i + a.clip_batch].contiguous() for i in range(0, Wn, a.clip_batch)]

        def clip_path():
            out = []
            for xb in batches:
                o = trainer.eval_batch(xb)
                out.append(0.7 * o["recon_error"] + 0.3 * o["anomaly_score"])
            return out

        def video_path():
            return m.score_video(frames, window=T, stride=s, chunk=a.chunk)["anomaly_scores"]

        diff = float((torch.cat(clip_path()) - video_path()).abs().max())
        r = dict(windows=Wn, frames_encoded=dict(clip=Wn * T, score_video=N), max_abs_score_diff=diff,
                 clip=timed(clip_path), score_video=timed(video_path))
        r["speedup"] = r["clip"]["median_ms"] / r["score_video"]["median_ms"]
        # acceptance: score_video's median below the clip path's fastest repetition
        r["median_below_clip_min"] = r["score_video"]["median_ms"] < r["clip"]["min_ms"]
        res["strides"][str(s)] = r
        print(json.dumps({str(s): r}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
