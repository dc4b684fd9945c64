"""Times the in-place window scoring of the three 3-D clip models -- a2.CausalAnomalyDetector,
mc.SimpleVideoAnomalyDetector (grey) and bbox.CausalAnomalyDetector -- against the route the package offered before:
windows gathered into clips with torch (index_select + permute + contiguous), then model(clips).  64 x 64 frames, T = 8,
a video of --video-frames frames in HBM, eval mode, fp32, one process.  Per model:

  score_video vs clip_path   the whole video at strides 4 and 1, both at batch 64 (the clip path in the same batches)
  push vs clip_path          one ClipStream push with the ring full -- one frame (max_push 1) and max_push frames
                             (--max-push, stride 1: as many windows) -- against gathering the same windows from the
                             video and model(clips) on them (a2, one window: the clip twice, as its plans need)

The legs of a comparison alternate within every repetition.  Wall-clock time of the host thread from the call to the
end of a device synchronise.  Median (min-max) of --reps after --warmup, whether the two ranges overlap, and the largest
absolute difference of the scores, which must be 0.  Writes one JSON file.

    python tools/clip_stream_timing.py --out profiles/clip_stream_64x64.json --git-hash $(git rev-parse --short HEAD)
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
    ap.add_argument("--video-frames", type=int, default=180)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--max-push", type=int, default=4)
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
        raise SystemExit("clip_stream_timing: needs a HIP device (a CPU run gives no time)")
    torch.manual_seed(0)
    N, T, B, HW = a.video_frames, a.window, 64, 64
    models = {"a2": (A2Detector().cuda().eval(), 3),
              "mc": (SimpleVideoAnomalyDetector(input_channels=1, temporal_frames=T).cuda().eval(), 1),
              "bbox": (BboxDetector(num_frames=T).cuda().eval(), 3)}

    def stats(ms):
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=len(ms))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def compare(legs, new, old, extra):
        """legs {name: (prepare or None, fn)}: alternate them --warmup + --reps times; prepare is not timed."""
        ms, worst = {k: [] for k in legs}, 0.0
        for i in range(a.warmup + a.reps):
            outs = {}
            for k, (prepare, fn) in legs.items():
                if prepare is not None:
                    prepare()
                t, outs[k] = timed(fn)
                if i >= a.warmup:
                    ms[k].append(t)
            worst = max(worst, float((outs[new] - outs[old]).abs().max()))
        r = {k: stats(v) for k, v in ms.items()}
        r.update(extra)
        r["max_abs_score_diff"] = worst
        r[f"speedup_{new}_over_{old}"] = r[old]["median_ms"] / r[new]["median_ms"]
        r["ranges_overlap"] = not (r[new]["max_ms"] < r[old]["min_ms"] or r[old]["max_ms"] < r[new]["min_ms"])
        return r

    res = dict(git=a.git_hash, device=torch.cuda.get_device_name(0), host_cpus=os.cpu_count(), frames=N,
               frame=[HW, HW], window=T, batch=B, dtype="fp32", clock="host wall clock, call to end of synchronize",
               models={})
    steps = torch.arange(T, device="cuda")[None]
    for name, (m, C) in models.items():
        x = torch.rand(N, C, HW, HW, device="cuda")

        def scores(o):
            return (o if isinstance(o, torch.Tensor) else o[0]).reshape(-1)

        def clip_path(starts, batch=B):
            idx = (starts[:, None] + steps).reshape(-1)
            clips = x.index_select(0, idx).view(-1, T, C, HW, HW).permute(0, 2, 1, 3, 4).contiguous()
            n = clips.shape[0]
            if name == "a2" and n == 1:
                clips = torch.cat([clips, clips])
            with torch.no_grad():
                return torch.cat([scores(m(clips[w0:w0 + batch])) for w0 in range(0, clips.shape[0], batch)])[:n]

        r = dict(channels=C, score_video={}, push={})
        for stride in (4, 1):
            starts = torch.arange(0, N - T + 1, stride, device="cuda")
            r["score_video"][str(stride)] = compare(
                {"score_video": (None, lambda: m.score_video(x, window=T, stride=stride, batch=B)["anomaly_scores"]),
                 "clip_path": (None, lambda: clip_path(starts))},
                "score_video", "clip_path", dict(windows=int(starts.numel())))
            print(json.dumps({name: {"score_video": {str(stride): r["score_video"][str(stride)]}}}), flush=True)
        for k in (1, a.max_push):
            st = m.open_stream(window=T, stride=1, max_push=k)
            state = dict(f=0)
            while state["f"] + k <= T + k:  # the ring full: every later push completes k windows
                st.push(x[state["f"]:state["f"] + k])
                state["f"] += k

            def advance():  # (wrap the video, refilling the ring, outside the timed region)
                if state["f"] + k > N:
                    st.reset()
                    state["f"] = 0
                    while state["f"] < T:
                        st.push(x[state["f"]:state["f"] + k])
                        state["f"] += k

            def push():
                o = st.push(x[state["f"]:state["f"] + k])
                state["f"] += k
                state["starts"] = o["window_starts"].cuda()
                return o["anomaly_scores"]

            r["push"][str(k)] = compare({"push": (advance, push), "clip_path": (None, lambda: clip_path(state["starts"]))},
                                        "push", "clip_path", dict(frames_per_push=k, windows_per_push=k, ring_slots=st.cap))
            print(json.dumps({name: {"push": {str(k): r["push"][str(k)]}}}), flush=True)
        res["models"][name] = r
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
