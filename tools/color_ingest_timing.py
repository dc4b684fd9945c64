"""Times one push of raw colour camera frames in steady state (rings full, eval mode, fp32, one process): packed bgr
frames at the camera's size in pinned host memory, one frame per camera per push, --streams S cameras in a stream
group, for CausalAnomalyDetector (target --height x --width) and the memory autoencoder (64x64).  Three legs, run one
after the other within every repetition, each on a group of its own:

  push_u8_color  group.push_u8(color="bgr") on the pinned colour frames (one table-form colour ingest launch: luma per
                 tap, resize, normalise; then push's body)
  host_route     what the package offered before: PIL convert("L") per frame on the host, data.resize_u8, the numpy
                 normalise, .to(device) per camera, then group.push
  push_u8_grey   group.push_u8 on grey pinned frames of the same size: the grey instantiation, to compare with
                 profiles/ingest_u8_240x360.json (push_u8)

and bbox.score_video over a --video-frames video of 64x64 planar RGB frames in HBM at strides 4 and 1, against
model(clips) over the same windows gathered with torch (index_select + permute + contiguous) at the same batch size.

Wall-clock time of the host thread from the call to the end of a device synchronise (the host route's cost is host
work, which device events would not see).  Median (min-max) of --reps after --warmup.  Also the largest absolute
difference between the colour push's and the host route's scores, and between score_video and the clip path, which must
be 0.  Writes one JSON file.

    python tools/color_ingest_timing.py --out profiles/color_ingest_240x360.json --git-hash $(git rev-parse --short HEAD)
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
    ap.add_argument("--video-frames", type=int, default=180)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--git-hash", default="unknown")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from vad_amd import data
    from vad_amd.ae import VideoAutoEncoder
    from vad_amd.bbox import CausalAnomalyDetector as BboxDetector
    from vad_amd.cad import CausalAnomalyDetector
    if not torch.cuda.is_available():
        raise SystemExit("color_ingest_timing: needs a HIP device (a CPU run gives no time)")
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
               source_memory="pinned host, uint8, packed bgr (grey leg: one byte per pixel)", window=T, stride=1,
               dtype="fp32", frames_per_camera_per_push=1, clock="host wall clock, call to end of synchronize",
               models={})
    pushes = a.warmup + a.reps
    NF = 4  # distinct frames per camera, pushed in turn
    for name, (m, size, mode, kw, norm) in models.items():
        res["models"][name] = dict(target=list(size), mode=mode, streams={})
        for S in a.streams:
            rng = np.random.default_rng(S)
            bgr = torch.from_numpy(rng.integers(0, 256, (S, NF, Hs, Ws, 3), dtype=np.uint8)).pin_memory()
            rgb_np = np.ascontiguousarray(bgr.numpy()[..., ::-1])  # (what a decoder hands PIL; the flip is not timed)
            grey = torch.from_numpy(rng.integers(0, 256, (S, NF, Hs, Ws), dtype=np.uint8)).pin_memory()

            def host_route(f):
                out = []
                for s in range(S):
                    g = np.asarray(Image.fromarray(rgb_np[s, f]).convert("L"))
                    out.append(torch.from_numpy(norm(data.resize_u8(g, *size))[None, None]).to("cuda"))
                return out

            legs = {
                "push_u8_color": lambda g, f: g.push_u8([bgr[s, f:f + 1] for s in range(S)], color="bgr"),
                "host_route": lambda g, f: g.push(host_route(f)),
                "push_u8_grey": lambda g, f: g.push_u8([grey[s, f:f + 1] for s in range(S)]),
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
                worst = max(worst, float((sc["push_u8_color"] - sc["host_route"]).abs().max()))
            r = {k: stats(v) for k, v in ms.items()}
            r["cameras"] = S
            r["max_abs_score_diff_color_vs_host_route"] = worst
            r["speedup_color_over_host_route"] = r["host_route"]["median_ms"] / r["push_u8_color"]["median_ms"]
            r["color_max_below_host_route_min"] = r["push_u8_color"]["max_ms"] < r["host_route"]["min_ms"]
            r["ranges_overlap"] = not (r["push_u8_color"]["max_ms"] < r["host_route"]["min_ms"]
                                       or r["host_route"]["max_ms"] < r["push_u8_color"]["min_ms"])
            res["models"][name]["streams"][str(S)] = r
            print(json.dumps({name: {str(S): r}}), flush=True)
            del groups, bgr, grey

    # bbox: score_video on the video in place against the clip path on clips gathered with torch
    bb = BboxDetector().cuda().eval()
    N, W, B = a.video_frames, 8, 64
    x = torch.rand(N, 3, 64, 64, device="cuda")
    res["bbox"] = dict(frames=N, frame=[64, 64], window=W, batch=B, strides={})
    for stride in (4, 1):
        starts = torch.arange(0, N - W + 1, stride, device="cuda")
        idx = (starts[:, None] + torch.arange(W, device="cuda")[None]).reshape(-1)

        def clip_path():
            clips = x.index_select(0, idx).view(-1, W, 3, 64, 64).permute(0, 2, 1, 3, 4).contiguous()
            with torch.no_grad():
                parts = [bb(clips[w0:w0 + B]) for w0 in range(0, clips.shape[0], B)]
            return torch.cat([p[0].reshape(-1) for p in parts])

        legs = {"score_video": lambda: bb.score_video(x, window=W, stride=stride, batch=B)["anomaly_scores"],
                "clip_path": clip_path}
        ms, worst = {k: [] for k in legs}, 0.0
        for i in range(pushes):
            outs = {}
            for k, fn in legs.items():
                t, outs[k] = timed(fn)
                if i >= a.warmup:
                    ms[k].append(t)
            worst = max(worst, float((outs["score_video"] - outs["clip_path"]).abs().max()))
        r = {k: stats(v) for k, v in ms.items()}
        r["windows"] = int(starts.numel())
        r["max_abs_score_diff"] = worst
        r["speedup_score_video_over_clip_path"] = r["clip_path"]["median_ms"] / r["score_video"]["median_ms"]
        r["ranges_overlap"] = not (r["score_video"]["max_ms"] < r["clip_path"]["min_ms"]
                                   or r["clip_path"]["max_ms"] < r["score_video"]["min_ms"])
        res["bbox"]["strides"][str(stride)] = r
        print(json.dumps({"bbox": {str(stride): r}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
