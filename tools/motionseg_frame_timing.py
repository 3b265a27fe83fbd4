"""One frame of System::TrackStereoVideo from RGB host images at 1242 x 375 - the current and the next stereo pair, nothing else - and, beside it on
the same images and the same build, one frame of System::TrackStereoPairSemantic fed the rendered object pixels as its class image: the median wall
time of the call over the frames of a synthetic sequence.  --package-root runs another checkout's vdo_slam_amd (a parent commit's: the existing entry
only) on the same inputs.
  python tools/motionseg_frame_timing.py [--entry video|semantic|both] [--frames 30] [--warmup 5] [--package-root DIR]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entry", choices=["video", "semantic", "both"], default="both")
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--tmp", default="/tmp")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.abspath(a.package_root))
    from tests import stereo_ref as SR
    from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ
    from vdo_slam_amd.system import System, write_settings
    W, H, n = synth.KITTI_W, synth.KITTI_H, a.frames + a.warmup
    Ts = SQ.camera_poses(n + 1); objs = SQ.default_objects()
    rng = np.random.default_rng(1)
    rendered = [SQ.render_frame(k, Ts, objs, flow_sigma=0.1) for k in range(n + 1)]
    disps = [np.clip(np.rint(fr["depth_raw"] / 256.0), 0, 127).astype(np.int64) for fr in rendered]
    rgb = lambda g: np.ascontiguousarray(np.repeat(g[..., None], 3, -1))
    ys, xs = np.mgrid[0:H, 0:W]
    frames = []
    for k in range(n):
        fr = rendered[k]
        right = rng.integers(0, 256, (H, W)).astype(np.uint8)
        SR.warp_right(fr["gray"], disps[k], right)
        nxt = rng.integers(0, 256, (H, W)).astype(np.uint8)
        xt, yt = xs + np.rint(fr["flow"][..., 0]).astype(np.int64), ys + np.rint(fr["flow"][..., 1]).astype(np.int64)
        ok = (xt >= 0) & (xt < W) & (yt >= 0) & (yt < H)
        nxt[yt[ok], xt[ok]] = fr["gray"][ok]
        nxt_right = rng.integers(0, 256, (H, W)).astype(np.uint8)
        SR.warp_right(nxt, disps[k + 1], nxt_right)
        frames.append((rgb(fr["gray"]), rgb(right), rgb(nxt), rgb(nxt_right), (fr["mask"] > 0).astype(np.uint8) * 26))
    cfg = write_settings(os.path.join(a.tmp, f"motionseg_frame_timing_{os.getpid()}.yaml"), W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ)
    rows = np.array([[0, lab, 0, 0, 0, 0, 0, 0, 0, 0] for lab in range(1, 40)], np.float32)
    where = os.path.relpath(os.path.abspath(a.package_root), ROOT)
    for entry in (("semantic", "video") if a.entry == "both" else (a.entry,)):
        s = System(cfg, sensor="stereo")
        ms, failed, found = [], 0, []
        for k, (l, r, nx, nr, c) in enumerate(frames):
            t0 = time.perf_counter()
            T = s.track_stereo_video(l, r, nx, nr, rows, n_images=1 << 30) if entry == "video" else s.track_stereo_pair_semantic(l, r, nx, c, rows, n_images=1 << 30)
            dt = (time.perf_counter() - t0) * 1e3
            failed += T is None
            if entry == "video":
                found.append(s.video_counts())
            if k >= a.warmup:
                ms.append(dt)
        s.close()
        ms.sort()
        name = "TrackStereoVideo" if entry == "video" else "TrackStereoPairSemantic"
        print(f"{name} {W} x {H} RGB host images, package {where}: median {ms[len(ms) // 2]:.3f} ms  min {ms[0]:.3f}  max {ms[-1]:.3f}  ({len(ms)} frames after {a.warmup}, "
              f"{failed} failed)")
        if found:
            f = np.array(found)
            print(f"  per frame, min / median / max: ego-motion inliers {f[:, 0].min()} / {int(np.median(f[:, 0]))} / {f[:, 0].max()}, moving pixels {f[:, 1].min()} / "
                  f"{int(np.median(f[:, 1]))} / {f[:, 1].max()}, labels {f[:, 2].min()} / {int(np.median(f[:, 2]))} / {f[:, 2].max()}")
    os.remove(cfg)


if __name__ == "__main__":
    main()
