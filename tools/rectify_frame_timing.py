"""One frame of System::TrackStereoPairSemantic from RGB host images at 1242 x 375: the median wall time of the call over the frames of a synthetic
sequence, without the Rectify.* settings keys (vdo_rgb2gray round trips and three uploads) or with identity keys (one vdo_rectify_compute: grey
conversion and upload fused).  --package-root runs another checkout's vdo_slam_amd (a parent commit's, without keys) on the same inputs.
  python tools/rectify_frame_timing.py [--keys none|identity] [--frames 30] [--warmup 5] [--package-root DIR]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", choices=["none", "identity"], default="none")
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
    Ts = SQ.camera_poses(n); objs = SQ.default_objects()
    rng = np.random.default_rng(1)
    frames = []
    for k in range(n):
        fr = SQ.render_frame(k, Ts, objs, flow_sigma=0.1)
        disp = np.clip(np.rint(fr["depth_raw"] / 256.0), 0, 127).astype(np.int64)
        right = rng.integers(0, 256, (H, W)).astype(np.uint8)
        SR.warp_right(fr["gray"], disp, right)
        nxt = rng.integers(0, 256, (H, W)).astype(np.uint8)
        ys, xs = np.mgrid[0:H, 0:W]
        xt, yt = xs + np.rint(fr["flow"][..., 0]).astype(np.int64), ys + np.rint(fr["flow"][..., 1]).astype(np.int64)
        ok = (xt >= 0) & (xt < W) & (yt >= 0) & (yt < H)
        nxt[yt[ok], xt[ok]] = fr["gray"][ok]
        rgb = lambda g: np.ascontiguousarray(np.repeat(g[..., None], 3, -1))
        frames.append((rgb(fr["gray"]), rgb(right), rgb(nxt), (fr["mask"] > 0).astype(np.uint8) * 26))
    kw = {}
    if a.keys == "identity":
        cam = dict(K=synth.KITTI_K, D=(0, 0, 0, 0, 0), R=(1, 0, 0, 0, 1, 0, 0, 0, 1))
        kw["rectify"] = dict(left=cam, right=cam)
    cfg = write_settings(os.path.join(a.tmp, f"rectify_frame_timing_{os.getpid()}.yaml"), W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ, **kw)
    rows = np.array([[0, lab, 0, 0, 0, 0, 0, 0, 0, 0] for lab in range(1, 40)], np.float32)
    s = System(cfg, sensor="stereo")
    ms, failed = [], 0
    for k, (l, r, nx, c) in enumerate(frames):
        t0 = time.perf_counter()
        T = s.track_stereo_pair_semantic(l, r, nx, c, rows, n_images=1 << 30)
        dt = (time.perf_counter() - t0) * 1e3
        failed += T is None
        if k >= a.warmup:
            ms.append(dt)
    s.close()
    os.remove(cfg)
    ms.sort()
    print(f"TrackStereoPairSemantic {W} x {H} RGB host images, keys {a.keys}, package {os.path.relpath(os.path.abspath(a.package_root), ROOT)}: "
          f"median {ms[len(ms) // 2]:.3f} ms  min {ms[0]:.3f}  max {ms[-1]:.3f}  ({len(ms)} frames after {a.warmup}, {failed} failed)")


if __name__ == "__main__":
    main()
