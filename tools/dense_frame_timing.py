"""One frame of System::TrackRGBD from host images at 1242 x 375 with and without the Dense.* settings keys, on the same frames and the same
build: the median wall time of the call over the frames of a synthetic sequence, and what the dense mapper did.
  python tools/dense_frame_timing.py [--frames 30] [--warmup 5] [--voxel 0.1] [--size 512 128 512]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--size", type=int, nargs=3, default=[512, 128, 512])
    ap.add_argument("--tmp", default="/tmp")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ
    from vdo_slam_amd.system import System, write_settings
    W, H, n = synth.KITTI_W, synth.KITTI_H, a.frames + a.warmup
    Ts = SQ.camera_poses(n); objs = SQ.default_objects()
    frames = [SQ.render_frame(k, Ts, objs, flow_sigma=0.1) for k in range(n)]
    for keyed in (False, True, False):
        cfg = write_settings(os.path.join(a.tmp, f"dense_frame_timing_{os.getpid()}.yaml"), W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ)
        if keyed:
            with open(cfg, "a") as f:
                f.write(f"Dense.VoxelSize: {a.voxel}\nDense.Size: {list(a.size)}\n")
        s = System(cfg, sensor="rgbd")
        ms, failed, updated = [], 0, []
        for k, fr in enumerate(frames):
            depth, mask = fr["depth_raw"].copy(), fr["mask"].copy()
            t0 = time.perf_counter()
            T = s.track_rgbd(fr["gray"], depth, fr["flow"], mask)
            dt = (time.perf_counter() - t0) * 1e3
            failed += T is None
            if keyed:
                updated.append(s.dense_info()["counts"][0])
            if k >= a.warmup:
                ms.append(dt)
        ms.sort()
        what = f"with Dense.VoxelSize {a.voxel}, Dense.Size {list(a.size)}" if keyed else "without the Dense.* keys"
        print(f"TrackRGBD {W} x {H} host images, {what}: median {ms[len(ms) // 2]:.3f} ms  min {ms[0]:.3f}  max {ms[-1]:.3f}  ({len(ms)} frames after {a.warmup}, {failed} failed)")
        if keyed:
            info = s.dense_info()
            print(f"  updated voxels per frame min / median / max {min(updated)} / {int(np.median(updated))} / {max(updated)}, {info['recenters']} recentrings, "
                  f"{info['kept_points']} points kept on the host")
        s.close()
        os.remove(cfg)


if __name__ == "__main__":
    main()
