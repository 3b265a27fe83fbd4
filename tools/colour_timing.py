"""Times vdo_colour_integrate_frame beside vdo_dense_integrate_frame on DenseMapper::DefaultSettings' 256 x 128 x 256 volume and a KITTI-sized frame:
the synthetic sequence is tracked by System, every frame's resident depth and mask are fused into a following volume and its grey image into the
colour volume beside it; then the LAST frame is fused again and again from a vdo_frame_images (depth and mask resident, the image on the device),
geometry and colour alternating, each timed by its handle's own device time (events around the kernels of the call).
  python tools/colour_timing.py [--frames 12] [--runs 20] [--warmup 3] [--voxel 0.1]"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:.3f} ms  min {ms[0]:.3f}  max {ms[-1]:.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--tmp", default="/tmp")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from vdo_slam_amd import synth, synth_frames as SF, synth_seq as SQ
    from vdo_slam_amd.ba import Context
    from vdo_slam_amd.colour import FollowingColourMesh
    from vdo_slam_amd.system import System, write_settings
    from vdo_slam_amd.frontend import FrameImages
    W, H, n = synth.KITTI_W, synth.KITTI_H, (256, 128, 256)
    Ts = SQ.camera_poses(a.frames); objs = SQ.default_objects()
    cfg = write_settings(os.path.join(a.tmp, f"colour_timing_{os.getpid()}.yaml"), W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ)
    s = System(cfg, sensor="rgbd")
    ctx = Context(0)
    fm = FollowingColourMesh(ctx, W, H, n, a.voxel, synth.KITTI_K, max_depth=SF.TH_DEPTH_BG)      # band trunc / 2, colour weight cap 64: the settings' defaults
    for k in range(a.frames):
        fr = SQ.render_frame(k, Ts, objs, flow_sigma=0.1)
        T = s.track_rgbd(fr["gray"], fr["depth_raw"].copy(), fr["flow"], fr["mask"].copy())
        if T is None:
            raise SystemExit(f"frame {k}: tracking failed")
        depth, mask = s.last_depth_mask(W, H)
        fm.fuse(depth, mask, fr["gray"], T)
    s.close(); os.remove(cfg)
    m, col = fm.mapper, fm.colourer
    frame = FrameImages(ctx, W, H)
    frame.upload(depth, np.zeros((H, W, 2), np.float32), mask)
    gray = torch.from_numpy(np.ascontiguousarray(fr["gray"])).cuda()
    torch.cuda.synchronize()
    nvox = n[0] * n[1] * n[2]
    rows = {}
    for vpt in (4, 1, 2, 8):
        m.set_voxels_per_thread(vpt); col.set_voxels_per_thread(vpt)
        t_geo, t_col = [], []
        for r in range(a.warmup + a.runs):                                       # the two alternate, so that a drift of the machine meets both
            geo = m.integrate_frame(frame._h, T)
            d_geo = m.timing()[1]
            cnt = col.integrate_frame(frame._h, gray.data_ptr(), W, 1, 0, True, T)
            d_col = col.timing()[1]
            if r >= a.warmup:
                t_geo.append(d_geo); t_col.append(d_col)
        rows[vpt] = (t_geo, t_col, geo, cnt)
    print(f"volume {n[0]} x {n[1]} x {n[2]} ({nvox * 4 / (1 << 20):.0f} MiB of TSDF words, as many of colour words), voxel {a.voxel} m, {W} x {H} frame, {a.frames} frames of the synthetic "
          f"sequence fused, {fm.recenters} recentrings; resident depth and mask, grey device image; each handle's device time; {a.runs} runs after {a.warmup}")
    for vpt, (t_geo, t_col, geo, cnt) in rows.items():
        print(f"  {vpt} voxels per thread: vdo_dense_integrate_frame  {stats(t_geo)}  (updated {geo[0]}, masked {geo[1]}, occluded {geo[2]})")
        print(f"  {vpt} voxels per thread: vdo_colour_integrate_frame {stats(t_col)}  (updated {cnt[0]}, label {cnt[1]}, outside the band {cnt[2]}; pack kernel included)")
    frame.close(); fm.close(); ctx.close()


if __name__ == "__main__":
    main()
