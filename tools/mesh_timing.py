"""Times vdo_mesh_extract on the default 256 x 128 x 256 volume after the synthetic sequence was fused into it (the depth, mask and pose of every
frame as System::TrackRGBD made them), with vdo_dense_extract of the same volume in the same process as the yardstick: device outputs, the
handle's own device time (events from the first launch to the end of the last kernel), warm-up calls, then the median / min / max of the runs.
  python tools/mesh_timing.py [--frames 12] [--runs 20] [--warmup 3] [--voxel 0.1]"""
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
    import torch
    from vdo_slam_amd import _capi as K, synth, synth_frames as SF, synth_seq as SQ
    from vdo_slam_amd.ba import Context
    from vdo_slam_amd.mesh import FollowingMesh
    from vdo_slam_amd.system import System, write_settings
    W, H, n = synth.KITTI_W, synth.KITTI_H, (256, 128, 256)
    Ts = SQ.camera_poses(a.frames); objs = SQ.default_objects()
    cfg = write_settings(os.path.join(a.tmp, f"mesh_timing_{os.getpid()}.yaml"), W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ)
    s = System(cfg, sensor="rgbd")
    ctx = Context(0)
    fm = FollowingMesh(ctx, W, H, n, a.voxel, synth.KITTI_K, max_depth=SF.TH_DEPTH_BG)
    for k in range(a.frames):
        fr = SQ.render_frame(k, Ts, objs, flow_sigma=0.1)
        T = s.track_rgbd(fr["gray"], fr["depth_raw"].copy(), fr["flow"], fr["mask"].copy())
        if T is None:
            raise SystemExit(f"frame {k}: tracking failed")
        depth, mask = s.last_depth_mask(W, H)
        fm.fuse(depth, mask, T)
    s.close(); os.remove(cfg)
    m, ms = fm.mapper, fm.mesher
    o = m.origin(); lo, hi = list(o), [o[c] + n[c] for c in range(3)]
    nvox = n[0] * n[1] * n[2]
    nv, nt = ms.count(m, lo, hi, 0, fm.min_weight)
    npts = m.count(lo, hi, fm.min_weight)
    dev = dict(device="cuda")
    xyz = torch.empty((max(nv, npts), 3), dtype=torch.float32, **dev); grad = torch.empty((max(nv, npts), 3), dtype=torch.int32, **dev)
    wgt = torch.empty(max(nv, npts), dtype=torch.int32, **dev); tri = torch.empty((nt, 3), dtype=torch.int32, **dev)
    torch.cuda.synchronize()
    clo = (C.c_int32 * 3)(*lo); chi = (C.c_int32 * 3)(*hi)
    t_mesh, t_count, t_pts = [], [], []
    for r in range(a.warmup + a.runs):                                         # the three alternate, so that a drift of the machine meets all of them
        ms.extract_raw(m, lo, hi, 0, fm.min_weight, nv, xyz.data_ptr(), grad.data_ptr(), wgt.data_ptr(), nt, tri.data_ptr(), True)
        d_mesh = ms.timing()[1]
        ms.extract_raw(m, lo, hi, 0, fm.min_weight, 0, None, None, None, 0, None, True)
        d_count = ms.timing()[1]
        cnt = C.c_int64()
        K.check(m._L.vdo_dense_extract(m._h, clo, chi, fm.min_weight, npts, C.c_void_p(xyz.data_ptr()), C.c_void_p(grad.data_ptr()), C.c_void_p(wgt.data_ptr()), 1, C.byref(cnt)))
        d_pts = m.timing()[1]
        if r >= a.warmup:
            t_mesh.append(d_mesh); t_count.append(d_count); t_pts.append(d_pts)
    med = sorted(t_mesh)[len(t_mesh) // 2]
    print(f"volume {n[0]} x {n[1]} x {n[2]} ({nvox * 4 / (1 << 20):.0f} MiB), voxel {a.voxel} m, {a.frames} frames of the synthetic sequence fused at {W} x {H}, "
          f"{fm.recenters} recentrings, min_weight {fm.min_weight}; device outputs; the handle's device time; {a.runs} runs after {a.warmup}")
    print(f"  vdo_mesh_extract, whole volume, {nv} vertices, {nt} triangles      {stats(t_mesh)}  | {nvox * 4 / (med * 1e-3) / 1e12:.3f} TB/s over the 4 bytes per voxel")
    print(f"  vdo_mesh_extract, whole volume, counts only (capacities 0)        {stats(t_count)}")
    print(f"  vdo_dense_extract, whole volume, {npts} points (the yardstick)    {stats(t_pts)}  | {nvox * 4 / (sorted(t_pts)[len(t_pts) // 2] * 1e-3) / 1e12:.3f} TB/s over the 4 bytes per voxel")
    fm.close(); ctx.close()


if __name__ == "__main__":
    main()
