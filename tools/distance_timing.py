"""Times vdo_distance_compute on the default 256 x 128 x 256 volume after the synthetic sequence was fused into it (the depth, mask and pose of every
frame as System::TrackRGBD made them) at R = 8, 20 and 64 voxels with methods 1 and 2 and with the handle's own choice, and a 1 M-point
vdo_distance_sample on device points, with vdo_mesh_extract of the same volume in the same process as the yardstick: device outputs, the handle's
own device time (events from the first command to the end of the last kernel), warm-up calls, then the median / min / max of the runs.
  python tools/distance_timing.py [--frames 12] [--runs 30] [--warmup 5] [--voxel 0.1]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:.3f} ms  min {ms[0]:.3f}  max {ms[-1]:.3f}"


def median(ms):
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--tmp", default="/tmp")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from vdo_slam_amd import distance as DD, synth, synth_frames as SF, synth_seq as SQ
    from vdo_slam_amd.ba import Context
    from vdo_slam_amd.mesh import FollowingMesh
    from vdo_slam_amd.system import System, write_settings
    W, H, n = synth.KITTI_W, synth.KITTI_H, (256, 128, 256)
    Ts = SQ.camera_poses(a.frames); objs = SQ.default_objects()
    cfg = write_settings(os.path.join(a.tmp, f"distance_timing_{os.getpid()}.yaml"), W, H, synth.KITTI_K, SF.BF, SF.DEPTH_MAP_FACTOR, SF.TH_DEPTH_BG, SF.TH_DEPTH_OBJ)
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
    field = DD.DistanceField(ctx, n)
    nv, nt = ms.count(m, lo, hi, 0, fm.min_weight)
    dev = dict(device="cuda")
    xyz = torch.empty((nv, 3), dtype=torch.float32, **dev); grad = torch.empty((nv, 3), dtype=torch.int32, **dev)
    wgt = torch.empty(nv, dtype=torch.int32, **dev); tri = torch.empty((nt, 3), dtype=torch.int32, **dev)
    npts = 1 << 20
    rng = np.random.default_rng(1)
    pts = torch.from_numpy(((np.array(lo) - 8 + rng.random((npts, 3)) * (np.array(n) + 16)) * a.voxel).astype(np.float32)).cuda()
    words = torch.empty(npts, dtype=torch.int32, **dev)
    torch.cuda.synchronize()
    cases = [(method, R) for R in (8, 20, 64) for method in (1, 2, 0)]
    t = {c: [] for c in cases}
    t_mesh, t_sample = [], []
    counts = {}
    for r in range(a.warmup + a.runs):                                         # everything alternates, so that a drift of the machine meets all of it
        for method, R in cases:
            field.set_method(method)
            counts[R] = field.compute(m, lo, hi, fm.min_weight, R)
            if r >= a.warmup:
                t[(method, R)].append(field.timing()[1])
        inside = field.sample_raw(npts, pts.data_ptr(), words.data_ptr(), True)
        d_sample = field.timing()[1]
        ms.extract_raw(m, lo, hi, 0, fm.min_weight, nv, xyz.data_ptr(), grad.data_ptr(), wgt.data_ptr(), nt, tri.data_ptr(), True)
        if r >= a.warmup:
            t_sample.append(d_sample); t_mesh.append(ms.timing()[1])
    mesh = median(t_mesh)
    print(f"volume {n[0]} x {n[1]} x {n[2]} ({nvox * 4 / (1 << 20):.0f} MiB), voxel {a.voxel} m, {a.frames} frames of the synthetic sequence fused at {W} x {H}, "
          f"{fm.recenters} recentrings, min_weight {fm.min_weight}; device outputs; the handle's device time; {a.runs} runs after {a.warmup}")
    print(f"  vdo_mesh_extract, whole volume, {nv} vertices, {nt} triangles (the yardstick)   {stats(t_mesh)}")
    for method, R in cases:
        med = median(t[(method, R)])
        sites, reach, _ = counts[R]
        print(f"  vdo_distance_compute, whole volume, R {R:3d}, method {method}: {sites} sites, {reach} voxels in reach   {stats(t[(method, R)])}  | {med / mesh:.2f} x the mesher"
              f"  | {nvox * 32 / (med * 1e-3) / 1e12:.3f} TB/s over 32 bytes per voxel")
    print(f"  vdo_distance_sample, {npts} device points, {inside} inside the box                 {stats(t_sample)}  | {npts * 16 / (median(t_sample) * 1e-3) / 1e12:.3f} TB/s over 16 bytes per point")
    field.close(); fm.close(); ctx.close()


if __name__ == "__main__":
    main()
