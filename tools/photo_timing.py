"""Timing record of the photometric aligner beside the aligner (a record, not a gate): one vdo_photo_linearise_frame and one
vdo_align_linearise_frame of the same 1242 x 375 resident frame at subsample 1, each against a model of the frame's size, in the same program; the
device time by the handles' own events (first command to last kernel), median of 30 calls after 5.  Writes profiles/photo_timing.txt.

    python tools/photo_timing.py [runs] [out]
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import align_ref as A          # noqa: E402
from tests import photo_ref as P          # noqa: E402

W, H = 1242, 375
K4 = (721.5377, 721.5377, 609.5593, 172.854)
WARM = 5
F = np.float32


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "photo_timing.txt")
    from vdo_slam_amd.align import Aligner
    from vdo_slam_amd.ba import Context
    from vdo_slam_amd.photo import PhotoAligner
    I4 = np.eye(4, dtype=F)
    T_true = A.exp_se3(np.array([0.02, -0.015, 0.01, 0.002, -0.003, 0.004])).astype(F)      # a quarter of a pixel footprint (Z / fx = 6.9 mm x 3) off the model
    D, If = P.wall_render(T_true, W, H, K4)
    Dm, Im = P.wall_render(I4, W, H, K4)
    Gm = np.broadcast_to(np.array([0.0, 0.0, -1000.0], F), (H, W, 3)).copy()
    img = np.rint(If).astype(np.uint8)
    ctx = Context(0)
    prm = dict(min_depth=0.0, max_depth=10.0, max_dist=0.4)
    ph = PhotoAligner(ctx, W, H, K4, max_diff=255.0, **prm)
    al = Aligner(ctx, W, H, K4, **prm)
    ph.set_image(img); ph.set_model(Dm, np.rint(Im).astype(F), K4, I4)
    al.set_model(Dm, Gm, K4, I4)
    L = ph._L
    fh = C.c_void_p()
    assert L.vdo_frame_images_create(ctx._h, C.c_int(W), C.c_int(H), C.byref(fh)) == 0
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    flow = np.zeros((H, W, 2), F); mask = np.zeros((H, W), np.int32)
    assert L.vdo_frame_images_upload(fh, D.ctypes.data_as(fp), flow.ctypes.data_as(fp), mask.ctypes.data_as(ip)) == 0

    def measure(handle):
        dev, wall = [], []
        for k in range(WARM + runs):
            sums, counts = handle.linearise_frame(fh, I4)
            w, d = handle.timing()
            if k >= WARM:
                dev.append(d); wall.append(w)
        return np.array(dev), np.array(wall), counts

    rows = []
    for name, handle in (("vdo_photo_linearise_frame", ph), ("vdo_align_linearise_frame", al)):
        dev, wall, counts = measure(handle)
        rows.append((name, dev, wall, counts))
    # the joint solve of the same frame: both linearisations per round
    ph2 = PhotoAligner(ctx, W, H, K4, max_diff=255.0, max_iterations=10, eps=1e-7, **prm)
    ph2.set_image(img); ph2.set_model(Dm, np.rint(Im).astype(F), K4, I4)
    solve = []
    for k in range(WARM + runs):
        T, rep, trace = ph2.solve_frame(al, fh, 0.01, I4)
        if k >= WARM:
            solve.append(ph2.timing())
    solve = np.array(solve)
    tiles = (-(-W // 8)) * (-(-H // 8))
    lines = [f"tools/photo_timing.py {runs}   (one MI355X; {W} x {H} resident frame, subsample 1, models of the frame's size, a textured wall 5 m away; the handles' own events, "
             f"first command to last kernel; {WARM} warm-up calls, median of {runs})",
             "kernels: profiles/photo_resources.txt", ""]
    for name, dev, wall, counts in rows:
        lines.append(f"  {name:<28} device median {np.median(dev):.4f} ms  min {dev.min():.4f}  max {dev.max():.4f}  | wall median {np.median(wall):.4f} ms  | used {counts[0]}, no depth "
                     f"{counts[1]}, masked {counts[2]}, no model {counts[3]}, far {counts[4]} of {W * H} samples")
    lines.append(f"  {'vdo_photo_solve_frame + geo':<28} wall median {np.median(solve[:, 0]):.4f} ms  | its photometric linearisations' device time median {np.median(solve[:, 1]):.4f} ms  | "
                 f"{rep['iterations']} rounds, status {rep['status']}, used {rep['used_geo']} + {rep['used_photo']}, rms {rep['rms_geo_first']:.4f} -> {rep['rms_geo_last']:.4f} m, "
                 f"{rep['rms_photo_first']:.2f} -> {rep['rms_photo_last']:.2f} levels")
    ratio = np.median(rows[0][1]) / np.median(rows[1][1])
    lines += ["", f"a linearisation of either kind is its row kernel, two launches of the tree ({tiles} tiles: {-(-(1 << (tiles - 1).bit_length()) // 256)} workgroups, then one) and one "
              f"256-byte download; the photometric one takes {ratio:.2f} x the aligner's device time (four 8-byte gathers per sample against one 4-byte and one 12-byte gather).",
              "A round of the joint solve costs the sum of the two, each with its own host-synchronous round trip."]
    text = "\n".join(lines) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    print(text)
    L.vdo_frame_images_destroy(fh)
    ph.close(); ph2.close(); al.close(); ctx.close()


if __name__ == "__main__":
    main()
