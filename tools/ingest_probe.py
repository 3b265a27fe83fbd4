"""Per-frame cost of reading one KITTI-sized frame from disk (1242x375: RGB PNG, 16-bit disparity PNG, .flo, instance-mask text), three ways:
  host    - DatasetIO's full host decode (ReadPNG x2, ReadOpticalFlow, LoadMask), what the driver does before TrackRGBD;
  inflate - the host half of the device path (InflatePNG x2 + reading the .flo and the mask text);
  device  - vdo_ingest_frame on those bytes: wall time of the call, device time (uploads + kernels) and kernel time.
Prints one JSON line (ms per frame, medians over --reps).  python tools/ingest_probe.py [--reps 30]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    from vdo_slam_amd import _capi as K, dataset_files as DF, synth, synth_seq as SQ
    from vdo_slam_amd.ba import Context
    from vdo_slam_amd.ingest import Ingest, inflate_png

    W, H = synth.KITTI_W, synth.KITTI_H
    fr = SQ.render_frame(0, SQ.camera_poses(1), SQ.default_objects(), flow_sigma=0.1)
    g = fr["gray"].astype(np.int32)
    rgb = np.stack([g, 255 - g // 2, (g * 7) % 256], -1).astype(np.uint8)
    tmp = tempfile.mkdtemp()
    prgb, pdep, pflo, pmask = DF.write_frame(os.path.join(tmp, "f"), rgb, np.clip(fr["depth_raw"], 0, 65535).astype(np.uint16), fr["flow"], fr["mask"])
    L = K.load_host_lib()
    L.host_io_read_flo.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_void_p]
    L.host_io_load_mask.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    L.host_io_read_png.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.c_void_p]
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    im = np.zeros((H, W, 3), np.uint8); dep = np.zeros((H, W), np.float32); flo = np.zeros((H, W, 2), np.float32); msk = np.zeros((H, W), np.int32)
    dims = (C.c_int * 3)()

    def host():
        assert L.host_io_read_png(prgb.encode(), 0, dims, p(im)) == 0 and L.host_io_read_png(pdep.encode(), 1, dims, p(dep)) == 0
        assert L.host_io_read_flo(pflo.encode(), dims, p(flo)) == 0 and L.host_io_load_mask(pmask.encode(), H, W, p(msk)) == 0

    def inflate():
        c, d = inflate_png(prgb), inflate_png(pdep)
        with open(pflo, "rb") as f: fb = f.read()
        with open(pmask, "rb") as f: mb = f.read()
        return c, d, fb, mb

    ctx = Context(0)
    ing = Ingest(ctx, W, H)
    out = dict(gray=torch.empty((H, W), dtype=torch.uint8, device="cuda"), depth=torch.empty((H, W), device="cuda"),
               flow=torch.empty((H, W, 2), device="cuda"), mask=torch.empty((H, W), dtype=torch.int32, device="cuda"))
    c, d, fb, mb = inflate()
    t_host, t_inf, t_dev, t_dev_gpu, t_kern = [], [], [], [], []
    for r in range(a.reps + 3):
        t0 = time.perf_counter(); host(); t1 = time.perf_counter(); inflate(); t2 = time.perf_counter()
        ing.frame(mask_text=mb, flo=fb, depth=d, color=c, rgb_order=1, gray_out=out["gray"].data_ptr(), depth_out=out["depth"].data_ptr(),
                  flow_out=out["flow"].data_ptr(), mask_out=out["mask"].data_ptr())
        wall, dev, kern = ing.last_timing()
        if r >= 3:
            t_host.append(1e3 * (t1 - t0)); t_inf.append(1e3 * (t2 - t1)); t_dev.append(wall); t_dev_gpu.append(dev); t_kern.append(kern)
    part = {}                                                          # kernel time of each part alone
    for name, kw in (("mask", dict(mask_text=mb, mask_out=out["mask"].data_ptr())), ("depth_png", dict(depth=d, depth_out=out["depth"].data_ptr())),
                     ("rgb_png", dict(color=c, gray_out=out["gray"].data_ptr())), ("flo", dict(flo=fb, flow_out=out["flow"].data_ptr()))):
        v = []
        for r in range(a.reps + 3):
            ing.frame(**kw)
            if r >= 3:
                v.append(ing.last_timing()[1])
        part[name] = round(float(np.median(v)), 3)
    assert np.array_equal(out["mask"].cpu().numpy(), msk) and np.array_equal(out["depth"].cpu().numpy(), dep) and np.array_equal(out["flow"].cpu().numpy(), flo)
    med = lambda v: round(float(np.median(v)), 3)
    print(json.dumps(dict(frame=f"{W}x{H}", reps=a.reps, host_datasetio_ms=med(t_host), host_read_inflate_ms=med(t_inf), device_call_wall_ms=med(t_dev),
                          device_upload_kernels_ms=med(t_dev_gpu), device_kernels_ms=med(t_kern), device_ms_per_part_alone=part, mask_text_bytes=len(mb))))
    ing.close()


if __name__ == "__main__":
    main()
