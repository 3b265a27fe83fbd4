"""ctypes handle on the C++ ``System`` (vdo_slam_amd/host/System.{h,cc}): the reference's entry API
``System(settings, RGBD)`` / ``TrackRGBD(im, depth, flow, mask, Tcw_gt, objPose_gt, t, imTraj, nImage)``
(include/System.h:42-53) on HOST images.  Used by bench.py (`value_host_inputs`) and the tests."""
import ctypes as C

import numpy as np

from . import _capi as K

SETTINGS = """%YAML:1.0
Camera.fx: {fx}
Camera.fy: {fy}
Camera.cx: {cx}
Camera.cy: {cy}
Camera.k1: 0.0
Camera.width: {w}
Camera.height: {h}
Camera.fps: 10.0
Camera.bf: {bf}
Camera.RGB: 1
ChooseData: {choose_data}
DepthMapFactor: {dmf}
ThDepthBG: {thbg}
ThDepthOBJ: {thobj}
MaxTrackPointBG: 1200 # 1200 1500 2000
MaxTrackPointOBJ: 800
SFMgThres: {sf_mg_thres} # 0.05
SFDsThres: 0.3
WINDOW_SIZE: {window}
OVERLAP_SIZE: {overlap}
UseSampleFeature: {use_sample_feature}
ORBextractor.nFeatures: {n_features}
ORBextractor.scaleFactor: 1.2
ORBextractor.nLevels: 8
ORBextractor.iniThFAST: 20
ORBextractor.minThFAST: 7
"""


def rectify_keys(left, right, raw_size=None, border=None, classes=None):
    """The Rectify.* lines of a settings file.  left / right: dicts with "K" (fx, fy, cx, cy), "D" (k1, k2, p1, p2[, k3]) and "R" (9 values,
    row-major) of the RAW cameras - Camera.* then describes the rectified one; raw_size = (width, height) of the raw images when it differs
    from Camera.width / height; border: the byte of pixels without a source; classes = 1: the class image is raw too."""
    out = []
    for side, cam in (("Left", left), ("Right", right)):
        for name in ("K", "D", "R"):
            vals = np.asarray(cam[name], np.float64).reshape(-1)
            out.append(f"Rectify.{side}.{name}: [" + ", ".join(repr(float(v)) for v in vals) + "]")
    if raw_size is not None:
        out += [f"Rectify.Width: {int(raw_size[0])}", f"Rectify.Height: {int(raw_size[1])}"]
    if border is not None:
        out.append(f"Rectify.Border: {int(border)}")
    if classes is not None:
        out.append(f"Rectify.Classes: {int(classes)}")
    return "\n".join(out) + "\n"


def write_settings(path, w, h, K4, bf, dmf, thbg, thobj, window=20, overlap=4, choose_data=2, use_sample_feature=0, sf_mg_thres=0.12, n_features=2500, rectify=None):
    """A settings file in the reference's flat YAML dialect (example/kitti-0000-0013.yaml).  rectify: None, or the keyword arguments of
    ``rectify_keys`` as a dict (STEREO systems only: the stereo entries then take raw images)."""
    fx, fy, cx, cy = K4
    with open(path, "w") as f:
        f.write(SETTINGS.format(fx=fx, fy=fy, cx=cx, cy=cy, w=w, h=h, bf=bf, dmf=dmf, thbg=thbg, thobj=thobj, window=window, overlap=overlap, choose_data=choose_data,
                                use_sample_feature=use_sample_feature, sf_mg_thres=sf_mg_thres, n_features=n_features))
        if rectify is not None:
            f.write(rectify_keys(**rectify))
    return str(path)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class System:
    def __init__(self, settings_path, sensor="rgbd"):
        """sensor: "rgbd" (System::RGBD, track_rgbd / track_files) or "stereo" (System::STEREO, track_stereo; optional Stereo.* settings keys)"""
        if sensor not in ("rgbd", "stereo"):
            raise ValueError(f"sensor {sensor!r}: 'rgbd' or 'stereo'")
        L = self._L = K.load_host_lib()
        L.host_system_create.restype = C.c_void_p
        L.host_system_create.argtypes = [C.c_char_p]
        L.host_system_create_stereo.restype = C.c_void_p
        L.host_system_create_stereo.argtypes = [C.c_char_p]
        L.host_system_destroy.argtypes = [C.c_void_p]
        L.host_system_track.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.host_system_motions.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.host_system_refined_poses.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.host_system_save.argtypes = [C.c_void_p, C.c_char_p]
        self._h = (L.host_system_create_stereo if sensor == "stereo" else L.host_system_create)(str(settings_path).encode())
        if not self._h:
            raise K.VdoError("System could not be created (settings file / HIP device)")
        self._T = np.zeros(16, np.float32)

    def track_rgbd(self, im, depth, flow, mask, obj_rows=None, n_images=1 << 30):
        """One TrackRGBD call.  im: [h, w] or [h, w, 3|4] uint8; depth [h, w] float32 (raw on entry, METRES on return, as the
        reference mutates it); flow [h, w, 2] float32; mask [h, w] int32 (recovered labels are written back); obj_rows:
        ground-truth rows [n, L] float32 (row[1] = label) or None.  Returns Tcw 4x4 float32, or None (rejected / failed frame)."""
        h, w = im.shape[:2]
        ch = 1 if im.ndim == 2 else im.shape[2]
        rows = None if obj_rows is None or len(obj_rows) == 0 else np.ascontiguousarray(obj_rows, np.float32)
        rc = self._L.host_system_track(self._h, _ptr(im), ch, _ptr(depth), _ptr(flow), _ptr(mask), w, h, _ptr(rows), 0 if rows is None else rows.shape[0],
                                       0 if rows is None else rows.shape[1], int(n_images), _ptr(self._T))
        return None if rc != 0 else self._T.reshape(4, 4).copy()

    def track_stereo(self, left, right, flow, mask, obj_rows=None, n_images=1 << 30):
        """One TrackStereo call on a STEREO system: left / right [h, w] or [h, w, 3|4] uint8 (rectified), flow and mask as track_rgbd.  The
        disparity is computed on the device and goes straight into the frame's step.  Returns Tcw 4x4 float32, or None."""
        L = self._L
        L.host_system_track_stereo.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        if left.shape != right.shape:
            raise ValueError(f"left {left.shape} and right {right.shape} differ")
        h, w = left.shape[:2]
        ch = 1 if left.ndim == 2 else left.shape[2]
        rows = None if obj_rows is None or len(obj_rows) == 0 else np.ascontiguousarray(obj_rows, np.float32)
        rc = L.host_system_track_stereo(self._h, _ptr(left), _ptr(right), ch, _ptr(flow), _ptr(mask), w, h, _ptr(rows), 0 if rows is None else rows.shape[0],
                                        0 if rows is None else rows.shape[1], int(n_images), _ptr(self._T))
        return None if rc != 0 else self._T.reshape(4, 4).copy()

    def track_stereo_pair(self, left, right, left_next, mask, obj_rows=None, n_images=1 << 30):
        """One TrackStereoPair call on a STEREO system: as track_stereo, with the NEXT left image in place of the flow image - the flow from this
        frame to the next is computed on the device (optional Flow.* settings keys) and goes straight into the frame's step.  Returns Tcw 4x4 float32, or None."""
        L = self._L
        L.host_system_track_stereo_pair.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        if left.shape != right.shape or left.shape != left_next.shape:
            raise ValueError(f"left {left.shape}, right {right.shape} and left_next {left_next.shape} differ")
        h, w = left.shape[:2]
        ch = 1 if left.ndim == 2 else left.shape[2]
        rows = None if obj_rows is None or len(obj_rows) == 0 else np.ascontiguousarray(obj_rows, np.float32)
        rc = L.host_system_track_stereo_pair(self._h, _ptr(left), _ptr(right), _ptr(left_next), ch, _ptr(mask), w, h, _ptr(rows), 0 if rows is None else rows.shape[0],
                                             0 if rows is None else rows.shape[1], int(n_images), _ptr(self._T))
        return None if rc != 0 else self._T.reshape(4, 4).copy()

    def track_stereo_pair_semantic(self, left, right, left_next, classes, obj_rows=None, n_images=1 << 30):
        """One TrackStereoPairSemantic call on a STEREO system: as track_stereo_pair, with a class image (uint8 [h, w], 0 = background) in place of
        the instance mask - the mask is made on the device from the class image and the frame's disparity (connected components; optional Labels.*
        settings keys) and never exists on the host.  Returns Tcw 4x4 float32, or None."""
        L = self._L
        L.host_system_track_stereo_pair_semantic.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                             C.c_int, C.c_void_p]
        if left.shape != right.shape or left.shape != left_next.shape:
            raise ValueError(f"left {left.shape}, right {right.shape} and left_next {left_next.shape} differ")
        h, w = left.shape[:2]
        ch = 1 if left.ndim == 2 else left.shape[2]
        classes = np.ascontiguousarray(classes)
        if classes.dtype != np.uint8 or classes.shape != (h, w):
            raise ValueError(f"classes: {classes.dtype} {classes.shape}, expected uint8 {(h, w)}")
        rows = None if obj_rows is None or len(obj_rows) == 0 else np.ascontiguousarray(obj_rows, np.float32)
        rc = L.host_system_track_stereo_pair_semantic(self._h, _ptr(left), _ptr(right), _ptr(left_next), ch, _ptr(classes), w, h, _ptr(rows), 0 if rows is None else rows.shape[0],
                                                      0 if rows is None else rows.shape[1], int(n_images), _ptr(self._T))
        return None if rc != 0 else self._T.reshape(4, 4).copy()

    def track_stereo_video(self, left, right, left_next, right_next, obj_rows=None, n_images=1 << 30):
        """One TrackStereoVideo call on a STEREO system: the current and the NEXT stereo pair, nothing else.  Both disparities, the flow, the camera
        motion, the class image of the pixels that move against the scene (optional Motion.* settings keys) and the instance mask are made on the
        device.  Returns Tcw 4x4 float32, or None."""
        L = self._L
        L.host_system_track_stereo_video.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                     C.c_void_p]
        if not (left.shape == right.shape == left_next.shape == right_next.shape):
            raise ValueError(f"left {left.shape}, right {right.shape}, left_next {left_next.shape} and right_next {right_next.shape} differ")
        h, w = left.shape[:2]
        ch = 1 if left.ndim == 2 else left.shape[2]
        rows = None if obj_rows is None or len(obj_rows) == 0 else np.ascontiguousarray(obj_rows, np.float32)
        rc = L.host_system_track_stereo_video(self._h, _ptr(left), _ptr(right), _ptr(left_next), _ptr(right_next), ch, w, h, _ptr(rows), 0 if rows is None else rows.shape[0],
                                              0 if rows is None else rows.shape[1], int(n_images), _ptr(self._T))
        return None if rc != 0 else self._T.reshape(4, 4).copy()

    def video_counts(self):
        """What the last track_stereo_video found: (ego-motion inliers, moving pixels after the vote, labels)"""
        L = self._L
        L.host_system_video_counts.argtypes = [C.c_void_p, C.c_void_p]
        out = np.zeros(3, np.int32)
        L.host_system_video_counts(self._h, _ptr(out))
        return tuple(int(v) for v in out)

    def track_files(self, rgb_path, depth_path, flow_path, mask_path, obj_rows=None, n_images=1 << 30):
        """One TrackRGBDFromFiles call: the frame's colour PNG, disparity PNG, .flo and mask text decoded on the device (the reference driver's
        imread / convertTo / readOpticalFlow / LoadMask, example/vdo_slam.cc:104-131) and tracked.  Returns Tcw 4x4 float32, or None."""
        L = self._L
        L.host_system_track_files.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        rows = None if obj_rows is None or len(obj_rows) == 0 else np.ascontiguousarray(obj_rows, np.float32)
        rc = L.host_system_track_files(self._h, str(rgb_path).encode(), str(depth_path).encode(), str(flow_path).encode(), str(mask_path).encode(), _ptr(rows),
                                       0 if rows is None else rows.shape[0], 0 if rows is None else rows.shape[1], int(n_images), _ptr(self._T))
        return None if rc != 0 else self._T.reshape(4, 4).copy()

    def rectified_left(self, w, h):
        """The rectified grey left image of the last stereo call of a System with Rectify.* keys: uint8 [h, w] (Camera.height, Camera.width)"""
        L = self._L
        L.host_system_rectified_left.argtypes = [C.c_void_p, C.c_void_p]
        out = np.zeros((h, w), np.uint8)
        if L.host_system_rectified_left(self._h, _ptr(out)) != 0:
            raise K.VdoError("System.rectified_left: no rectifier (Rectify.* settings keys) or the download failed")
        return out

    def frame_images(self, w, h):
        """Tracking::SyncFrameState()'s converted depth map (metres) and repaired mask of the last frame: (depth [h, w] f32, mask [h, w] i32)"""
        L = self._L
        L.host_system_frame_images.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        d = np.zeros((h, w), np.float32); m = np.zeros((h, w), np.int32)
        if L.host_system_frame_images(self._h, _ptr(d), _ptr(m)) != 0:
            raise K.VdoError("System.frame_images failed")
        return d, m

    def set_defer(self, on=True):
        """Throughput mode: the object stage of a frame ends inside the next track_rgbd call (same results one frame later)."""
        self._L.host_system_set_defer.argtypes = [C.c_void_p, C.c_int]
        self._L.host_system_set_defer(self._h, int(bool(on)))

    def flush(self):
        self._L.host_system_flush.argtypes = [C.c_void_p]
        if self._L.host_system_flush(self._h) != 0:
            raise K.VdoError("System flush failed")

    def motions(self, cap=32):
        sl = np.zeros(cap, np.int32); Hm = np.zeros((cap, 16), np.float32)
        n = self._L.host_system_motions(self._h, cap, _ptr(sl), _ptr(Hm))
        return [(int(sl[a]), Hm[a].reshape(4, 4).copy()) for a in range(min(n, cap))]

    def refined_poses(self, n):
        rf = np.zeros((n, 16), np.float32)
        m = self._L.host_system_refined_poses(self._h, n, _ptr(rf))
        return rf[:min(m, n)].reshape(-1, 4, 4)

    def tracks(self, dynamic=False):
        """(off, frame, feat, obj): tracklet t = pairs [off[t], off[t+1]) of (frame, feature index); obj = object id per dynamic tracklet"""
        L = self._L
        L.host_system_tracks.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), K.c_int32_p, K.c_int32_p, K.c_int32_p, K.c_int32_p]
        sz = (C.c_int64 * 2)()
        if L.host_system_tracks(self._h, int(dynamic), sz, None, None, None, None) != 0:
            raise K.VdoError("System.tracks failed")
        nt, npairs = int(sz[0]), int(sz[1])
        off = np.zeros(nt + 1, np.int32); fr = np.zeros(max(npairs, 1), np.int32); ft = np.zeros(max(npairs, 1), np.int32); ob = np.zeros(max(nt, 1), np.int32)
        ip = lambda a: a.ctypes.data_as(K.c_int32_p)
        if L.host_system_tracks(self._h, int(dynamic), sz, ip(off), ip(fr), ip(ft), ip(ob)) != 0:
            raise K.VdoError("System.tracks failed")
        return off, fr[:npairs], ft[:npairs], (ob[:nt] if dynamic else None)

    def frame_state(self, what, rows):
        """Tracking::SyncFrameState() + a flat copy (host_system_frame_state): what = 0 static set [10][n], 1 object set [12][n], 2 per object [n][19],
        3 samples [8][n], 4 scalars [17]; returns (n, flat float32 array)"""
        L = self._L
        L.host_system_frame_state.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        n = L.host_system_frame_state(self._h, what, None, 0)
        if n < 0:
            raise K.VdoError("System.frame_state failed")
        buf = np.zeros(max(rows * n, 1), np.float32)
        if L.host_system_frame_state(self._h, what, _ptr(buf), buf.size) != n:
            raise K.VdoError("System.frame_state failed")
        return n, buf[:rows * n]

    def map_export(self, what):
        """flat copy of the Map in the reference's format (host_system_map_export): 0 vmCameraPose [F][16], 1 vmCameraPose_RF, 2 vmRigidMotion [n][16], 3 vmRigidMotion_RF,
        4 vnRMLabel [n], 5 vp3DPointSta [n][3], 6 vp3DPointDyn [n][3], 7 motions per frame [F-1]"""
        L = self._L
        L.host_system_map_export.restype = C.c_long
        L.host_system_map_export.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
        n = L.host_system_map_export(self._h, what, None, 0)
        if n < 0:
            raise K.VdoError("System.map_export failed")
        buf = np.zeros(max(n, 1), np.float32)
        if L.host_system_map_export(self._h, what, _ptr(buf), n) != n:
            raise K.VdoError("System.map_export failed")
        return buf[:n]

    def save(self, path):
        self._L.host_system_save(self._h, str(path).encode())

    def dense_info(self):
        """The dense map of a system whose settings carry Dense.VoxelSize: dict(origin, recenters, kept_points, counts = (updated, masked, occluded)
        voxels of the last frame), or None when the system has no mapper (Tracking::dense() is null)."""
        L = self._L
        L.host_system_dense_info.argtypes = [C.c_void_p, C.c_void_p]
        out = np.zeros(8, np.int64)
        if L.host_system_dense_info(self._h, _ptr(out)) != 0:
            return None
        return dict(origin=tuple(int(v) for v in out[:3]), recenters=int(out[3]), kept_points=int(out[4]), counts=tuple(int(v) for v in out[5:8]))

    def save_dense_map(self, path):
        """System::SaveDenseMap: the points kept so far and the surface in the volume as a binary little-endian PLY (``dense.read_ply`` reads it).
        False without a mapper or when the file cannot be written."""
        L = self._L
        L.host_system_save_dense_map.argtypes = [C.c_void_p, C.c_char_p]
        return L.host_system_save_dense_map(self._h, str(path).encode()) == 0

    def save_dense_mesh(self, path):
        """System::SaveDenseMesh: the mesh pieces kept so far and the mesh of the whole volume as a binary little-endian PLY (``mesh.read_ply`` reads
        it).  False without a mapper, without ``Dense.Mesh: 1`` or when the file cannot be written."""
        L = self._L
        L.host_system_save_dense_mesh.argtypes = [C.c_void_p, C.c_char_p]
        return L.host_system_save_dense_mesh(self._h, str(path).encode()) == 0

    def render_dense_view(self, T):
        """System::RenderDenseView: what the dense map predicts a camera at T (4 x 4, world -> camera) would see, at the camera's image size:
        (depth [h, w] f32 in metres, normals [h, w, 3] f32), or None when the system has no mapper."""
        L = self._L
        L.host_system_render_dense_view.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        Tc = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
        wh = np.zeros(2, np.int32)
        if L.host_system_render_dense_view(self._h, _ptr(Tc), _ptr(wh), None, None) == 1:
            return None
        d = np.zeros((int(wh[1]), int(wh[0])), np.float32); n = np.zeros((int(wh[1]), int(wh[0]), 3), np.float32)
        rc = L.host_system_render_dense_view(self._h, _ptr(Tc), _ptr(wh), _ptr(d), _ptr(n))
        if rc != 0:
            raise K.VdoError("System.render_dense_view failed")
        return d, n

    def dense_colour_counts(self):
        """With ``Dense.Colour: 1``: the voxels the last frame (coloured, skipped by the mask, skipped as outside the band); None without a mapper or
        without the key."""
        L = self._L
        L.host_system_dense_colour_counts.argtypes = [C.c_void_p, C.c_void_p]
        out = np.zeros(3, np.int64)
        rc = L.host_system_dense_colour_counts(self._h, _ptr(out))
        if rc == 1:
            return None
        if rc != 0:
            raise K.VdoError("System.dense_colour_counts failed")
        return tuple(int(v) for v in out)

    def render_dense_colour(self, T):
        """System::RenderDenseColour: the colour image that belongs to ``render_dense_view(T)``'s depth image: rgba [h, w, 4] uint8 (alpha 0 where there
        is no surface or no colour), or None when the system has no mapper or no ``Dense.Colour: 1``."""
        L = self._L
        L.host_system_render_dense_colour.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        Tc = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
        wh = np.zeros(2, np.int32)
        if L.host_system_render_dense_colour(self._h, _ptr(Tc), _ptr(wh), None) == 1:
            return None
        rgba = np.zeros((int(wh[1]), int(wh[0]), 4), np.uint8)
        if L.host_system_render_dense_colour(self._h, _ptr(Tc), _ptr(wh), _ptr(rgba)) != 0:
            raise K.VdoError("System.render_dense_colour failed")
        return rgba

    def dense_clearance(self, points):
        """System::DenseClearance with ``Dense.Distance: 1``: how much room world points [n, 3] have to the static scene -> (metres float32 [n]: the
        exact Euclidean distance to the nearest voxel at a zero crossing, +inf beyond ``Dense.Distance.Radius``, NaN outside the volume; state uint8 [n]:
        0 unknown, 1 free, 2 inside, 255 outside the volume), or None when the system has no mapper or no ``Dense.Distance: 1``.  The field is computed
        when the map was fused or moved since the last query; ``self.distance_computes`` is the number of fields computed so far."""
        L = self._L
        L.host_system_dense_clearance.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
        m = np.zeros(len(p), np.float32); st = np.zeros(len(p), np.uint8); computes = np.zeros(1, np.int64)
        rc = L.host_system_dense_clearance(self._h, len(p), _ptr(p), _ptr(m), _ptr(st), _ptr(computes))
        if rc == 1:
            return None
        if rc != 0:
            raise K.VdoError("System.dense_clearance failed")
        self.distance_computes = int(computes[0])
        return m, st

    def object_clearances(self):
        """System::ObjectClearances: [(mod_label, metres)] for every live object model - the clearance at the world position of the model's origin -, or
        None without ``Dense.Distance: 1`` or without an object mapper."""
        L = self._L
        L.host_system_object_clearances.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        labels = np.zeros(64, np.int32); m = np.zeros(64, np.float32); count = np.zeros(1, np.int32)
        rc = L.host_system_object_clearances(self._h, 64, _ptr(labels), _ptr(m), _ptr(count))
        if rc == 1:
            return None
        if rc != 0:
            raise K.VdoError("System.object_clearances failed")
        return [(int(labels[i]), m[i]) for i in range(min(64, int(count[0])))]

    @staticmethod
    def _align_report(r):
        return dict(iterations=int(r[0]), status=int(r[1]), used=int(r[2]), rms_first=float(r[3]), rms_last=float(r[4]), xi=r[5:11].copy())

    def dense_alignment(self):
        """With Dense.Align.Iterations > 0: (report dict of the last frame's alignment against the map - iterations, status, used, rms_first, rms_last,
        xi -, the pose [4, 4] f32 the frame was fused with), or None when there has been none."""
        L = self._L
        L.host_system_dense_alignment.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        r = np.zeros(11, np.float64); fused = np.zeros(16, np.float32)
        rc = L.host_system_dense_alignment(self._h, _ptr(r), _ptr(fused))
        if rc == 1:
            return None
        if rc != 0:
            raise K.VdoError("System.dense_alignment failed")
        return self._align_report(r), fused.reshape(4, 4)

    def last_dense_alignment(self):
        """System::LastDenseAlignment: the report dict of AlignDenseView or of the last aligned frame, whichever came later; None when there has been none."""
        L = self._L
        L.host_system_last_dense_alignment.argtypes = [C.c_void_p, C.c_void_p]
        r = np.zeros(11, np.float64)
        rc = L.host_system_last_dense_alignment(self._h, _ptr(r))
        if rc == 1:
            return None
        if rc != 0:
            raise K.VdoError("System.last_dense_alignment failed")
        return self._align_report(r)

    def align_dense_view(self, T, depth, mask=None):
        """System::AlignDenseView + LastDenseAlignment: depth [h, w] f32 metres and mask [h, w] i32 (or None) at the camera's image size aligned against
        the map's view at T (4 x 4, world -> camera): (refined T [4, 4] f32, report dict), or None when the system has no mapper."""
        L = self._L
        L.host_system_align_dense_view.argtypes = [C.c_void_p] * 6
        Tc = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
        d = np.ascontiguousarray(depth, np.float32); m = np.ascontiguousarray(mask, np.int32) if mask is not None else None
        out = np.zeros(16, np.float32); r = np.zeros(11, np.float64)
        rc = L.host_system_align_dense_view(self._h, _ptr(Tc), _ptr(d), _ptr(m) if m is not None else None, _ptr(out), _ptr(r))
        if rc == 1:
            return None
        if rc != 0:
            raise K.VdoError("System.align_dense_view failed")
        return out.reshape(4, 4), self._align_report(r)

    @staticmethod
    def _photo_report(r):
        return dict(iterations=int(r[0]), status=int(r[1]), used_geo=int(r[2]), used_photo=int(r[3]), rms_geo_first=float(r[4]), rms_geo_last=float(r[5]), rms_photo_first=float(r[6]),
                    rms_photo_last=float(r[7]), xi=r[8:14].copy())

    def dense_photo_alignment(self):
        """With Dense.Align.Photo: (joint report dict of the last frame's alignment - iterations, status, used_geo, used_photo, rms_geo_first / last in
        metres, rms_photo_first / last in grey levels, xi -, the pose [4, 4] f32 the frame was fused with), or None when there has been none."""
        L = self._L
        L.host_system_dense_photo_alignment.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        r = np.zeros(14, np.float64); fused = np.zeros(16, np.float32)
        rc = L.host_system_dense_photo_alignment(self._h, _ptr(r), _ptr(fused))
        if rc == 1:
            return None
        if rc != 0:
            raise K.VdoError("System.dense_photo_alignment failed")
        return self._photo_report(r), fused.reshape(4, 4)

    def last_dense_photo_alignment(self):
        """System::LastDensePhotoAlignment: the joint report dict of AlignDenseViewPhoto or of the last frame, whichever came later; None when there has been none."""
        L = self._L
        L.host_system_last_dense_photo_alignment.argtypes = [C.c_void_p, C.c_void_p]
        r = np.zeros(14, np.float64)
        rc = L.host_system_last_dense_photo_alignment(self._h, _ptr(r))
        if rc == 1:
            return None
        if rc != 0:
            raise K.VdoError("System.last_dense_photo_alignment failed")
        return self._photo_report(r)

    def align_dense_view_photo(self, T, depth, mask, image):
        """System::AlignDenseViewPhoto + LastDensePhotoAlignment: as align_dense_view, with the frame's image uint8 [h, w] or [h, w, 1 | 3 | 4] (in the order
        of Camera.RGB) for the photometric term against the tracker's model frame: (refined T [4, 4] f32, joint report dict), or None without a mapper
        or without Dense.Align.Photo."""
        L = self._L
        L.host_system_align_dense_view_photo.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p]
        Tc = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
        d = np.ascontiguousarray(depth, np.float32); m = np.ascontiguousarray(mask, np.int32) if mask is not None else None
        img = np.ascontiguousarray(image, np.uint8)
        channels = 1 if img.ndim == 2 else img.shape[2]
        if channels not in (1, 3, 4) or img.shape[:2] != d.shape:
            raise ValueError(f"image: {img.shape}, depth {d.shape}")
        out = np.zeros(16, np.float32); r = np.zeros(14, np.float64)
        rc = L.host_system_align_dense_view_photo(self._h, _ptr(Tc), _ptr(d), _ptr(m) if m is not None else None, _ptr(img), channels, _ptr(out), _ptr(r))
        if rc == 1:
            return None
        if rc != 0:
            raise K.VdoError("System.align_dense_view_photo failed")
        return out.reshape(4, 4), self._photo_report(r)

    def object_motions(self, cap=64):
        """The motions of the last frame as the object mapper takes them (host_system_object_motions): [(mod_label, sem_label, n_inliers, H [4, 4] f32)]
        in the tracker's order - mod_label the tracking id, sem_label the label the object's pixels carry in the frame's mask, H the world-frame motion
        from the last frame to this one."""
        L = self._L
        L.host_system_object_motions.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        mod = np.zeros(cap, np.int32); sem = np.zeros(cap, np.int32); inl = np.zeros(cap, np.int32); H = np.zeros((cap, 4, 4), np.float32)
        n = min(cap, L.host_system_object_motions(self._h, cap, _ptr(mod), _ptr(sem), _ptr(inl), _ptr(H)))
        return [(int(mod[a]), int(sem[a]), int(inl[a]), H[a].copy()) for a in range(n)]

    def object_info(self, cap=256):
        """System::ObjectModelInfo: dict(models = [(mod_label, live, frames fused, points)] - finished first, then live -, dropped, skipped), or None
        when the system has no object mapper (no Dense.Objects.VoxelSize)."""
        L = self._L
        L.host_system_object_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        rows = np.zeros((cap, 4), np.int64); counts = np.zeros(2, np.int64)
        n = L.host_system_object_info(self._h, cap, _ptr(rows), _ptr(counts))
        if n == -1:
            return None
        if n < 0:
            raise K.VdoError("System.object_info failed")
        return dict(models=[(int(r[0]), bool(r[1]), int(r[2]), int(r[3])) for r in rows[:min(n, cap)]], dropped=int(counts[0]), skipped=int(counts[1]))

    def save_object_meshes(self, prefix):
        """System::SaveObjectMeshes: <prefix>_<mod_label>_mesh.ply per model in the object frame (``mesh.read_ply`` reads them).  False without an
        object mapper, without ``Dense.Mesh: 1`` or when a file cannot be written."""
        L = self._L
        L.host_system_save_object_meshes.argtypes = [C.c_void_p, C.c_char_p]
        return L.host_system_save_object_meshes(self._h, str(prefix).encode()) == 0

    def save_object_maps(self, prefix):
        """System::SaveObjectMaps: <prefix>_<mod_label>.ply per model in the object frame and <prefix>_poses.txt.  False without an object mapper or
        when a file cannot be written."""
        L = self._L
        L.host_system_save_object_maps.argtypes = [C.c_void_p, C.c_char_p]
        return L.host_system_save_object_maps(self._h, str(prefix).encode()) == 0

    def render_object_view(self, mod_label, T, w, h):
        """System::RenderObjectView: what the model of the live object mod_label predicts a camera at T (4 x 4, world -> camera) would see, at the
        camera's image size (w, h): (depth [h, w] f32, normals [h, w, 3] f32 in the object frame), or None without an object mapper or such a model."""
        L = self._L
        L.host_system_render_object_view.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        Tc = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
        d = np.zeros((h, w), np.float32); n = np.zeros((h, w, 3), np.float32)
        rc = L.host_system_render_object_view(self._h, int(mod_label), _ptr(Tc), _ptr(d), _ptr(n))
        if rc == 1:
            return None
        if rc != 0:
            raise K.VdoError("System.render_object_view failed")
        return d, n

    def last_depth_mask(self, w, h):
        """The resident depth (metres) and mask of the last frame as the step left them - what the dense mapper fused: (depth [h, w] f32, mask [h, w] i32)"""
        L = self._L
        L.host_system_last_depth_mask.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        d = np.zeros((h, w), np.float32); m = np.zeros((h, w), np.int32)
        if L.host_system_last_depth_mask(self._h, _ptr(d), _ptr(m)) != 0:
            raise K.VdoError("System.last_depth_mask failed")
        return d, m

    def close(self):
        if self._h:
            self._L.host_system_destroy(self._h); self._h = None

    def __del__(self):
        try: self.close()
        except Exception: pass
