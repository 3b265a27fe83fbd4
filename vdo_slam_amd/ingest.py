"""ctypes handle on the dataset ingest of the C-ABI (``vdo_ingest_*``, vdo_slam_amd/csrc/ingest.hip): one frame's mask text, .flo
payload and inflated PNG scanlines decoded on the device into the images ``FramePipeline.step`` takes.  ``inflate_png`` is the host
half of the PNG path (DatasetIO's InflatePNG: chunk walk + zlib, scanlines left filtered)."""
import ctypes as C

import numpy as np

from . import _capi as K

MASK, FLO, DEPTH, COLOR = 0, 1, 2, 3


class PngScanlinesC(C.Structure):
    _fields_ = [("data", C.c_void_p), ("bytes", C.c_int64), ("width", C.c_int32), ("height", C.c_int32), ("bit_depth", C.c_int32), ("channels", C.c_int32)]


def inflate_png(path):
    """(scanlines uint8 [height * (1 + width * channels * bit_depth / 8)], width, height, bit_depth, channels), or None when the file is refused."""
    L = K.load_host_lib()
    L.host_io_inflate_png.restype = C.c_long
    L.host_io_inflate_png.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_void_p, C.c_long]
    dims = (C.c_int * 4)()
    with open(path, "rb") as f:
        head = f.read(29)
    cap = 0
    if len(head) == 29 and head[12:16] == b"IHDR":                  # room for the scanlines the header announces: one inflate
        w, h, bd, ct = int.from_bytes(head[16:20], "big"), int.from_bytes(head[20:24], "big"), head[24], head[25]
        cap = h * (1 + w * {0: 1, 2: 3, 6: 4}.get(ct, 4) * max(bd, 8) // 8) if w <= 1 << 15 and h <= 1 << 15 else 0
    buf = np.empty(max(cap, 1), np.uint8)
    n = L.host_io_inflate_png(str(path).encode(), dims, buf.ctypes.data_as(C.c_void_p), cap)
    if n < 0:
        return None
    if n > cap:
        buf = np.empty(n, np.uint8)
        L.host_io_inflate_png(str(path).encode(), dims, buf.ctypes.data_as(C.c_void_p), n)
    return buf[:n], int(dims[1]), int(dims[0]), int(dims[2]), int(dims[3])


def _lib():
    L = K.lib()
    L.vdo_ingest_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.vdo_ingest_destroy.argtypes = [C.c_void_p]
    L.vdo_ingest_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(PngScanlinesC), C.POINTER(PngScanlinesC), C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vdo_ingest_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    return L


class Ingest:
    """A handle sized for width x height images.  ``frame`` writes into DEVICE buffers given as pointers (e.g. ``tensor.data_ptr()``)."""

    def __init__(self, ctx, width, height):
        self._L = _lib()
        self._h = C.c_void_p()
        K.check(self._L.vdo_ingest_create(ctx._h, int(width), int(height), C.byref(self._h)))
        self._ctx = ctx
        ctx._retain()
        self.width, self.height = int(width), int(height)

    @staticmethod
    def _png(p):
        if p is None:
            return None, None
        data, w, h, bd, ch = p
        data = np.ascontiguousarray(data, np.uint8)
        return PngScanlinesC(data.ctypes.data, data.size, w, h, bd, ch), data

    def frame(self, mask_text=None, flo=None, depth=None, color=None, rgb_order=1, gray_out=0, depth_out=0, flow_out=0, mask_out=0):
        """mask_text / flo: bytes; depth / color: (scanlines, width, height, bit_depth, channels) as inflate_png returns them; *_out: device
        pointers (0 = skip that part).  Raises VdoError (message from the library) when the frame is refused."""
        d, keep_d = self._png(depth)
        c, keep_c = self._png(color)
        mt = None if mask_text is None else C.create_string_buffer(bytes(mask_text), max(len(mask_text), 1))
        fl = None if flo is None else C.create_string_buffer(bytes(flo), max(len(flo), 1))
        K.check(self._L.vdo_ingest_frame(self._h, None if mt is None else C.cast(mt, C.c_void_p), 0 if mask_text is None else len(mask_text),
                                         None if fl is None else C.cast(fl, C.c_void_p), 0 if flo is None else len(flo),
                                         None if d is None else C.byref(d), None if c is None else C.byref(c), int(rgb_order),
                                         C.c_void_p(gray_out or None), C.c_void_p(depth_out or None), C.c_void_p(flow_out or None), C.c_void_p(mask_out or None)))

    def last_timing(self):
        """(wall ms of the last frame call, device ms from the first upload to the last kernel, device ms of the kernels alone)"""
        ms = (C.c_double * 3)()
        K.check(self._L.vdo_ingest_last_timing(self._h, ms))
        return tuple(ms)

    def close(self):
        if self._h:
            self._L.vdo_ingest_destroy(self._h)
            self._h = C.c_void_p()
            self._ctx._release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
