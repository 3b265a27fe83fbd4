"""ORB descriptor matcher: gated brute-force Hamming search on the device (``vdo_orb_match`` /
``vdo_orb_match_extractors`` of libvdo_hip.so; semantics in include/vdo_slam_hip.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K

TH_LOW = 50           # ORB-SLAM2's ORBmatcher thresholds
TH_HIGH = 100


class MatchSetC(C.Structure):
    _fields_ = [("n", C.c_int32), ("desc", K.c_uint8_p), ("x", K.c_float_p), ("y", K.c_float_p),
                ("octave", K.c_int32_p), ("is_device", C.c_int32)]


class MatchParamsC(C.Structure):
    _fields_ = [("max_distance", C.c_int32), ("ratio", C.c_float), ("window", C.c_float),
                ("max_octave_diff", C.c_int32), ("cross_check", C.c_int32), ("chunk_rows", C.c_int32)]


_declared = False


def _lib():
    global _declared
    L = K.lib()
    if not _declared:
        vp, ip = C.c_void_p, K.c_int32_p
        L.vdo_orb_match.argtypes = [vp, C.POINTER(MatchSetC), C.POINTER(MatchSetC), C.POINTER(MatchParamsC), ip, ip, ip, ip]
        L.vdo_orb_match.restype = C.c_int
        L.vdo_orb_match_extractors.argtypes = [vp, vp, C.POINTER(MatchParamsC), ip, ip, ip, ip, C.c_int32]
        L.vdo_orb_match_extractors.restype = C.c_int
        _declared = True
    return L


def params(max_distance=256, ratio=0.0, window=-1.0, max_octave_diff=-1, cross_check=False, chunk_rows=0) -> MatchParamsC:
    """Defaults switch every gate and filter off: the plain nearest neighbour."""
    return MatchParamsC(int(max_distance), float(ratio), float(window), int(max_octave_diff), int(bool(cross_check)), int(chunk_rows))


def _set(d):
    """``vdo_match_set`` of a dict shaped like ``ORBextractor.__call__``'s output; returns (struct, keepalive)."""
    desc = np.ascontiguousarray(d["desc"], dtype=np.uint8).reshape(-1, 32)
    n = desc.shape[0]
    keep = [desc if n else np.zeros((1, 32), np.uint8)]           # (a descriptor pointer is never null, even for no rows)
    s = MatchSetC(n, keep[0].ctypes.data_as(K.c_uint8_p), None, None, None, 0)
    for k, dt, cp in (("x", np.float32, K.c_float_p), ("y", np.float32, K.c_float_p), ("octave", np.int32, K.c_int32_p)):
        if d.get(k) is None:
            continue
        a = np.ascontiguousarray(d[k], dtype=dt)
        if a.shape != (n,):
            raise ValueError(f"{k}: shape {a.shape}, {n} descriptor rows")
        keep.append(a if n else np.zeros(1, dt))
        setattr(s, k, keep[-1].ctypes.data_as(cp))
    return s, keep


def _outputs(n):
    return [np.zeros(max(n, 1), np.int32) for _ in range(3)], C.c_int32()


def match(ctx, q, t, **prm):
    """Match ``q`` against ``t`` (dicts with ``desc`` [n, 32] uint8 and optionally ``x``, ``y``, ``octave``).  Keyword parameters
    as :func:`params`.  Returns ``(train_idx, best_dist, second_dist, n_matches)``, int32 arrays of ``len(q["desc"])``."""
    qs, keep_q = _set(q)
    ts, keep_t = _set(t)
    p = params(**prm)
    (idx, best, second), m = _outputs(qs.n)
    K.check(_lib().vdo_orb_match(ctx._h, C.byref(qs), C.byref(ts), C.byref(p), idx.ctypes.data_as(K.c_int32_p), best.ctypes.data_as(K.c_int32_p),
                                 second.ctypes.data_as(K.c_int32_p), C.byref(m)))
    n = qs.n
    return idx[:n], best[:n], second[:n], m.value


def match_extractors(orb_q, orb_t, **prm):
    """The same between the keypoints of the last extraction of two :class:`vdo_slam_amd.frontend.ORBextractor` objects, in the order
    they were returned; descriptors and keypoints stay on the device."""
    p = params(**prm)
    L = _lib()
    nq = C.c_int()
    L.vdo_orb_last_keypoints.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    K.check(L.vdo_orb_last_keypoints(orb_q._h, C.byref(nq)))
    n = nq.value
    (idx, best, second), m = _outputs(n)
    K.check(L.vdo_orb_match_extractors(orb_q._h, orb_t._h, C.byref(p), idx.ctypes.data_as(K.c_int32_p), best.ctypes.data_as(K.c_int32_p),
                                       second.ctypes.data_as(K.c_int32_p), C.byref(m), n))
    return idx[:n], best[:n], second[:n], m.value
