"""Writers of the reference driver's per-frame files (example/vdo_slam.cc:104-131) from numpy arrays: PNG (grey / RGB / RGBA, 8 or 16 bit,
a chosen filter type per row, the stream split over IDAT chunks), Middlebury .flo and the instance-mask text LoadMask reads.  For tests
and tools that need a sequence on disk."""
import struct
import zlib

import numpy as np


def png_bytes(arr, bit_depth=8, filters=(0,), n_idat=2, level=6):
    """PNG file bytes of a grey (h, w) or colour (h, w, 3|4) image; row y uses filters[y % len(filters)] (PNG spec 9.2)."""
    h, w = arr.shape[:2]
    ch = 1 if arr.ndim == 2 else arr.shape[2]
    ctype = {1: 0, 3: 2, 4: 6}[ch]
    raw = np.ascontiguousarray(arr.astype(">u2" if bit_depth == 16 else np.uint8)).reshape(h, -1).view(np.uint8).reshape(h, -1).astype(np.int32)
    bpp = ch * bit_depth // 8
    rows = []
    prev = np.zeros(raw.shape[1], np.int32)
    for y in range(h):
        ft = filters[y % len(filters)]
        cur = raw[y]
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])[: cur.size]
        c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])[: cur.size]
        if ft == 0:
            pred = 0
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = prev
        elif ft == 3:
            pred = (a + prev) // 2
        else:
            p = a + prev - c
            pa, pb, pc = np.abs(p - a), np.abs(p - prev), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
        rows.append(bytes([ft]) + ((cur - pred) & 255).astype(np.uint8).tobytes())
        prev = cur

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    z = zlib.compress(b"".join(rows), level)
    cut = [len(z) * k // n_idat for k in range(n_idat + 1)]
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, bit_depth, ctype, 0, 0, 0))
    for k in range(n_idat):
        out += chunk(b"IDAT", z[cut[k]:cut[k + 1]])
    return out + chunk(b"IEND", b"")


def flo_bytes(flow):
    """Middlebury .flo of a (h, w, 2) float32 flow field: "PIEH" (202021.25), width, height, then the field row by row."""
    h, w = flow.shape[:2]
    return struct.pack("<fii", 202021.25, w, h) + np.ascontiguousarray(flow, np.float32).tobytes()


def mask_text(mask):
    """The instance-mask text of an (h, w) integer image: one line of space-separated integers per image row."""
    return ("\n".join(" ".join(map(str, row)) for row in np.asarray(mask).tolist()) + "\n").encode()


def write_frame(prefix, rgb, disparity_u16, flow, mask, filters=(1, 2, 3, 4, 0)):
    """The four files of one frame: <prefix>.png (colour), <prefix>_depth.png (16-bit disparity), <prefix>.flo, <prefix>_mask.txt.
    Returns their paths (rgb, depth, flow, mask)."""
    paths = (f"{prefix}.png", f"{prefix}_depth.png", f"{prefix}.flo", f"{prefix}_mask.txt")
    blobs = (png_bytes(rgb, 8, filters), png_bytes(disparity_u16, 16, filters), flo_bytes(flow), mask_text(mask))
    for p, b in zip(paths, blobs):
        with open(p, "wb") as f:
            f.write(b)
    return paths
