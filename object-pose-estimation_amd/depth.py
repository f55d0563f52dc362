"""Depth images on the host: 16-bit PGM files (what a recorded sensor stream is kept as) and a point-set renderer for
synthetic frames.  The conversion itself is Context.depth_to_cloud (ope_depth_to_cloud, csrc/depth.hip)."""
from __future__ import annotations

import numpy as np

from . import DepthParams

# The reference's three intrinsics sets, (fx, fy, cx, cy), DetectAndLocalize/src/datagrabber.cpp:133-136, 146-149, 159-162.
SENSOR_INTRINSICS = {
    "euclid": (306.178, 306.929, 158.523, 122.747),
    "kinect": (525.0, 525.0, 319.5, 239.5),
    "astra": (570.342, 570.342, 314.5, 235.5),
}


def preset_params(sensor: str = "kinect") -> DepthParams:
    """The preset of ope_depth_sensor_params without loading the library: the reference's cx / fx act on the ROW and its
    cy / fy on the COLUMN (datagrabber.cpp:86,170-171), scale 1000, z_max 2.0."""
    fx, fy, cx, cy = SENSOR_INTRINSICS[sensor]
    return DepthParams(f_row=fx, c_row=cx, f_col=fy, c_col=cy, scale=1000.0, z_max=2.0)


def write_pgm16(path: str, image) -> None:
    """A (rows, cols) uint16 image as a binary PGM ("P5", maxval 65535, big-endian samples)."""
    image = np.asarray(image)
    if image.dtype != np.uint16 or image.ndim != 2:
        raise ValueError("write_pgm16: expected a 2-D uint16 image")
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n65535\n" % (image.shape[1], image.shape[0]))
        f.write(image.astype(">u2").tobytes())


def read_pgm16(path: str) -> np.ndarray:
    """A binary PGM ("P5", maxval <= 65535) as a (rows, cols) uint16 image.  Samples are one byte for maxval < 256, else two,
    big-endian.  ValueError for anything else: another magic number, a header that is not three positive integers, a
    missing separator, too few sample bytes."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] != b"P5":
        raise ValueError("read_pgm16: not a binary PGM (P5)")
    pos, vals = 2, []
    while len(vals) < 3:
        start = pos
        while pos < len(data) and data[pos:pos + 1] in b" \t\r\n":
            pos += 1
        if pos < len(data) and data[pos:pos + 1] == b"#":
            while pos < len(data) and data[pos:pos + 1] != b"\n":
                pos += 1
            continue
        if pos == start:
            raise ValueError("read_pgm16: malformed header")
        end = pos
        while end < len(data) and data[end:end + 1].isdigit():
            end += 1
        if end == pos or end - pos > 9:
            raise ValueError("read_pgm16: malformed header")
        vals.append(int(data[pos:end]))
        pos = end
    cols, rows, maxval = vals
    if cols < 1 or rows < 1 or not 1 <= maxval <= 65535:
        raise ValueError("read_pgm16: bad size or maxval")
    if pos >= len(data) or data[pos:pos + 1] not in b" \t\r\n":
        raise ValueError("read_pgm16: no separator after maxval")
    pos += 1
    width = 1 if maxval < 256 else 2
    need = rows * cols * width
    if len(data) - pos < need:
        raise ValueError("read_pgm16: truncated file")
    img = np.frombuffer(data, ">u2" if width == 2 else np.uint8, rows * cols, pos)
    return img.astype(np.uint16).reshape(rows, cols)


def render_depth(points, params, rows: int, cols: int) -> np.ndarray:
    """A z-buffer of a point set: every finite point with z > 0 lands on the pixel its projection rounds to
    (row = y * f_row / z + c_row, col = x * f_col / z + c_col: the inverse of the conversion, the reference's swapped
    principal point included) with depth = round(z * scale), the nearest point wins, holes are 0.  Depths outside 1 .. 65535 and
    pixels outside the image are dropped.  (A point set has no closed surfaces: a far point shows wherever no nearer point
    fell on its pixel.)"""
    p = np.asarray(points, np.float64)
    p = p[np.isfinite(p).all(axis=1) & (p[:, 2] > 0)]
    r = np.rint(p[:, 1] * float(params.f_row) / p[:, 2] + float(params.c_row)).astype(np.int64)
    c = np.rint(p[:, 0] * float(params.f_col) / p[:, 2] + float(params.c_col)).astype(np.int64)
    d = np.rint(p[:, 2] * float(params.scale)).astype(np.int64)
    img = np.full(rows * cols, 65536, np.int64)
    ok = (r >= 0) & (r < rows) & (c >= 0) & (c < cols) & (d >= 1) & (d <= 65535)
    np.minimum.at(img, r[ok] * cols + c[ok], d[ok])
    img[img == 65536] = 0
    return img.astype(np.uint16).reshape(rows, cols)


def write_ppm8(path: str, bgr) -> None:
    """A (rows, cols, 3) uint8 image in OpenCV's channel order B, G, R as a binary PPM ("P6", maxval 255; the file's samples are
    R, G, B)."""
    bgr = np.asarray(bgr)
    if bgr.dtype != np.uint8 or bgr.ndim != 3 or bgr.shape[2] != 3:
        raise ValueError("write_ppm8: expected a (rows, cols, 3) uint8 image")
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (bgr.shape[1], bgr.shape[0]))
        f.write(np.ascontiguousarray(bgr[:, :, ::-1]).tobytes())


def read_ppm8(path: str) -> np.ndarray:
    """A binary PPM ("P6", maxval <= 255) as a (rows, cols, 3) uint8 image with the channels B, G, R, as cv::imread gives it.
    ValueError for anything else."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] != b"P6":
        raise ValueError("read_ppm8: not a binary PPM (P6)")
    # the header is a PGM's but for the magic number: read it as one
    import re
    m = re.match(rb"P6(?:\s+|#[^\n]*\n)+(\d{1,9})(?:\s+|#[^\n]*\n)+(\d{1,9})(?:\s+|#[^\n]*\n)+(\d{1,9})\s", data)
    if not m:
        raise ValueError("read_ppm8: malformed header")
    cols, rows, maxval = (int(v) for v in m.groups())
    if cols < 1 or rows < 1 or not 1 <= maxval <= 255:
        raise ValueError("read_ppm8: bad size or maxval (8-bit samples only)")
    if len(data) - m.end() < 3 * rows * cols:
        raise ValueError("read_ppm8: truncated file")
    rgb = np.frombuffer(data, np.uint8, 3 * rows * cols, m.end()).reshape(rows, cols, 3)
    return np.ascontiguousarray(rgb[:, :, ::-1])
