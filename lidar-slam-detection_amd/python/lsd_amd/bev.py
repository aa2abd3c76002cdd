"""Bird's-eye intensity image of a dense map: the front end of lio_bev (csrc/bev.hip), shaped like the reference's
tools/postprocessing/convert_cloud_image.py.

    python -m lsd_amd.bev -i map.pcd -w 50 -r 25 -o out_dir        # writes out_dir/bev.png (16-bit grey)

preprocess / convert take and return what the reference's functions do; from_cloud runs both on the device from points or from a
lio.Cloud without a PCD round trip.  The PCD reader and the PNG writer / reader need numpy and the standard library only."""
import argparse
import os
import struct
import sys
import zlib

import numpy as np

# ---- PCD ------------------------------------------------------------------------------------------------------------------------------------
_PCD_TYPES = {("F", 4): "f4", ("F", 8): "f8", ("I", 1): "i1", ("I", 2): "i2", ("I", 4): "i4", ("I", 8): "i8", ("U", 1): "u1", ("U", 2): "u2",
              ("U", 4): "u4", ("U", 8): "u8"}


def read_pcd(path):
    """n x 4 f32 (x, y, z, intensity) of an ascii or binary PCD file; the fields may come in any order, other fields are skipped.
    ValueError for binary_compressed data, a missing field or a malformed header."""
    with open(path, "rb") as f:
        raw = f.read()
    head, pos = {}, 0
    while True:
        end = raw.find(b"\n", pos)
        if end < 0:
            raise ValueError(f"{path}: no DATA line in the PCD header")
        line = raw[pos:end].decode("ascii", "replace").strip()
        pos = end + 1
        if not line or line.startswith("#"):
            continue
        key, _, rest = line.partition(" ")
        head[key.upper()] = rest.split()
        if key.upper() == "DATA":
            break
    try:
        fields, sizes, types = head["FIELDS"], [int(s) for s in head["SIZE"]], head["TYPE"]
        counts = [int(c) for c in head.get("COUNT", ["1"] * len(fields))]
        n = int(head["POINTS"][0]) if "POINTS" in head else int(head["WIDTH"][0]) * int(head.get("HEIGHT", ["1"])[0])
        data = head["DATA"][0].lower()
    except (KeyError, IndexError, ValueError) as e:
        raise ValueError(f"{path}: malformed PCD header ({e})") from None
    if not (len(fields) == len(sizes) == len(types) == len(counts)):
        raise ValueError(f"{path}: FIELDS, SIZE, TYPE and COUNT disagree")
    for want in ("x", "y", "z", "intensity"):
        if want not in fields:
            raise ValueError(f"{path}: the PCD file has no field '{want}'")
    if data == "binary_compressed":
        raise ValueError(f"{path}: binary_compressed PCD data is not supported (save the cloud as binary or ascii)")
    out = np.zeros((n, 4), np.float32)
    if data == "ascii":
        starts = np.concatenate([[0], np.cumsum(counts)])
        rows = raw[pos:].split()
        width = int(starts[-1])
        if len(rows) < n * width:
            raise ValueError(f"{path}: {len(rows)} values for {n} points of {width}")
        tab = np.array(rows[:n * width], dtype=object).reshape(n, width)
        for k, want in enumerate(("x", "y", "z", "intensity")):
            j = fields.index(want)
            col = tab[:, int(starts[j])]
            out[:, k] = np.array([float(v) for v in col], np.float64).astype(_PCD_TYPES.get((types[j], sizes[j]), "f8")).astype(np.float32)
    elif data == "binary":
        names, formats = [], []
        for name, s, t, c in zip(fields, sizes, types, counts):
            if (t, s) not in _PCD_TYPES:
                raise ValueError(f"{path}: field {name} has the unknown type {t}{s}")
            names.append(name if name not in names else f"{name}#{len(names)}")
            formats.append(_PCD_TYPES[(t, s)] if c == 1 else (_PCD_TYPES[(t, s)], (c,)))
        dt = np.dtype({"names": names, "formats": formats})
        if len(raw) - pos < n * dt.itemsize:
            raise ValueError(f"{path}: {len(raw) - pos} data bytes for {n} points of {dt.itemsize}")
        rec = np.frombuffer(raw, dt, n, pos)
        for k, want in enumerate(("x", "y", "z", "intensity")):
            col = rec[want]
            out[:, k] = (col if col.ndim == 1 else col[:, 0]).astype(np.float32)
    else:
        raise ValueError(f"{path}: unknown PCD DATA kind '{data}'")
    return out


# ---- PNG (16-bit greyscale) -----------------------------------------------------------------------------------------------------------------
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def write_png16(path, image, level=6):
    """image: h x w uint16 -> a 16-bit greyscale PNG (filter 0 on every row)"""
    img = np.ascontiguousarray(image)
    if img.ndim != 2 or img.dtype != np.uint16 or img.size == 0:
        raise ValueError("write_png16: a non-empty h x w uint16 image is required")
    h, w = img.shape
    rows = np.zeros((h, 1 + 2 * w), np.uint8)
    rows[:, 1:] = img.astype(">u2").view(np.uint8).reshape(h, 2 * w)
    body = _PNG_MAGIC + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + \
        _chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(body)


def read_png16(path):
    """the h x w uint16 image of a 16-bit greyscale, non-interlaced PNG (all five row filters)"""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:8] != _PNG_MAGIC:
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, hdr = 8, [], None
    while pos + 8 <= len(raw):
        (ln,), kind = struct.unpack(">I", raw[pos:pos + 4]), raw[pos + 4:pos + 8]
        body = raw[pos + 8:pos + 8 + ln]
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
        pos += 12 + ln
    if hdr is None or hdr[2:] != (16, 0, 0, 0, 0):
        raise ValueError(f"{path}: only 16-bit greyscale, non-interlaced PNG files are read")
    w, h = hdr[0], hdr[1]
    data = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, 1 + 2 * w)
    out = np.zeros((h, 2 * w), np.uint8)
    prev = np.zeros(2 * w, np.int32)
    for r in range(h):
        ft, line = int(data[r, 0]), data[r, 1:].astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        else:
            cur = np.zeros(2 * w, np.int32)
            for i in range(2 * w):
                a = cur[i - 2] if i >= 2 else 0
                b, c = prev[i], (prev[i - 2] if i >= 2 else 0)
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) >> 1
                elif ft == 4:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                else:
                    raise ValueError(f"{path}: unknown PNG row filter {ft}")
                cur[i] = (line[i] + pred) & 255
        out[r] = cur
        prev = cur
    return out.view(">u2").astype(np.uint16).reshape(h, w)


# ---- the reference's functions --------------------------------------------------------------------------------------------------------------
def _unpack(handle):
    info = handle.info()
    keys, inten, zs = handle.pixels()
    w = info["image_w"]
    xs, ys = (keys % w).astype(np.int64), (keys // w).astype(np.int64)
    meta = {"x_min": info["x_min"], "x_max": info["x_max"], "y_min": info["y_min"], "y_max": info["y_max"], "pixel_per_meter": info["pixel_per_meter"]}
    return xs, ys, zs, inten, int(info["image_w"]), int(info["image_h"]), meta


def process_points(points, pixel_per_meter, handle=None):
    """load_pointcloud + filter_noise + scatter over n x 4 points: (xs, ys, zs, intensity, image_w, image_h, meta)"""
    from . import lio

    h = handle if handle is not None else lio.BevImage()
    h.preprocess_host(points, pixel_per_meter)
    return _unpack(h)


def preprocess(filename, pixel_per_meter):
    """the reference's preprocess: the occupied pixels of a PCD file after the noise filter, with their mean z and intensity"""
    return process_points(read_pcd(filename), pixel_per_meter)


def convert(xs, ys, zs, intensity, image_w, image_h, window, pixel_per_meter, handle=None):
    """the reference's convert: the patch-equalised uint16 image of a list of distinct pixels"""
    from . import lio

    xs, ys = np.asarray(xs, np.int64).reshape(-1), np.asarray(ys, np.int64).reshape(-1)
    image_w, image_h = int(image_w), int(image_h)
    _check_window(window, pixel_per_meter)
    if len(xs) != len(ys) or len(xs) != len(np.asarray(intensity).reshape(-1)):
        raise ValueError("convert: xs, ys and intensity must have one entry per pixel")
    if len(xs) and (xs.min() < 0 or ys.min() < 0 or xs.max() >= image_w or ys.max() >= image_h):
        raise ValueError("convert: a pixel lies outside the image")
    if image_w < 1 or image_h < 1 or image_w * image_h > 0xFFFFFFFF:
        raise ValueError("convert: the image does not fit the 32-bit pixel key")
    keys = ys * image_w + xs
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    if len(keys) > 1 and np.any(keys[1:] == keys[:-1]):
        raise ValueError("convert: the pixels must be distinct (the output of preprocess is)")
    h = handle if handle is not None else lio.BevImage()
    h.upload_pixels(keys.astype(np.uint32), np.asarray(intensity, np.float32).reshape(-1)[order],
                    None if zs is None else np.asarray(zs, np.float32).reshape(-1)[order], image_w, image_h)
    return h.convert(window, pixel_per_meter)


def from_cloud(cloud, window=50.0, pixel_per_meter=25, handle=None):
    """the image of n x 4 points (x, y, z, intensity) or of a lio.Cloud as it lies on the device"""
    from . import lio

    _check_window(window, pixel_per_meter)
    h = handle if handle is not None else lio.BevImage()
    if isinstance(cloud, lio.Cloud):
        h.preprocess_cloud(cloud, pixel_per_meter)
    else:
        h.preprocess_host(cloud, pixel_per_meter)
    return h.convert(window, pixel_per_meter)


def _check_window(window, pixel_per_meter):
    if not (np.isfinite(pixel_per_meter) and pixel_per_meter > 0):
        raise ValueError("pixel_per_meter must be positive")
    if not (np.isfinite(window) and int(window * pixel_per_meter) >= 2):
        raise ValueError("window x pixel_per_meter must give a patch of at least 2 pixels")


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m lsd_amd.bev", description="project the pointcloud to BEV")
    parser.add_argument("-i", "--data_path", required=True, help="pointcloud path")
    parser.add_argument("-w", "--window", default=50.0, type=float, help="sliding window to equalization (m)")
    parser.add_argument("-r", "--pixel_per_meter", default=25, type=int, help="pixel per meter")
    parser.add_argument("-o", "--output", required=True, help="output path for save")
    args = parser.parse_args(argv)
    # every argument is checked before any device work
    try:
        _check_window(args.window, args.pixel_per_meter)
    except ValueError as e:
        parser.error(str(e))
    if not os.path.isfile(args.data_path):
        parser.error(f"{args.data_path}: no such pointcloud file")
    if not os.path.isdir(args.output):
        parser.error(f"{args.output}: no such output directory")
    print("loading {}".format(args.data_path))
    points = read_pcd(args.data_path)
    print("start to process total {} points".format(len(points)))
    from . import lio

    h = lio.BevImage()
    info = h.preprocess_host(points, args.pixel_per_meter)
    print("after noise filter: {} points".format(info["n_kept"]))
    print("after scatter: {} points".format(info["n_pixels"]))
    image = h.convert(args.window, args.pixel_per_meter)
    print("image size: {}, {}".format(image.shape[1], image.shape[0]))
    write_png16(os.path.join(args.output, "bev.png"), image)
    return 0


if __name__ == "__main__":
    sys.exit(main())
