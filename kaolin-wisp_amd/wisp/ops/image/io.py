"""Image files <-> arrays (wisp/ops/image/io.py:71-84: load_rgb).  The reference decodes with torchvision; here PIL decodes when
it imports, and a small built-in reader covers non-interlaced 8-bit grey / RGB / RGBA PNG (what NeRF-synthetic data is) with the
standard library alone when it does not.  The built-in pair is slow (a Python loop per byte for the average and Paeth filters) and exact."""
import struct
import zlib

import numpy as np

_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 2: 3, 6: 4}            # PNG colour type -> channels (grey, RGB, RGBA)


def _have_pil():
    try:
        import PIL.Image          # noqa: F401
        return True
    except Exception:
        return False


def _paeth(a, b, c):
    """PNG's Paeth predictor on int16 arrays: whichever of left / up / upper-left lies nearest to a + b - c, ties in that order."""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def read_png(path):
    """u8 [H, W, C] (C = 1, 3 or 4) of a non-interlaced 8-bit grey / RGB / RGBA PNG; all five filter types.  Anything else
    (palette, 16 bit, grey + alpha, Adam7) raises ValueError."""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:8] != _PNG_MAGIC:
        raise ValueError(f"{path}: not a PNG file")
    pos, header, idat = 8, None, []
    while pos + 8 <= len(raw):
        length, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + length]
        if len(body) != length:
            raise ValueError(f"{path}: truncated chunk {kind!r}")
        pos += 12 + length
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    if header is None:
        raise ValueError(f"{path}: no IHDR chunk")
    w, h, depth, ctype, _, _, interlace = header
    if depth != 8 or ctype not in _CHANNELS or interlace != 0:
        raise ValueError(f"{path}: the built-in PNG reader handles non-interlaced 8-bit grey / RGB / RGBA only "
                         f"(bit depth {depth}, colour type {ctype}, interlace {interlace}); install Pillow for other files")
    ch = _CHANNELS[ctype]
    stride = w * ch
    data = zlib.decompress(b"".join(idat))
    if len(data) != h * (stride + 1):
        raise ValueError(f"{path}: {len(data)} bytes of image data, expected {h * (stride + 1)}")
    rows = np.frombuffer(data, dtype=np.uint8).reshape(h, stride + 1)
    out = np.zeros((h, stride), dtype=np.uint8)
    zero = np.zeros(stride, dtype=np.uint8)
    for y in range(h):
        ftype, line = int(rows[y, 0]), rows[y, 1:]
        up = out[y - 1] if y > 0 else zero
        if ftype == 0:
            out[y] = line
        elif ftype == 2:
            out[y] = line + up                                            # u8 arithmetic wraps mod 256, as the format asks
        elif ftype == 1:
            # x[i] = line[i] + x[i - ch]: a running sum per channel
            out[y] = np.cumsum(line.reshape(w, ch), axis=0, dtype=np.uint8).reshape(-1)
        elif ftype in (3, 4):
            # each byte depends on the decoded byte one pixel to its left: a plain loop over Python ints (faster than numpy here)
            cur, ln, upb = bytearray(stride), line.tobytes(), up.tobytes()
            if ftype == 3:
                for i in range(stride):
                    a = cur[i - ch] if i >= ch else 0
                    cur[i] = (ln[i] + ((a + upb[i]) >> 1)) & 255
            else:
                for i in range(stride):
                    a, c = (cur[i - ch], upb[i - ch]) if i >= ch else (0, 0)
                    b = upb[i]
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    cur[i] = (ln[i] + (a if (pa <= pb and pa <= pc) else (b if pb <= pc else c))) & 255
            out[y] = np.frombuffer(bytes(cur), dtype=np.uint8)
        else:
            raise ValueError(f"{path}: unknown filter type {ftype} in row {y}")
    return out.reshape(h, w, ch)


def write_png(path, img, filter_type=0, level=6):
    """Write u8 [H, W] / [H, W, 1 | 3 | 4] as an 8-bit PNG with the standard library alone; every row uses `filter_type` (0..4)."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8:
        raise ValueError(f"write_png takes uint8, got {img.dtype}")
    if img.ndim == 2:
        img = img[..., None]
    h, w, ch = img.shape
    ctype = {1: 0, 3: 2, 4: 6}[ch]
    cur = img.reshape(h, w * ch).astype(np.int16)
    up = np.concatenate([np.zeros((1, w * ch), np.int16), cur[:-1]], 0)
    left = np.concatenate([np.zeros((h, ch), np.int16), cur[:, :-ch]], 1)
    diag = np.concatenate([np.zeros((h, ch), np.int16), up[:, :-ch]], 1)
    if filter_type == 0:
        res = cur
    elif filter_type == 1:
        res = cur - left
    elif filter_type == 2:
        res = cur - up
    elif filter_type == 3:
        res = cur - ((left + up) >> 1)
    elif filter_type == 4:
        res = cur - _paeth(left, up, diag)
    else:
        raise ValueError("filter_type must be 0..4")
    body = np.concatenate([np.full((h, 1), filter_type, np.uint8), (res & 0xFF).astype(np.uint8)], 1).tobytes()

    def chunk(kind, payload):
        return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(_PNG_MAGIC + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(body, level)) + chunk(b"IEND", b""))


def load_u8(path, use_pil=None):
    """u8 [H, W, C] of an image file, C as the file has it (1, 3 or 4).  use_pil: None = PIL when it imports."""
    if use_pil is None:
        use_pil = _have_pil()
    if not use_pil:
        return read_png(path)
    import PIL.Image
    with PIL.Image.open(path) as im:
        if im.mode not in ("L", "RGB", "RGBA"):
            im = im.convert("RGBA" if ("A" in im.mode or "transparency" in im.info) else "RGB")
        arr = np.array(im, dtype=np.uint8)
    return arr[..., None] if arr.ndim == 2 else arr


def save_u8(path, img, use_pil=None):
    """Write u8 [H, W, 1 | 3 | 4] as PNG: PIL when it imports, the built-in writer otherwise."""
    if use_pil is None:
        use_pil = _have_pil()
    if not use_pil:
        return write_png(path, img)
    import PIL.Image
    img = np.ascontiguousarray(img)
    PIL.Image.fromarray(img[..., 0] if img.ndim == 3 and img.shape[2] == 1 else img).save(path, format="PNG")


def load_rgb(path, normalize=True):
    """np.array [H, W, C]: fp32 in [0, 1] (`u8 / 255.0` in fp32, as the reference's `img.float() / 255.0`) or the u8 values."""
    img = load_u8(path)
    if normalize:
        return img.astype(np.float32) / np.float32(255.0)
    return img
