"""numpy restatement of the reference tool chain's yuv422p* -> yuv444p* step (libswscale's generic scaler:
luma unscaled, chroma 2x up along x with the 4:2:0 path's bicubic, unscaled along y).  Built on the oracle's
horizontal filter, oracle.sws_chroma_filter(w, 1 << 14), and the output rules of yuv2plane1
(output.c:320-330 for 10/12 bits, output.c:395-403 with the constant dither 64 for 8 bits).
PARITY UNPINNED: no libswscale binary or vector exists here; tests/test_upconv422.py ties this restatement to
oracle.sws_420_to_444 (whose vertical rows are normalised to 4096) on chroma that is constant along y."""
import numpy as np


def dtype_of(depth):
    return np.uint8 if depth == 8 else np.dtype("<u2")


def chroma_422_to_444(oracle, c, w, depth):
    """c: (H, ceil(w/2)) chroma plane -> (H, w) samples of the yuv444p* plane."""
    f, p = oracle.sws_chroma_filter(w, 1 << 14)
    c = np.asarray(c)
    assert c.shape[1] == (w + 1) // 2, (c.shape, w)
    hsh = 7 if depth == 8 else depth - 1
    out = np.empty((c.shape[0], w), dtype_of(depth))
    for r0 in range(0, c.shape[0], 256):                       # row blocks: 8K pictures stay small in memory
        s = c[r0: r0 + 256].astype(np.int64)
        hv = np.zeros((s.shape[0], w), np.int64)
        for k in range(f.shape[1]):                            # hScale8To15_c / hScale16To15_c
            hv += s[:, p + k] * f[:, k].astype(np.int64)
        hv = np.minimum(hv >> hsh, 32767).astype(np.int16).astype(np.int64)   # stored as int16_t: wraps below -32768
        o = (hv + 64) >> 7 if depth == 8 else (hv + (1 << (14 - depth))) >> (15 - depth)
        out[r0: r0 + 256] = np.clip(o, 0, (1 << depth) - 1)
    return out


def sws_422_to_444(oracle, y, u, v, depth):
    """yuv422p* frame (Y (H,W); U, V (H, ceil(W/2))) -> (3,H,W) yuv444p* samples."""
    y = np.asarray(y)
    w = y.shape[1]
    return np.stack([y.astype(dtype_of(depth)), chroma_422_to_444(oracle, u, w, depth), chroma_422_to_444(oracle, v, w, depth)])


def yuv422(seed, h, w, depth, kind="noise"):
    """A yuv422p* test frame: 'noise' (samples of the depth), 'ramp', or 'full16' (16-bit samples whatever the depth)."""
    rng = np.random.default_rng(seed)
    dt = dtype_of(depth)
    cw = (w + 1) // 2
    if kind in ("noise", "full16"):
        top = 1 << (16 if kind == "full16" and depth > 8 else depth)
        return [rng.integers(0, top, s).astype(dt) for s in ((h, w), (h, cw), (h, cw))]
    yy, xx = np.mgrid[0:h, 0:cw]
    ramp = ((3 * xx + 5 * yy + seed) % (1 << depth)).astype(dt)
    return [rng.integers(0, 1 << depth, (h, w)).astype(dt), ramp, ramp[:, ::-1].copy()]
