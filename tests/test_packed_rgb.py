"""Packed RGB front end: rgb24 / bgr24 / argb / rgba / abgr / bgra, rgb48* / bgr48* / rgba64* / bgra64* (LE and BE) and
rgb0 / bgr0 / 0rgb / 0bgr sources.  What the reference tool chain does with them before encode2():
av_find_best_pix_fmt_of_2 / get_pix_fmt_score (libavutil/pixdesc.c:2714-2873) over ffv2enc.c:596-601 pick gbrp for
8-bit and gbrp12le for 16-bit packed RGB, alpha dropped; libswscale's *unscaled* converters then run:
  rgbToPlanarRgbWrapper (libswscale/swscale_unscaled.c:1147-1190, dispatched at :2015-2017) with packedtogbr24p
  (:1118-1146): a byte permutation into G, B, R planes; argb / abgr skip the first byte of every pixel;
  Rgb16ToPlanarRgb16Wrapper (:674-732, dispatched at :1987-1999) with packed16togbra16 (:540-672): big-endian samples
  byte-swapped, every sample >> (16 - depth), alpha dropped (a gbrp10le encoder gets >> 6 from the same code).
packed_to_gbrp() below restates those lines; the HIP kernel must be byte-equal to it.  DELIBERATE DEVIATION:
rgb0 / bgr0 / 0rgb / 0bgr pass the dispatch test at :2015 but land in rgbToPlanarRgbWrapper's default: branch, which
writes nothing -- there is no reference output to match.  They are converted as rgba / bgra / argb / abgr with the
padding byte ignored, and held here to that definition only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_PINNED, FRAME_YUV420, FRAME_REGISTER, FRAME_YUV422, FRAME_NV, FRAME_NV_VU, FRAME_PACKED = 1, 2, 4, 8, 16, 32, 64
# name -> (AVPixelFormat value (libavutil/pixfmt.h), bytes per sample, components, B first, leading byte, big-endian)
FMTS = {
    "rgb24": (2, 1, 3, False, False, False), "bgr24": (3, 1, 3, True, False, False),
    "argb": (25, 1, 4, False, True, False), "rgba": (26, 1, 4, False, False, False),
    "abgr": (27, 1, 4, True, True, False), "bgra": (28, 1, 4, True, False, False),
    "rgb48be": (34, 2, 3, False, False, True), "rgb48le": (35, 2, 3, False, False, False),
    "bgr48be": (59, 2, 3, True, False, True), "bgr48le": (60, 2, 3, True, False, False),
    "rgba64be": (106, 2, 4, False, False, True), "rgba64le": (107, 2, 4, False, False, False),
    "bgra64be": (108, 2, 4, True, False, True), "bgra64le": (109, 2, 4, True, False, False),
    "0rgb": (120, 1, 4, False, True, False), "rgb0": (121, 1, 4, False, False, False),
    "0bgr": (122, 1, 4, True, True, False), "bgr0": (123, 1, 4, True, False, False),
}
PIX = {"gbrp": 73, "gbrp10le": 77, "gbrp12le": 137, "yuv444p": 5, "yuv444p10le": 70, "yuv444p12le": 133, "gray": 8}
DEPTH = {"gbrp": 8, "gbrp10le": 10, "gbrp12le": 12}


def src_flags(fmt):
    return FRAME_PACKED | FMTS[fmt][0] << 16


def packed_to_gbrp(src, fmt, depth):
    """numpy restatement of libswscale's unscaled packed RGB -> gbrp* step: src is an (h, w, C) array holding the
    format's bytes as they lie in memory (uint8, or uint16 in the format's byte order) -> (3, h, w) G, B, R planes."""
    _, bps, nc, bgr, lead, be = FMTS[fmt]
    src = np.ascontiguousarray(src)
    h, w = src.shape[:2]
    raw = src.view(np.uint8).reshape(h, w, nc * bps)
    if bps == 1:
        # packedtogbr24p (swscale_unscaled.c:1118-1146): src++ for alpha_first (argb / abgr), then dest[k][x] = src[k]
        # into dst201 (rgb: R -> plane 2, G -> 0, B -> 1) or dst102 (bgr: B -> plane 1, G -> 0, R -> 2), :1150-1184
        assert depth == 8
        comp = [raw[:, :, int(lead) + k] for k in range(3)]
    else:
        # packed16togbra16 (:540-672): av_bswap16 on a swapped (big-endian) source, then >> (16 - bpc); dst2013 (rgb)
        # / dst1023 (bgr) as above, :677-678, 714-726; alpha (component 3) dropped
        s = raw.reshape(h, w, nc, 2).astype(np.uint16)
        val = (s[..., 0] << 8 | s[..., 1]) if be else (s[..., 1] << 8 | s[..., 0])
        val = val >> (16 - depth)
        comp = [val[:, :, k] for k in range(3)]
    r, g, b = (comp[2], comp[1], comp[0]) if bgr else (comp[0], comp[1], comp[2])
    out = np.stack([g, b, r])
    return out.astype(np.uint8 if depth == 8 else np.uint16)


def packed_dtype(fmt):
    bps, be = FMTS[fmt][1], FMTS[fmt][5]
    return np.dtype(np.uint8) if bps == 1 else np.dtype(">u2" if be else "<u2")


def packed_frame(fmt, seed, h, w, kind="noise"):
    """(h, w, C) packed frame of random (or ramp) samples, alpha / padding bytes random too."""
    rng = np.random.default_rng(seed)
    bps, nc = FMTS[fmt][1], FMTS[fmt][2]
    top = 1 << (8 * bps)
    if kind == "noise":
        v = rng.integers(0, top, (h, w, nc))
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        v = np.stack([(3 * xx + 5 * yy + 41 * k + seed) * (1 if bps == 1 else 97) % top for k in range(nc)], axis=-1)
        v = v ^ rng.integers(0, 2, v.shape)                       # odd low bits (discarded at 16 bit)
    return v.astype(packed_dtype(fmt))


@pytest.fixture(scope="module")
def lib():
    from ffmpeg_ffv2_amd import _lib, build
    build.build()
    lib = _lib.load()
    lib.ffv2amd_codec_encode_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.ffv2amd_ring_send.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_ssize_t), C.c_void_p, C.c_int64, C.c_uint]
    lib.ffv2amd_qpring_send.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_ssize_t), C.c_void_p, C.c_int64, C.c_uint]
    return lib


# ---- CPU: the restatement on hand-written pixels ----
def test_restatement_argb_bgr24_rgba64be_by_hand():
    # argb: A R G B per pixel
    argb = np.array([[[9, 1, 2, 3], [9, 4, 5, 6]], [[9, 7, 8, 10], [9, 11, 12, 13]]], np.uint8)
    g, b, r = packed_to_gbrp(argb, "argb", 8)
    assert (r == [[1, 4], [7, 11]]).all() and (g == [[2, 5], [8, 12]]).all() and (b == [[3, 6], [10, 13]]).all()
    # bgr24: B G R per pixel
    bgr = np.array([[[1, 2, 3], [4, 5, 6]], [[7, 8, 9], [10, 11, 12]]], np.uint8)
    g, b, r = packed_to_gbrp(bgr, "bgr24", 8)
    assert (b == [[1, 4], [7, 10]]).all() and (g == [[2, 5], [8, 11]]).all() and (r == [[3, 6], [9, 12]]).all()
    # rgba64be: R G B A, 16-bit big-endian, into gbrp12le: >> 4
    raw = bytes([0x12, 0x34, 0xAB, 0xCD, 0xFF, 0xFF, 0x00, 0x01,      # (0,0): R 0x1234 G 0xabcd B 0xffff A
                 0x00, 0x0F, 0x00, 0x10, 0x80, 0x00, 0xFF, 0xFF,      # (0,1)
                 0x01, 0x00, 0x02, 0x00, 0x03, 0x00, 0x00, 0x00,      # (1,0)
                 0xFF, 0xF0, 0x00, 0x00, 0x7F, 0xFF, 0x12, 0x34])     # (1,1)
    src = np.frombuffer(raw, ">u2").reshape(2, 2, 4)
    g, b, r = packed_to_gbrp(src, "rgba64be", 12)
    assert (r == [[0x123, 0x000], [0x010, 0xFFF]]).all()
    assert (g == [[0xABC, 0x001], [0x020, 0x000]]).all()
    assert (b == [[0xFFF, 0x800], [0x030, 0x7FF]]).all()
    # the same pixels little-endian give the same planes
    assert (packed_to_gbrp(src.astype("<u2"), "rgba64le", 12) == packed_to_gbrp(src, "rgba64be", 12)).all()


def test_restatement_shift_discards_low_bits():
    full = np.full((1, 2, 3), 0xFFFF, "<u2")
    assert (packed_to_gbrp(full, "rgb48le", 12) == 4095).all()
    assert (packed_to_gbrp(full, "rgb48le", 10) == 1023).all()
    a = np.array([[[0xABC0, 0x1230, 0x0010]]], "<u2")
    b = a | np.array([[[0x000F, 0x0007, 0x0001]]], "<u2")
    assert (packed_to_gbrp(a, "rgb48le", 12) == packed_to_gbrp(b, "rgb48le", 12)).all()
    assert packed_to_gbrp(b, "rgb48le", 12)[:, 0, 0].tolist() == [0x123, 0x001, 0xABC]


def test_padding_formats_are_their_alpha_forms():
    for pad, alpha in (("rgb0", "rgba"), ("bgr0", "bgra"), ("0rgb", "argb"), ("0bgr", "abgr")):
        src = packed_frame(pad, 3, 5, 7)
        assert (packed_to_gbrp(src, pad, 8) == packed_to_gbrp(src, alpha, 8)).all()


# ---- CPU: the C-ABI (fails without the feature) ----
def test_library_exports_and_null_checks(lib):
    for name in ("ffv2amd_frame_bytes_packed", "ffv2amd_convert_packed_device", "ffv2amd_encode_frame_packed",
                 "ffv2amd_qp_send_frame_packed", "ffv2amd_debug_packed_time", "ffv2amd_codec_encode_packed"):
        assert hasattr(lib, name), name
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    data = (C.c_void_p * 4)(p, None, None, None)
    ls = (C.c_ssize_t * 4)(16, 0, 0, 0)
    n = C.c_size_t(0)
    ms = C.c_float(0)
    for fmt, (fid, *_) in FMTS.items():
        assert lib.ffv2amd_frame_bytes_packed(None, fid) == 0
        assert lib.ffv2amd_convert_packed_device(None, 1, p, 16, 0, fid, p, None) == -22
        assert lib.ffv2amd_encode_frame_packed(None, p, 16, fid, 0, p, 64, C.byref(n)) == -22
        assert lib.ffv2amd_qp_send_frame_packed(None, p, 16, fid, 16, 0) == -22
        assert lib.ffv2amd_debug_packed_time(None, 1, p, 16, 0, fid, p, 1, C.byref(ms)) == -22
        assert lib.ffv2amd_ring_send(None, data, ls, None, 0, src_flags(fmt)) == -22
        assert lib.ffv2amd_qpring_send(None, data, ls, None, 0, src_flags(fmt)) == -22
        assert lib.ffv2amd_codec_encode_packed(None, None, None, fid, None) == -22
    from tests.codec_ctypes import Ctx
    ctx = Ctx()
    for extra in (FRAME_NV, FRAME_NV_VU, FRAME_YUV420, FRAME_YUV422):
        assert lib.ffv2amd_codec_send_frame(C.byref(ctx), None, src_flags("rgb24") | extra) == -22


def test_header_values_match_pixfmt():
    """include/ffv2_amd.h: the 18 source formats carry the AVPixelFormat values of the reference tree's
    libavutil/pixfmt.h (FF_API_VAAPI on: three VA-API entries before yuv420p16le), plus the flag and the field."""
    text = open(os.path.join(ROOT, "include", "ffv2_amd.h")).read()
    defs = dict(re.findall(r"#define\s+FFV2AMD_PIX_(\w+)\s+(\d+)", text))
    for fmt, (fid, *_) in FMTS.items():
        assert int(defs[fmt.upper()]) == fid, fmt
    assert re.search(r"#define\s+FFV2AMD_FRAME_PACKED\s+64u", text)
    assert re.search(r"#define\s+FFV2AMD_FRAME_SRC_FMT\(fmt\)\s+\(\(\(unsigned\)\(fmt\) & 0xffu\) << 16\)", text)


def test_python_format_table():
    from ffmpeg_ffv2_amd.encoder import PACKED_FORMATS, packed_frame_flags
    assert set(PACKED_FORMATS) == set(FMTS)
    for fmt, (fid, bps, nc, *_) in FMTS.items():
        assert PACKED_FORMATS[fmt] == (fid, bps, nc), fmt
        assert packed_frame_flags(fmt) == src_flags(fmt)


# ---- GPU ----
def _enc(w, h, pix, **kw):
    from ffmpeg_ffv2_amd import FFV2Encoder
    return FFV2Encoder(w, h, pix, device=0, **kw)


def _target(fmt):
    return "gbrp" if FMTS[fmt][1] == 1 else "gbrp12le"


GEOMS = [(1, 1), (9, 17), (129, 65), (2, 4097), (1080, 1920)]       # (h, w)


def _pitched(torch, frames, extra):
    """F packed frames in one device allocation, rows `row + extra` bytes apart, every padding byte 0x5A; -> the
    (F, h, w, C) strided view (element-typed when the pitch allows it, else None) and (buffer, pitch, frame stride)."""
    F = len(frames)
    h, w, nc = frames[0].shape
    isz = frames[0].dtype.itemsize
    row = w * nc * isz
    pitch = row + extra
    fstride = pitch * h + 48 + (extra & 1)
    host = np.full(F * fstride + 64, 0x5A, np.uint8)
    for f, a in enumerate(frames):
        host[f * fstride: f * fstride + pitch * h].reshape(h, pitch)[:, :row] = np.ascontiguousarray(a).view(np.uint8).reshape(h, row)
    return torch.from_numpy(host).to("cuda:0"), pitch, fstride


def _check_layout(enc, out, want, sentinel):
    """out: (F, frame_stride) uint8 from the device, prefilled with sentinel: the picture equals want[f], every other
    byte of the frame (row and plane padding) is still the sentinel."""
    i = enc.info
    got = enc.unpack_frames(out)
    for f in range(len(want)):
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, "frame %d: first mismatch at (plane, y, x) = %s: %d vs %d" % (
            f, bad[0], got[f][tuple(bad[0])], want[f][tuple(bad[0])])
        mask = np.ones(i.frame_stride, bool)
        row = i.width * (1 if i.depth == 8 else 2)
        for p in range(3):
            for y in range(i.height):
                o = p * i.plane_stride + y * i.row_pitch
                mask[o: o + row] = False
        assert (out[f][mask] == sentinel).all(), "frame %d: a padding byte was written" % f


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", list(FMTS))
def test_convert_packed_device_is_exact(fmt):
    """All geometries, tight / padded / odd source pitches (odd ones make most rows start unaligned: the per-pixel
    path), two frames a frame stride apart; 16-bit formats also into gbrp10le (>> 6)."""
    import torch
    from ffmpeg_ffv2_amd import _lib
    targets = ["gbrp"] if FMTS[fmt][1] == 1 else ["gbrp12le", "gbrp10le"]
    for pix in targets:
        for h, w in GEOMS:
            big = h * w > 100000
            enc = _enc(w, h, pix)
            src = [packed_frame(fmt, h * w + f, h, w, "noise" if f % 2 else "ramp") for f in range(1 if big else 2)]
            want = [packed_to_gbrp(a, fmt, DEPTH[pix]) for a in src]
            for extra in ([0] if big else [0, 64 + 13, 1]):
                buf, pitch, fstride = _pitched(torch, src, extra)
                out = torch.full((len(src), enc.info.frame_stride), 0xC3, dtype=torch.uint8, device="cuda:0")
                _lib.check(enc._lib.ffv2amd_convert_packed_device(enc._h, len(src), buf.data_ptr(), pitch, fstride,
                                                                  FMTS[fmt][0], out.data_ptr(), None), "convert")
                torch.cuda.synchronize()
                _check_layout(enc, out.cpu().numpy(), want, 0xC3)
            enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["rgb24", "bgra", "rgb48le", "rgba64be"])
def test_convert_packed_torch_views(fmt):
    """convert_packed on strided torch views (rows padded, frames one allocation apart) -> encode_batch_device."""
    import torch
    h, w = 72, 130
    enc = _enc(w, h, _target(fmt), max_batch=3)
    src = [packed_frame(fmt, 30 + f, h, w) for f in range(3)]
    nc, isz = FMTS[fmt][2], FMTS[fmt][1]
    buf, pitch, fstride = _pitched(torch, src, 16 * nc * isz)         # element-aligned padding
    tdt = torch.uint8 if isz == 1 else torch.int16
    assert fstride % isz == 0 and pitch % isz == 0
    view = torch.as_strided(buf.view(tdt), (3, h, w, nc), (fstride // isz, pitch // isz, nc, 1))
    assert not view.is_contiguous()
    frames = enc.convert_packed(view, fmt)
    got = enc.unpack_frames(frames.cpu().numpy())
    for f in range(3):
        assert (got[f] == packed_to_gbrp(src[f], fmt, DEPTH[_target(fmt)])).all(), f
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", list(FMTS))
def test_encode_frame_packed_equals_planar_and_oracle(oracle, fmt):
    pix = _target(fmt)
    h, w = 136, 201
    enc = _enc(w, h, pix)
    for seed, qp in ((0, 0), (1, 16)):
        src = packed_frame(fmt, seed, h, w, "ramp" if seed else "noise")
        planes = packed_to_gbrp(src, fmt, DEPTH[pix])
        try:
            want = oracle.encode(planes, pix, qp=qp)
        except RuntimeError:                                       # the reference would abort on this frame
            with pytest.raises(Exception):
                enc.encode2_packed(src, fmt, qp=qp)
            continue
        assert enc.encode2(planes, qp=qp) == want
        # a strided host frame (rows of a larger buffer)
        big = np.zeros((h, w + 7, src.shape[2]), src.dtype)
        big[:, :w] = src
        assert enc.encode2_packed(big[:, :w], fmt, qp=qp) == want, (fmt, qp)
    enc.close()


@pytest.mark.gpu
def test_refused_combinations(lib):
    from ffmpeg_ffv2_amd import FFV2Encoder
    from ffmpeg_ffv2_amd._lib import FFV2Error
    encs = {p: FFV2Encoder(64, 48, p) for p in ("gbrp", "gbrp10le", "gbrp12le", "yuv444p", "yuv444p12le", "gray")}
    z = np.zeros((48, 64 * 8), np.uint8)
    out = np.zeros(1 << 16, np.uint8)
    n = C.c_size_t(0)
    data = (C.c_void_p * 4)(z.ctypes.data, None, None, None)
    ls = (C.c_ssize_t * 4)(z.strides[0], 0, 0, 0)
    dbuf = 256                                                     # never dereferenced: refused first
    for pix, enc in encs.items():
        for fmt, (fid, bps, nc, *_) in list(FMTS.items()) + [("bogus%d" % v, (v, 1, 3)) for v in (0, 5, 73, 124, 255, 999)]:
            ok = (bps == 1 and pix == "gbrp" or bps == 2 and pix in ("gbrp10le", "gbrp12le")) and fmt in FMTS
            if ok:
                assert lib.ffv2amd_frame_bytes_packed(enc._h, fid) == 48 * 64 * nc * bps, (pix, fmt)
                continue
            assert lib.ffv2amd_frame_bytes_packed(enc._h, fid) == 0, (pix, fmt)
            assert lib.ffv2amd_convert_packed_device(enc._h, 1, dbuf, 4096, 0, fid, dbuf, None) == -22, (pix, fmt)
            assert lib.ffv2amd_encode_frame_packed(enc._h, z.ctypes.data, z.strides[0], fid, 0, out.ctypes.data, out.size,
                                                   C.byref(n)) == -22, (pix, fmt)
            assert lib.ffv2amd_qp_send_frame_packed(enc._h, z.ctypes.data, z.strides[0], fid, 16, 0) == -22, (pix, fmt)
            if fmt in FMTS:
                with pytest.raises(FFV2Error) as ei:
                    enc.packed_fmt(fmt)
                assert ei.value.code == -22
    # the flag: PACKED with a YUV source-layout bit is refused, on the ring and the qp ring
    g = encs["gbrp"]
    g.ring_open(1)
    for extra in (FRAME_NV, FRAME_NV_VU, FRAME_YUV420, FRAME_YUV422):
        assert lib.ffv2amd_ring_send(g._h, data, ls, None, 0, src_flags("rgb24") | extra) == -22
    assert lib.ffv2amd_ring_send(g._h, data, ls, None, 0, src_flags("rgb48le")) == -22
    assert lib.ffv2amd_ring_send(g._h, data, ls, None, 0, FRAME_PACKED) == -22          # format 0: unknown
    assert lib.ffv2amd_ring_pending(g._h) == 0
    g.ring_close()
    g.qpring_open(16, 2)
    for extra in (FRAME_NV, FRAME_NV_VU, FRAME_YUV420, FRAME_YUV422):
        assert lib.ffv2amd_qpring_send(g._h, data, ls, None, 0, src_flags("rgb24") | extra) == -22
    assert lib.ffv2amd_qpring_send(g._h, data, ls, None, 0, src_flags("rgba64le")) == -22
    assert lib.ffv2amd_qpring_pending(g._h) == 0
    g.qpring_close()
    for e in encs.values():
        e.close()


@pytest.mark.gpu
def test_ring_mixes_packed_and_planar(oracle):
    """gbrp and gbrp12le rings get planar frames and packed frames -- pageable, page-locked (pinned_frames_packed) and
    FFV2AMD_FRAME_REGISTER -- in one stream: packets in send order, each the planar path's / the oracle's."""
    from ffmpeg_ffv2_amd import frames as synth
    W, H = 640, 360
    for pix, fmts in (("gbrp", ["rgb24", "bgra", "0rgb", "abgr", "bgr24"]), ("gbrp12le", ["rgb48le", "rgba64be", "bgr48be"])):
        depth = DEPTH[pix]
        enc = _enc(W, H, pix)
        enc.ring_open(3)
        planar = synth.make("S2", 1, 3, H, W, depth)
        sends = [("planar", planar, {})]
        for k, fmt in enumerate(fmts):
            a, b = packed_frame(fmt, 40 + k, H, W, "ramp"), packed_frame(fmt, 50 + k, H, W)
            pin = enc.pinned_frames_packed(1, fmt)[0]
            pin[:] = b
            sends += [(fmt, a, {}), (fmt, pin, {"pinned": True}), (fmt, b, {"register": True}), ("planar", planar, {}),
                      (fmt, a, {"register": True})]
        want_planar = oracle.encode(planar, pix)
        got, wanted = [], []
        for t, (kind, fr, kw) in enumerate(sends):
            if kind == "planar":
                send = lambda: enc.ring_send(fr, tag=t)                 # noqa: E731
                wanted.append(want_planar)
            else:
                send = lambda: enc.ring_send_packed(fr, kind, tag=t, **kw)   # noqa: E731
                wanted.append(oracle.encode(packed_to_gbrp(fr, kind, depth), pix))
            while not send():
                got.append(enc.ring_receive())
        while enc.ring_pending():
            got.append(enc.ring_receive())
        assert [g[0] for g in got] == list(range(len(sends)))
        for t, (tag, pk) in enumerate(got):
            assert pk == wanted[t], (pix, t, sends[t][0])
        enc.ring_close()
        enc.free_pinned()
        enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pix", ["gbrp", "gbrp12le"])
def test_qpring_batch_mixes_packed_and_planar(oracle, pix):
    from ffmpeg_ffv2_amd import frames as synth
    W, H, qp = 200, 136, 16
    depth = DEPTH[pix]
    enc = _enc(W, H, pix)
    enc.qpring_open(qp, 4)
    fmts = ["rgb24", "bgra", "0bgr", "argb"] if depth == 8 else ["rgb48le", "bgra64be", "rgba64le", "bgr48be"]
    sends = [("planar", synth.make("S1", 2, 3, H, W, depth))]
    sends += [(f, packed_frame(f, 10 + k, H, W, "ramp")) for k, f in enumerate(fmts)]
    sends += [(fmts[0], packed_frame(fmts[0], 30, H, W, "ramp")), ("planar", synth.make("S2", 3, 3, H, W, depth)),
              (fmts[1], packed_frame(fmts[1], 31, H, W, "ramp"))]
    for t, (kind, fr) in enumerate(sends):
        assert enc.qpring_send(fr, tag=t, packed=None if kind == "planar" else kind)
    assert enc.qpring_flush()
    for t, (kind, fr) in enumerate(sends):
        conv = fr if kind == "planar" else packed_to_gbrp(fr, kind, depth)
        try:
            want = oracle.encode(conv, pix, qp=qp)
        except RuntimeError:
            with pytest.raises(Exception):
                enc.qpring_receive()
            continue
        assert enc.qpring_receive() == (t, want), (t, kind)
    enc.qpring_close()
    enc.close()


def _drive(lib, ctx, frames, flags):
    from tests.codec_ctypes import Packet, frame_of
    out, sent = [], 0
    while len(out) < len(frames):
        while sent < len(frames):
            r = lib.ffv2amd_codec_send_frame(C.byref(ctx), C.byref(frame_of([frames[sent]], 500 + sent)), flags)
            if r == -11:
                break
            assert r == 0, r
            sent += 1
        if sent == len(frames):
            assert lib.ffv2amd_codec_send_frame(C.byref(ctx), None, 0) in (0, -11)
        pkt = Packet()
        r = lib.ffv2amd_codec_receive_packet(C.byref(ctx), C.byref(pkt), 1)
        if r == -11:
            continue
        if r < 0:
            out.append((None, r))
            continue
        out.append((pkt.pts, bytes(pkt.data[: pkt.size])))
        lib.ffv2amd_packet_unref(C.byref(pkt))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("qp,per_call", [(0, 0), (16, 0), (16, 3)])
@pytest.mark.parametrize("fmt", ["rgb24", "bgr0", "rgba64be"])
def test_packed_frames_through_send_frame(oracle, lib, devices, qp, per_call, fmt):
    from tests.codec_ctypes import make_ctx
    W, H = 322, 130
    pix = _target(fmt)
    src = [packed_frame(fmt, 70 + n, H, W, "noise" if n % 2 else "ramp") for n in range(5)]
    ctx = make_ctx(W, H, PIX[pix], qp=qp, ring_depth=2, devices=devices, qp_frames_per_call=per_call)
    assert lib.ffv2amd_codec_init(C.byref(ctx)) == 0
    got = _drive(lib, ctx, src, src_flags(fmt))
    for n, (pts, pk) in enumerate(got):
        try:
            want = (500 + n, oracle.encode(packed_to_gbrp(src[n], fmt, DEPTH[pix]), pix, qp=qp))
        except RuntimeError:
            want = (None, -1)
        assert (pts, pk) == want, n
    assert lib.ffv2amd_codec_close(C.byref(ctx)) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bgra", "rgb48be"])
def test_codec_encode_packed(oracle, lib, fmt):
    from tests.codec_ctypes import Packet, frame_of, make_ctx
    W, H = 96, 70
    pix = _target(fmt)
    for qp in (0, 16):
        ctx = make_ctx(W, H, PIX[pix], qp=qp)
        assert lib.ffv2amd_codec_init(C.byref(ctx)) == 0
        src = packed_frame(fmt, 5 + qp, H, W, "ramp")
        pkt, got = Packet(), C.c_int(0)
        r = lib.ffv2amd_codec_encode_packed(C.byref(ctx), C.byref(pkt), C.byref(frame_of([src], 9)), FMTS[fmt][0], C.byref(got))
        try:
            want = oracle.encode(packed_to_gbrp(src, fmt, DEPTH[pix]), pix, qp=qp)
        except RuntimeError:
            assert r < 0
            want = None
        if want is not None:
            assert r == 0 and got.value == 1 and pkt.pts == 9 and bytes(pkt.data[: pkt.size]) == want, (fmt, qp)
            lib.ffv2amd_packet_unref(C.byref(pkt))
        assert lib.ffv2amd_codec_close(C.byref(ctx)) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["rgb24", "bgr0", "rgb48le", "bgra64be"])
def test_cli_packed_sync_and_async_match_planar_cli(tmp_path, fmt):
    subprocess.run(["make", "-s", "-C", ROOT, "examples/ffv2enc_cli"], check=True)
    cli = os.path.join(ROOT, "examples", "ffv2enc_cli")
    W, H = 320, 240
    pix = _target(fmt)
    src = [packed_frame(fmt, n, H, W, "ramp") for n in range(4)]
    raw = tmp_path / ("in.%s" % fmt)
    raw.write_bytes(b"".join(np.ascontiguousarray(f).tobytes() for f in src))
    planar = tmp_path / ("in.%s" % pix)
    planar.write_bytes(b"".join(packed_to_gbrp(f, fmt, DEPTH[pix]).astype(np.uint8 if pix == "gbrp" else "<u2").tobytes()
                                for f in src))
    for qp in (0, 16):
        ref = tmp_path / ("planar%d.ffv2" % qp)
        r = subprocess.run(["timeout", "-k", "10", "300", cli, str(W), str(H), pix, str(planar), str(ref), str(qp), "0"],
                           capture_output=True, text=True)
        if r.returncode != 0:                                      # a frame the reference would abort on
            assert qp > 0, r.stderr
            continue
        want = ref.read_bytes()
        assert len(want) > 0
        for extra in ([], ["--async", "3"]):
            out = tmp_path / ("out%d_%d.ffv2" % (qp, len(extra)))
            r = subprocess.run(["timeout", "-k", "10", "300", cli, str(W), str(H), fmt, str(raw), str(out), str(qp), "0"] + extra,
                               capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert out.read_bytes() == want, (qp, extra)
    r = subprocess.run(["timeout", "-k", "10", "120", cli, str(W), str(H), fmt, str(raw), str(tmp_path / "x.ffv2"), "--no-convert"],
                       capture_output=True, text=True)
    assert r.returncode == 2
