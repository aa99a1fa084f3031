#!/usr/bin/env python3
"""Semi-planar front end on the MI355X: one JSON line for 3840x2160 p010le and 1920x1080 nv12.

  kernel : ffv2amd_convert_nv_device, luma included (ffv2amd_debug_nv_time: device events, one warm-up launch) over
           an 8-frame batch of pitched surfaces -- us per frame and achieved bytes/s from the bytes the step needs
           (source Y + interleaved chroma read, three 4:4:4 planes written) against the 8 TB/s HBM peak; next to it
           the planar 4:2:0 path on the same geometry (ffv2amd_upconvert_420_device: luma row copy + chroma kernel,
           timed with device events around `reps` launches);
  ring   : host frames in, host packets out through the asynchronous ring (depth 4), page-locked frames, for at least
           --seconds: the semi-planar form next to yuv420p* (same bytes over PCIe);
  device : device-resident pitched surfaces -> packets in HBM (convert_nv + encode_batch_device, batches of 4): Gpix/s.
Needs the GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ffmpeg_ffv2_amd import FFV2Encoder, frames as synth  # noqa: E402
from ffmpeg_ffv2_amd import _lib  # noqa: E402

HBM_PEAK = 8e12
CASES = [("p010le", "yuv444p10le", 3840, 2160), ("nv12", "yuv444p", 1920, 1080)]


def surfaces(enc, fmt, nframes, pad=256):
    """nframes decoder-style surfaces (Y rows, then chroma rows, pitch = row + pad bytes) as strided torch views."""
    (h, w), (ch, c2) = enc.nv_shape(fmt)
    isz = enc.dtype.itemsize
    yp, up = w + pad // isz, c2 + pad // isz
    per = yp * h + up * ch
    g = torch.Generator(device="cuda:0").manual_seed(1)
    buf = torch.randint(0, 1 << 16 if isz == 2 else 256, (nframes, per), dtype=torch.int32, device="cuda:0", generator=g)
    buf = buf.to(torch.int16 if isz == 2 else torch.uint8)
    y = buf[:, : yp * h].unflatten(1, (h, yp))[:, :, :w]
    uv = buf[:, yp * h:].unflatten(1, (ch, up))[:, :, :c2]
    return y, uv, buf


def kernel_rate(fmt, fmt444, W, H, nframes, reps):
    enc = FFV2Encoder(W, H, fmt444, device=0, max_batch=1)
    lib = enc._lib
    isz = enc.dtype.itemsize
    y, uv, _ = surfaces(enc, fmt, nframes)
    dst = torch.empty((nframes, enc.info.frame_stride), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ms = C.c_float(0)
    _lib.check(lib.ffv2amd_debug_nv_time(enc._h, nframes, y.data_ptr(), y.stride(1) * isz, uv.data_ptr(), uv.stride(1) * isz,
                                         y.stride(0) * isz, enc.nv_flags(fmt), dst.data_ptr(), reps, C.byref(ms)),
               "ffv2amd_debug_nv_time")
    src_bytes = enc.frame_bytes_nv(fmt)
    moved = (src_bytes + 3 * W * H * isz) * nframes
    nv = {"us_per_frame": round(ms.value * 1e3 / nframes, 2), "bytes_per_frame": moved // nframes,
          "TB_per_s": round(moved / (ms.value * 1e-3) / 1e12, 3),
          "fraction_of_8TBps": round(moved / (ms.value * 1e-3) / HBM_PEAK, 3)}
    # planar 4:2:0 on the same geometry: tightly packed yuv420p* frames
    per = lib.ffv2amd_frame_bytes_420(enc._h)
    src = torch.randint(0, 1 << 10 if isz == 2 else 256, (nframes * per // isz,), dtype=torch.int32,
                        device="cuda:0").to(torch.int16 if isz == 2 else torch.uint8).view(torch.uint8)
    stream = torch.cuda.current_stream().cuda_stream
    launch = lambda: _lib.check(lib.ffv2amd_upconvert_420_device(enc._h, nframes, src.data_ptr(), dst.data_ptr(),  # noqa: E731
                                                                  C.c_void_p(stream)), "ffv2amd_upconvert_420_device")
    launch()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        launch()
    b.record()
    b.synchronize()
    pms = a.elapsed_time(b) / reps
    pmoved = (per + 3 * W * H * isz) * nframes
    planar = {"us_per_frame": round(pms * 1e3 / nframes, 2), "TB_per_s": round(pmoved / (pms * 1e-3) / 1e12, 3)}
    enc.close()
    return {"semi_planar": nv, "planar_420": planar, "nv_vs_planar_time": round(ms.value / pms, 3),
            "frames_per_launch": nframes, "reps": reps}


def ring_rate(fmt, fmt444, W, H, host444, form, seconds, depth=4):
    enc = FFV2Encoder(W, H, fmt444, device=0, max_batch=1)
    enc.ring_open(depth)
    nsrc = len(host444)
    if form == "420":
        src = enc.pinned_frames_420(nsrc)
        for d, f in zip(src, host444):
            d[0][:], d[1][:], d[2][:] = f[0], f[1][::2, ::2], f[2][::2, ::2]
        send = lambda n: enc.ring_send_420(*src[n % nsrc], tag=n, pinned=True)            # noqa: E731
    else:
        src = enc.pinned_frames_nv(nsrc, fmt)
        sh = 6 if fmt == "p010le" else 0
        for d, f in zip(src, host444):
            d[0][:] = f[0] << sh
            d[1][:, 0::2], d[1][:, 1::2] = f[1][::2, ::2] << sh, f[2][::2, ::2] << sh
        send = lambda n: enc.ring_send_nv(*src[n % nsrc], fmt, tag=n, pinned=True)         # noqa: E731
    frame_bytes = (W * H + 2 * ((W + 1) // 2) * ((H + 1) // 2)) * enc.dtype.itemsize

    def run(until=None, count=None):
        sent, got = 0, 0
        t0 = time.perf_counter()
        while True:
            stop = (count is not None and sent >= count) or (until is not None and time.perf_counter() - t0 >= until)
            if not stop and send(sent):
                sent += 1
                continue
            if got == sent:
                break
            tag, _ = enc.ring_receive(wait=True)
            assert tag == got, "ring delivered out of order"
            got += 1
        return time.perf_counter() - t0, got

    run(count=2 * depth)
    dt, n = run(until=seconds)
    enc.ring_close()
    enc.free_pinned()
    enc.close()
    return {"gpix_per_s": round(W * H * n / dt / 1e9, 2), "GB_per_s": round(frame_bytes * n / dt / 1e9, 1), "frames": n,
            "seconds": round(dt, 3)}


def device_rate(fmt, fmt444, W, H, seconds, batch=4):
    enc = FFV2Encoder(W, H, fmt444, device=0, max_batch=batch)
    y, uv, _ = surfaces(enc, fmt, batch)
    sh = 6 if fmt == "p010le" else 0                               # keep samples within the depth (no wide rerun)
    if sh:
        y.bitwise_and_(0x7fc0); uv.bitwise_and_(0x7fc0)
    frames = torch.empty((batch, enc.info.frame_stride), dtype=torch.uint8, device="cuda:0")
    outs = [enc.alloc_packets(batch) for _ in range(2)]
    for k in range(2):                                             # warm-up
        enc.encode_batch_device(enc.convert_nv(y, uv, fmt, out=frames), out=outs[k])
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for k in range(8):
            enc.encode_batch_device(enc.convert_nv(y, uv, fmt, out=frames), out=outs[k & 1])
            n += batch
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = outs[0][2].cpu().numpy()
    enc.close()
    return {"gpix_per_s": round(W * H * n / dt / 1e9, 2), "frames": n, "batch": batch, "seconds": round(dt, 3),
            "status_ok": bool((st >= 0).all())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--skip-ring", action="store_true", help="the kernels only (for a profiler run)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_nv needs the MI355X"
    out = {"metric": "semi-planar front end (parity unpinned)"}
    for fmt, fmt444, W, H in CASES:
        r = {"geometry": "%dx%d" % (W, H), "kernel": kernel_rate(fmt, fmt444, W, H, 8, a.reps)}
        if not a.skip_ring:
            depth = 10 if fmt == "p010le" else 8
            host = [synth.make("S1" if n % 2 == 0 else "S2", n, 3, H, W, depth) for n in range(4)]
            ring = {"420": ring_rate(fmt, fmt444, W, H, host, "420", a.seconds),
                    fmt: ring_rate(fmt, fmt444, W, H, host, fmt, a.seconds)}
            ring["nv_gpix_vs_420"] = round(ring[fmt]["gpix_per_s"] / ring["420"]["gpix_per_s"], 3)
            r["ring_depth4_pinned"] = ring
            r["device_resident_to_packets"] = device_rate(fmt, fmt444, W, H, a.seconds)
        out[fmt] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
