#!/usr/bin/env python3
"""Packed RGB front end on the MI355X: one JSON line for 3840x2160 rgb48le -> gbrp12le, bgra -> gbrp and rgb24 -> gbrp.

  kernel : ffv2amd_convert_packed_device (ffv2amd_debug_packed_time: device events, one warm-up launch) over an 8-frame
           batch and over single frames -- us per frame and achieved bytes/s from the bytes the step needs (the packed
           source read, three gbrp* planes written) against the 8 TB/s HBM peak;
  ring   : host frames in, host packets out through the asynchronous ring (depth 4), page-locked frames, for at least
           --seconds: each packed form next to the planar gbrp* form of the same depth, measured in the same run;
  device : device-resident packed frames -> packets in HBM (convert_packed + encode_batch_device, batches of 4): Gpix/s.
Needs the GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ffmpeg_ffv2_amd import FFV2Encoder, frames as synth  # noqa: E402
from ffmpeg_ffv2_amd import _lib  # noqa: E402
from ffmpeg_ffv2_amd.encoder import PACKED_FORMATS  # noqa: E402

HBM_PEAK = 8e12
CASES = [("rgb48le", "gbrp12le"), ("bgra", "gbrp"), ("rgb24", "gbrp")]
W, H = 3840, 2160


def sources(fmt, nframes):
    """nframes tight packed frames on the device (any sample values: every one is in range after the shift)."""
    _, bps, nc = PACKED_FORMATS[fmt]
    g = torch.Generator(device="cuda:0").manual_seed(1)
    n = nframes * H * W * nc * bps
    return torch.randint(0, 256, (n,), dtype=torch.int32, device="cuda:0", generator=g).to(torch.uint8)


def kernel_rate(fmt, pix, nframes, reps):
    enc = FFV2Encoder(W, H, pix, device=0, max_batch=1)
    fid, bps, nc = PACKED_FORMATS[fmt]
    src = sources(fmt, nframes)
    dst = torch.empty((nframes, enc.info.frame_stride), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    pitch = W * nc * bps
    ms = C.c_float(0)
    _lib.check(enc._lib.ffv2amd_debug_packed_time(enc._h, nframes, src.data_ptr(), pitch, pitch * H, fid, dst.data_ptr(),
                                                  reps, C.byref(ms)), "ffv2amd_debug_packed_time")
    moved = (enc.frame_bytes_packed(fmt) + 3 * W * H * bps) * nframes
    enc.close()
    return {"us_per_frame": round(ms.value * 1e3 / nframes, 2), "bytes_per_frame": moved // nframes,
            "TB_per_s": round(moved / (ms.value * 1e-3) / 1e12, 3),
            "fraction_of_8TBps": round(moved / (ms.value * 1e-3) / HBM_PEAK, 3), "frames_per_launch": nframes, "reps": reps}


def ring_rate(fmt, pix, host, form, seconds, depth=4):
    enc = FFV2Encoder(W, H, pix, device=0, max_batch=1)
    enc.ring_open(depth)
    nsrc = len(host)
    if form == "planar":
        src = enc.pinned_frames(nsrc)
        for n in range(nsrc):
            src[n][:] = host[n]
        send = lambda n: enc.ring_send(src[n % nsrc], tag=n, pinned=True)                    # noqa: E731
        frame_bytes = 3 * W * H * enc.dtype.itemsize
    else:
        src = enc.pinned_frames_packed(nsrc, fmt)
        shift = 16 - enc.info.depth if enc.info.depth > 8 else 0
        for d, f in zip(src, host):                  # G, B, R planes -> R, G, B(, A) pixels of the same picture
            d[:, :, 0], d[:, :, 1], d[:, :, 2] = f[2] << shift, f[0] << shift, f[1] << shift
            if fmt == "bgra":
                d[:, :, 0], d[:, :, 2] = f[1], f[2]
            if d.shape[2] == 4:
                d[:, :, 3] = 255
        send = lambda n: enc.ring_send_packed(src[n % nsrc], fmt, tag=n, pinned=True)        # noqa: E731
        frame_bytes = enc.frame_bytes_packed(fmt)

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


def device_rate(fmt, pix, seconds, batch=4):
    enc = FFV2Encoder(W, H, pix, device=0, max_batch=batch)
    _, bps, nc = PACKED_FORMATS[fmt]
    src = sources(fmt, batch).view(torch.uint8 if bps == 1 else torch.int16).view(batch, H, W, nc)
    frames = torch.empty((batch, enc.info.frame_stride), dtype=torch.uint8, device="cuda:0")
    outs = [enc.alloc_packets(batch) for _ in range(2)]
    for k in range(2):                                             # warm-up
        enc.encode_batch_device(enc.convert_packed(src, fmt, out=frames), out=outs[k])
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for k in range(8):
            enc.encode_batch_device(enc.convert_packed(src, fmt, out=frames), out=outs[k & 1])
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
    assert torch.cuda.is_available(), "bench_packed needs the MI355X"
    out = {"metric": "packed RGB front end (conversion exact; *0 formats a deliberate deviation)", "geometry": "%dx%d" % (W, H)}
    for fmt, pix in CASES:
        r = {"target": pix, "kernel_batch8": kernel_rate(fmt, pix, 8, a.reps),
             "kernel_single": kernel_rate(fmt, pix, 1, a.reps)}
        if not a.skip_ring:
            depth = 12 if pix == "gbrp12le" else 8
            host = [synth.make("S1" if n % 2 == 0 else "S2", n, 3, H, W, depth) for n in range(4)]
            ring = {"planar": ring_rate(fmt, pix, host, "planar", a.seconds), fmt: ring_rate(fmt, pix, host, fmt, a.seconds)}
            ring["packed_gpix_vs_planar"] = round(ring[fmt]["gpix_per_s"] / ring["planar"]["gpix_per_s"], 3)
            ring["packed_bytes_vs_planar"] = round(ring[fmt]["GB_per_s"] / ring["planar"]["GB_per_s"], 3)
            r["ring_depth4_pinned"] = ring
            r["device_resident_to_packets"] = device_rate(fmt, pix, a.seconds)
        out[fmt] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
