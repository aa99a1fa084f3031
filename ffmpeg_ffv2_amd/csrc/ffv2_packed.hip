// ffv2_packed.hip -- packed RGB sources (rgb24, bgra, rgb48le, ...) -> the encoder's gbrp* planes.
//
// ffv2's encode2() takes planar RGB only (gbrp, gbrp10le, gbrp12le: ffv2enc.c:596-601).  Handed a packed RGB
// source the reference tool chain picks gbrp for 8-bit and gbrp12le for 16-bit sources
// (av_find_best_pix_fmt_of_2 / get_pix_fmt_score, libavutil/pixdesc.c:2714-2873) and converts with one of
// libswscale's *unscaled* converters, which are exact:
//   8 bit   rgbToPlanarRgbWrapper (libswscale/swscale_unscaled.c:1147-1190, dispatched at :2015-2017) with
//           packedtogbr24p (:1118-1146): rgb24 bgr24 rgba bgra argb abgr -> gbrp.  A byte permutation:
//           G -> plane 0, B -> plane 1, R -> plane 2; argb / abgr skip the first byte of every pixel.
//   16 bit Rgb16ToPlanarRgb16Wrapper (:674-732, dispatched at :1987-1999) with packed16togbra16 (:540-672):
//           rgb48 bgr48 rgba64 bgra64, LE and BE -> gbrp10le / gbrp12le.  Big-endian samples are byte-swapped,
//           every sample is shifted right by 16 - depth, alpha is dropped.
// rgb0 / bgr0 / 0rgb / 0bgr reach rgbToPlanarRgbWrapper's default: branch, which writes nothing: there is no
// reference output.  DELIBERATE DEVIATION: they are converted as rgba / bgra / argb / abgr, the padding byte
// ignored.
//
// Device part: a streaming de-interleave, one launch for a batch of frames.  The unit of work is 16 bytes of
// one output row in each of the three planes (16 pixels at 8 bit, 8 at 16 bit), read as 3 or 4 dwordx4 loads
// (16 * C bytes of the packed row); the bytes of each output dword are picked with v_perm_b32.  Units are
// numbered along rows, rows along frames; lane l of a wave takes units base + g * 64 + l, so each dwordx4 store
// of a wave writes 1 KB of one plane row back to back (whole 128-byte lines).  A unit whose source is not
// 16-byte aligned (odd pitches, odd base addresses) or that reaches past the row's last pixel goes pixel by
// pixel with byte loads, in the same launch; no plane is written past a row's last sample.
#include "ffv2_kernels.h"

namespace {

struct PackedArgs {
    const uint8_t *src;        // frame 0's packed rows, src_pitch apart; frame f at + f * src_frame_stride
    size_t src_pitch, src_frame_stride;
    uint8_t *dst;
    size_t frame_stride, plane_stride, row_pitch;
    int w, h;
    uint32_t units_row;        // units per row
    uint32_t units;            // units_row * h * nframes
    int shift;                 // 16-bit sources: >> (16 - depth)
};

// the dword made of bytes o0..o3 (offsets into w[]) -- compile-time offsets after unrolling: two v_perm_b32 and an or
__device__ __forceinline__ uint32_t pick4(const uint32_t *w, int o0, int o1, int o2, int o3)
{
    const uint32_t lo = __builtin_amdgcn_perm(w[o1 >> 2], w[o0 >> 2],
                                              (uint32_t)(o0 & 3) | (uint32_t)(4 + (o1 & 3)) << 8 | 0x0c0c0000u);
    const uint32_t hi = __builtin_amdgcn_perm(w[o3 >> 2], w[o2 >> 2],
                                              0x0c0cu | (uint32_t)(o2 & 3) << 16 | (uint32_t)(4 + (o3 & 3)) << 24);
    return lo | hi;
}

// source component (after a leading byte) of output plane p: gbrp order G, B, R
template <bool BGR> __device__ __forceinline__ constexpr int comp_of_plane(int p)
{
    return p == 0 ? 1 : p == 1 ? (BGR ? 0 : 2) : (BGR ? 2 : 0);
}

// BPS bytes per sample, C components per pixel, BGR order, LEAD: a padding / alpha byte first, SWAP: big-endian
template <int BPS, int C, bool BGR, bool LEAD, bool SWAP>
__global__ __launch_bounds__(256) void ffv2_packed_kernel(const PackedArgs a)
{
    constexpr int PX = 16 / BPS;             // pixels per unit
    constexpr int NW = 4 * C;                // source dwords per unit
    constexpr int G = BPS;                   // units per lane: 16 pixels a lane
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6;
#pragma unroll
    for (int gi = 0; gi < G; gi++) {
        const uint32_t u = (wave * G + gi) * 64u + lane;
        if (u >= a.units) return;
        const uint32_t row = u / a.units_row, ux = u - row * a.units_row;
        const uint32_t f = row / (uint32_t)a.h, y = row - f * (uint32_t)a.h;
        const int x0 = (int)ux * PX;
        const uint8_t *s = a.src + (size_t)f * a.src_frame_stride + (size_t)y * a.src_pitch + (size_t)x0 * (C * BPS);
        uint8_t *d = a.dst + (size_t)f * a.frame_stride + (size_t)y * a.row_pitch + (size_t)x0 * BPS;
        if (x0 + PX <= a.w && ((((uintptr_t)s) | ((uintptr_t)d)) & 15) == 0) {
            uint32_t w[NW];
#pragma unroll
            for (int i = 0; i < C; i++) {
                const uint4 q = reinterpret_cast<const uint4 *>(s)[i];
                w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
            }
#pragma unroll
            for (int p = 0; p < 3; p++) {
                const int c = comp_of_plane<BGR>(p) + (LEAD ? 1 : 0);
                uint32_t o[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (BPS == 1) {
                        o[k] = pick4(w, (4 * k) * C + c, (4 * k + 1) * C + c, (4 * k + 2) * C + c, (4 * k + 3) * C + c);
                    } else {
                        const int b0 = ((2 * k) * C + c) * 2, b1 = ((2 * k + 1) * C + c) * 2;
                        const uint32_t v = SWAP ? pick4(w, b0 + 1, b0, b1 + 1, b1) : pick4(w, b0, b0 + 1, b1, b1 + 1);
                        o[k] = ((v & 0xffffu) >> a.shift) | ((v >> 16) >> a.shift) << 16;
                    }
                }
                *reinterpret_cast<uint4 *>(d + (size_t)p * a.plane_stride) = make_uint4(o[0], o[1], o[2], o[3]);
            }
        } else {
            const int n = a.w - x0 < PX ? a.w - x0 : PX;
            for (int i = 0; i < n; i++) {
                const uint8_t *px = s + i * (C * BPS) + (LEAD ? 1 : 0);
#pragma unroll
                for (int p = 0; p < 3; p++) {
                    const uint8_t *q = px + comp_of_plane<BGR>(p) * BPS;
                    if (BPS == 1) {
                        d[(size_t)p * a.plane_stride + i] = q[0];
                    } else {
                        const uint32_t v = SWAP ? (uint32_t)q[0] << 8 | q[1] : (uint32_t)q[1] << 8 | q[0];
                        reinterpret_cast<uint16_t *>(d + (size_t)p * a.plane_stride)[i] = (uint16_t)(v >> a.shift);
                    }
                }
            }
        }
    }
}

template <int BPS, int C, bool BGR, bool LEAD, bool SWAP>
hipError_t launch(const PackedArgs &a, hipStream_t s)
{
    const uint64_t lanes = ((uint64_t)a.units + BPS - 1) / BPS;
    const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
    hipLaunchKernelGGL((ffv2_packed_kernel<BPS, C, BGR, LEAD, SWAP>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t ffv2_launch_packed(const FFV2Geom &g, int nframes, const FFV2PackedSrc &src, uint8_t *dst, hipStream_t s)
{
    const int bps = g.bytes_per_sample;
    if (g.planes != 3 || bps != src.bps || (src.nc != 3 && src.nc != 4) || nframes < 1) return hipErrorInvalidValue;
    if ((bps == 2 && src.lead) || (bps == 1 && src.swap) || (src.lead && src.nc != 4)) return hipErrorInvalidValue;
    PackedArgs a{};
    a.src = src.src; a.src_pitch = src.pitch; a.src_frame_stride = src.frame_stride; a.dst = dst;
    a.frame_stride = g.frame_stride; a.plane_stride = g.plane_stride; a.row_pitch = g.row_pitch;
    a.w = g.width; a.h = g.height;
    const uint32_t px = (uint32_t)(16 / bps);
    a.units_row = ((uint32_t)g.width + px - 1) / px;
    const uint64_t units = (uint64_t)a.units_row * (uint64_t)g.height * (uint64_t)nframes;
    if (units > 0x7fffffffull) return hipErrorInvalidValue;
    a.units = (uint32_t)units;
    a.shift = bps == 2 ? 16 - g.depth : 0;
    if (bps == 1) {
        if (src.nc == 3) return src.bgr ? launch<1, 3, true, false, false>(a, s) : launch<1, 3, false, false, false>(a, s);
        if (src.lead) return src.bgr ? launch<1, 4, true, true, false>(a, s) : launch<1, 4, false, true, false>(a, s);
        return src.bgr ? launch<1, 4, true, false, false>(a, s) : launch<1, 4, false, false, false>(a, s);
    }
#define PK16(C)                                                                                              \
    do {                                                                                                     \
        if (src.bgr) return src.swap ? launch<2, C, true, false, true>(a, s) : launch<2, C, true, false, false>(a, s); \
        return src.swap ? launch<2, C, false, false, true>(a, s) : launch<2, C, false, false, false>(a, s);   \
    } while (0)
    if (src.nc == 3) PK16(3);
    PK16(4);
#undef PK16
}
